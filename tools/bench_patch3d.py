"""Timing of the patch sampling passes at the pipeline's real shape: one synthetic instance, an int16 image and nine masks of
140 x 512 x 512, two patches of 64 x 192 x 192.

Centre pick (ctseg_patch_centres, P = 2: the count pass and the select pass), beside what the parent commit has for the counts,
``torch.count_nonzero(masks, dim=(1, 2, 3))``, and beside a ``copy_`` of the mask block, whose bandwidth gives the bytes floor of
the count pass (mask bytes over the bytes per second, read plus written, that the copy reaches).  The entry's two launches are timed together with
device events; their split (count, select) comes from a ``torch.profiler`` pass of its own over a few calls, after the timed
rounds, and is null where the profiler reports no kernels.

Crop pass, per patch (nine masks written beside the label map and hist): the identity crop and the degree-1 extreme rotation
(trilinear) through ctseg_patch3d_to_hwd, beside ctseg_augment3d_to_hwd on the same instance with the same output grid and matrix
family, and beside the torch restatement of the identity crop (slice, permute, ``contiguous``, window; image and masks).

Preallocated outputs, one process, device events around ``--reps`` back-to-back calls; the variants alternate over ``--rounds``
rounds and the median round is reported with the spread (min, max).  A figure is one call (enqueue + kernels), not a kernel time.

  python tools/bench_patch3d.py --out profiles/patch3d.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd.volumetric import transforms as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(140, 512, 512))
    ap.add_argument("--patch", type=int, nargs=3, default=(64, 192, 192))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    K, P = 9, 2
    D, H, W = a.shape
    Pd, Ph, Pw = a.patch
    g = torch.Generator().manual_seed(12342)
    image = (torch.randn(D, H, W, generator=g) * 400).to(torch.int16).to(dev)
    masks = torch.zeros(K, D, H, W, dtype=torch.uint8)
    for k in range(K):
        masks[k, 10 + 10 * k:50 + 10 * k, 60 + 40 * k:160 + 40 * k, 80 + 30 * k:260 + 30 * k] = 1
    want_counts = masks.reshape(K, -1).sum(1, dtype=torch.int64)
    masks = masks.to(dev)
    masks_copy = torch.empty_like(masks)
    n = Pd * Ph * Pw

    # ---- centre pick ----
    need = nat.lib().ctseg_patch_centres_workspace(K, D, H, W)
    nb = (need // 4 - 16) // K
    ws = torch.full((need // 4,), -1, dtype=torch.int32, device=dev)
    centres = torch.empty((P, 4), dtype=torch.int32, device=dev)
    draws = (ctypes.c_uint32 * (3 * P))(1, 2 ** 31, 2 ** 31, 1, 2 ** 32 - 1, 12345)
    patch = (ctypes.c_int32 * 3)(Pd, Ph, Pw)

    def pick():
        nat.call("ctseg_patch_centres", nat.ptr(masks), K, D, H, W, ctypes.addressof(draws), P, (1 << K) - 1, ctypes.addressof(patch),
                 nat.ptr(ws), need, nat.ptr(centres))

    def torch_count():
        return torch.count_nonzero(masks, dim=(1, 2, 3))

    def copy():
        masks_copy.copy_(masks)

    pick()
    assert torch.equal(ws[K * nb:K * nb + K].long().cpu(), want_counts) and torch.equal(torch_count().cpu(), want_counts)
    assert int(centres[:, 3].min()) >= 0

    # ---- crop ----
    img_out = torch.empty((Ph, Pw, Pd), dtype=torch.float32, device=dev)
    m_out = torch.empty((K, Ph, Pw, Pd), dtype=torch.uint8, device=dev)
    lab = torch.empty((Ph, Pw, Pd), dtype=torch.uint8, device=dev)
    hist = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    aug = T.augmented_degree_1["train"].augment
    extreme = dict(T.Augment3D.identity_params(), angles=tuple(float(v) for v in aug.rotate))
    sampler = T.PatchSampler3D(a.patch)
    pmats = {"identity": sampler.matrix(), "rotated": sampler.matrix(extreme)}
    amats = {"identity": np.eye(3, 4, dtype=np.float32), "rotated": T.Augment3D.matrix(a.patch, extreme)}
    cp = {k: (ctypes.c_float * 12)(*v.reshape(-1).tolist()) for k, v in pmats.items()}
    ca = {k: (ctypes.c_float * 12)(*v.reshape(-1).tolist()) for k, v in amats.items()}
    win = (2, -160.0, 240.0)

    def crop(which, interp):
        nat.call("ctseg_patch3d_to_hwd", nat.ptr(image), nat.I16, nat.ptr(masks), K, D, H, W, Pd, Ph, Pw, ctypes.addressof(cp[which]),
                 nat.ptr(centres), interp, 0, 0.0, None, *win, 1.0, 0.0, nat.ptr(img_out), nat.ptr(m_out), nat.ptr(lab), nat.ptr(hist))

    def augment(which, interp):
        nat.call("ctseg_augment3d_to_hwd", nat.ptr(image), nat.I16, nat.ptr(masks), K, D, H, W, Pd, Ph, Pw, ctypes.addressof(ca[which]),
                 interp, 0, 0.0, None, *win, 1.0, 0.0, nat.ptr(img_out), nat.ptr(m_out), nat.ptr(lab), nat.ptr(hist))

    c = [int(v) for v in centres[0, :3].cpu()]          # (set-up only: the timed torch restatement needs the start on the host)
    s0 = [c[i] - a.patch[i] // 2 for i in range(3)]

    def torch_crop():
        v = image[s0[0]:s0[0] + Pd, s0[1]:s0[1] + Ph, s0[2]:s0[2] + Pw].permute(1, 2, 0).contiguous().float()
        v = (v.clamp_(win[1], win[2]) - win[1]) / (win[2] - win[1] + 1e-8)
        m = masks[:, s0[0]:s0[0] + Pd, s0[1]:s0[1] + Ph, s0[2]:s0[2] + Pw].permute(0, 2, 3, 1).contiguous()
        return v, m

    crop("identity", 0)
    v, m = torch_crop()
    assert torch.equal(m_out, m) and float((img_out - v).abs().max()) < 1e-6 and int(hist.sum()) == n
    hist.zero_()

    variants = {"centres (count + select)": pick, "torch.count_nonzero": torch_count, "copy_ of the masks": copy,
                "crop identity": lambda: crop("identity", 0), "crop rotated": lambda: crop("rotated", 1),
                "augment3d identity": lambda: augment("identity", 0), "augment3d rotated": lambda: augment("rotated", 1),
                "torch crop identity": torch_crop}

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / a.reps

    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))

    split = {"count_ms": None, "select_ms": None}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                pick()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            for key, tag in (("count_ms", "patch_count_kernel"), ("select_ms", "patch_select_kernel")):
                if tag in ev.key and ev.count:
                    total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    split[key] = total / ev.count / 1e3
    except Exception as e:      # the profiler is optional here: the event timings above stand on their own
        split["profiler_error"] = repr(e)

    mask_bytes = K * D * H * W
    res = {"shape": list(a.shape), "patch": list(a.patch), "masks": K, "patches": P, "image_dtype": "int16", "reps": a.reps,
           "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "timing": "device events around reps back-to-back calls; median of rounds", "count_blocks_per_class": nb,
           "rotated_angles_rad": list(extreme["angles"]), "variants": {}, "kernel_split_from_profiler": split}
    for name in variants:
        res["variants"][name] = {"ms_per_call": statistics.median(times[name]), "ms_min_max": [min(times[name]), max(times[name])]}
    ms = {k: v["ms_per_call"] for k, v in res["variants"].items()}
    copy_bw = 2 * mask_bytes / (ms["copy_ of the masks"] * 1e-3)          # the copy reads and writes every byte
    res["mask_bytes"] = mask_bytes
    res["copy_GB_per_s"] = copy_bw / 1e9
    res["count_bytes_floor_ms"] = mask_bytes / copy_bw * 1e3
    res["centres_over_torch_count"] = ms["centres (count + select)"] / ms["torch.count_nonzero"]
    res["centres_GB_per_s"] = mask_bytes / (ms["centres (count + select)"] * 1e-3) / 1e9
    for which in ("identity", "rotated"):
        res[f"crop_{which}_over_augment3d"] = ms[f"crop {which}"] / ms[f"augment3d {which}"]
    res["crop_identity_over_torch"] = ms["crop identity"] / ms["torch crop identity"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
