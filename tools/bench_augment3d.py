"""Timing of the 3-D augmentation pass (ctseg_augment3d_to_hwd) against the plain resize pass (ctseg_resize3d_to_hwd) at the
pipeline's real shape: one synthetic instance, an int16 image and nine masks of 140 x 512 x 512, resized to 96 x 256 x 256.

Three launches, preallocated outputs, one process, device events around ``--reps`` back-to-back launches; the three alternate over
``--rounds`` rounds and the median round is reported with the spread (min, max):
  (a) resize           ctseg_resize3d_to_hwd, image + nine masks written
  (b) identity         the new entry, identity matrix, nearest, the same outputs
  (c) rotated          the new entry, the preset's extreme rotation (augmented_degree_1 "train": every angle at its half-range),
                       trilinear, the label map and hist plus nine masks written
A figure is one launch (enqueue + kernel, the launches queued back to back), not a kernel time from a profiler.

Bytes are algorithmic: every source byte an output voxel depends on, once per voxel, plus every output byte.  Per output voxel:
(a), (b) 2 + 9 read, 4 + 9 written = 24 B; (c) 8 * 2 + 9 read, 4 + 9 + 1 written = 39 B (voxels whose samples fall outside the
volume read less).

  python tools/bench_augment3d.py --out profiles/augment3d.json
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
    ap.add_argument("--size", type=int, nargs=3, default=(96, 256, 256))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    K = 9
    D, H, W = a.shape
    Do, Ho, Wo = a.size
    g = torch.Generator().manual_seed(12342)
    image = (torch.randn(D, H, W, generator=g) * 400).to(torch.int16).to(dev)
    masks = torch.zeros(K, D, H, W, dtype=torch.uint8)
    for k in range(K):
        masks[k, 10 + 10 * k:50 + 10 * k, 60 + 40 * k:160 + 40 * k, 80 + 30 * k:260 + 30 * k] = 1
    masks = masks.to(dev)
    n = Do * Ho * Wo
    img_out = torch.empty((Ho, Wo, Do), dtype=torch.float32, device=dev)
    m_out = torch.empty((K, Ho, Wo, Do), dtype=torch.uint8, device=dev)
    lab = torch.empty((Ho, Wo, Do), dtype=torch.uint8, device=dev)
    hist = torch.zeros(K + 1, dtype=torch.int64, device=dev)

    aug = T.augmented_degree_1["train"].augment
    extreme = dict(T.Augment3D.identity_params(), angles=tuple(float(v) for v in aug.rotate))
    mats = {"identity": np.eye(3, 4, dtype=np.float32), "rotated": T.Augment3D.matrix(a.size, extreme)}
    cmats = {k: (ctypes.c_float * 12)(*v.reshape(-1).tolist()) for k, v in mats.items()}

    def resize():
        nat.call("ctseg_resize3d_to_hwd", nat.ptr(image), nat.I16, nat.ptr(masks), K, D, H, W, Do, Ho, Wo, 0, 0.0, 1.0,
                 nat.ptr(img_out), nat.ptr(m_out), None, None)

    def augment(which, interp, labels):
        nat.call("ctseg_augment3d_to_hwd", nat.ptr(image), nat.I16, nat.ptr(masks), K, D, H, W, Do, Ho, Wo,
                 ctypes.addressof(cmats[which]), interp, 0, 0.0, None, 0, 0.0, 1.0, 1.0, 0.0, nat.ptr(img_out), nat.ptr(m_out),
                 nat.ptr(lab) if labels else None, nat.ptr(hist) if labels else None)

    variants = {"resize": (resize, 24), "identity": (lambda: augment("identity", 0, False), 24),
                "rotated": (lambda: augment("rotated", 1, True), 39)}

    # what is timed computes what it should: (b) equals (a) bit for bit, (c) counts every output voxel once
    resize()
    ref = (img_out.clone(), m_out.clone())
    variants["identity"][0]()
    assert torch.equal(img_out, ref[0]) and torch.equal(m_out, ref[1])
    variants["rotated"][0]()
    assert int(hist.sum()) == n

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / a.reps

    for fn, _ in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, (fn, _) in variants.items():
            times[name].append(timed(fn))
    res = {"shape": list(a.shape), "size": list(a.size), "masks": K, "image_dtype": "int16", "reps": a.reps, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "timing": "device events around reps back-to-back launches",
           "rotated_angles_rad": list(extreme["angles"]), "variants": {}}
    for name, (_, bpv) in variants.items():
        ms = statistics.median(times[name])
        res["variants"][name] = {"ms_per_launch": ms, "ms_min_max": [min(times[name]), max(times[name])],
                                 "algorithmic_bytes": bpv * n, "bytes_per_output_voxel": bpv,
                                 "achieved_GB_per_s": bpv * n / (ms * 1e-3) / 1e9}
    base = res["variants"]["resize"]["ms_per_launch"]
    res["identity_over_resize"] = res["variants"]["identity"]["ms_per_launch"] / base
    res["rotated_over_resize"] = res["variants"]["rotated"]["ms_per_launch"] / base
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
