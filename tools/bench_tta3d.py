"""Timing of the test-time-augmentation merge (ctseg_tta_accumulate, ctseg_tta_finish) at the 3-D pipeline's real shape: one view of
C = 10 classes on the model grid (96, 256, 256), its fp32 channels-last logits 12 floats wide, the accumulator 12 floats wide.

Three launches, preallocated buffers, one process, device events around ``--reps`` back-to-back launches; the launches and their
torch yardsticks alternate over ``--rounds`` rounds and the median round is reported with the spread (min, max):
  (a) same_grid        one accumulate onto the model grid itself: identity matrix, trilinear, mean of probabilities
  (b) native_rotated   one accumulate onto a native (140, 512, 512) grid, rows in (d, h, w) order, for the view of the preset's
                       extreme rotation (augmented_degree_1 "train": every angle at its half-range), trilinear, probabilities
  (c) finish           labels only, from the model-grid accumulator
A figure is one launch (enqueue + kernel, the launches queued back to back), not a kernel time from a profiler.

Bytes are algorithmic, a floor: the view's block read once (4 * ld bytes per view voxel) plus the read-modify-write of every covered
accumulator row (2 * 4 * acc_ld bytes); finish reads every row (4 * acc_ld) and writes one byte.  The kernel itself asks for up to
eight view rows per target voxel; how many of them the caches absorb is what the distance from the floor shows.

The yardstick is the torch expression on the same tensors in the same run, its sampling grid built beforehand and not timed:
``acc.add_(softmax(grid_sample(logits, grid), 1), alpha=w)`` for (a) and (b), ``acc.argmax(1).to(uint8)`` for (c).  It is a
yardstick, not a threshold.

  python tools/bench_tta3d.py --out profiles/tta3d.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))

from capstone_amd.volumetric import transforms as T  # noqa: E402
from capstone_amd.volumetric import tta  # noqa: E402


def torch_grid(M, view, target, dev):
    """grid_sample's normalised grid (align_corners=True) of the matrix M for an input laid out (H, W, D): (1, Dt, Ht, Wt, 3)"""
    D, H, W = view
    o = torch.meshgrid(*(torch.arange(n, dtype=torch.float32, device=dev) for n in target), indexing="ij")
    q = [M[a][0] * o[0] + M[a][1] * o[1] + M[a][2] * o[2] + M[a][3] for a in range(3)]          # d, h, w of the view
    norm = [2.0 * q[a] / (n - 1) - 1.0 for a, n in enumerate((D, H, W))]
    return torch.stack([norm[0], norm[2], norm[1]], dim=-1)[None]          # x = the input's last axis (d), y = w, z = h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=(96, 256, 256))
    ap.add_argument("--native", type=int, nargs=3, default=(140, 512, 512))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    C, ld = 10, 12
    acc_ld = tta.acc_width(C)
    size, native = tuple(a.size), tuple(a.native)
    D, H, W = size
    n_view, n_native = D * H * W, native[0] * native[1] * native[2]
    g = torch.Generator(device=dev).manual_seed(12342)
    store = 4.0 * torch.randn((H, W, D, ld), generator=g, device=dev)
    logits = store[..., :C].permute(3, 0, 1, 2).unsqueeze(0)               # (1, C, H, W, D), channels-last storage in place
    acc_same = torch.zeros((n_view, acc_ld), device=dev)
    acc_native = torch.zeros((n_native, acc_ld), device=dev)

    aug = T.augmented_degree_1["train"].augment
    extreme = dict(T.Augment3D.identity_params(), angles=tuple(float(v) for v in aug.rotate))
    ident = np.eye(3, 4, dtype=np.float32)
    rotated = tta.view_to_target_matrix(size, extreme, native)

    grid_same = torch_grid(ident, size, size, dev)
    grid_native = torch_grid(rotated, size, native, dev)
    t_same = torch.zeros((1, C) + size, device=dev)
    t_native = torch.zeros((1, C) + native, device=dev)

    def torch_accumulate(acc, grid):
        acc.add_(torch.softmax(F.grid_sample(logits, grid, mode="bilinear", padding_mode="border", align_corners=True), 1), alpha=1.0)

    variants = {
        "same_grid": (lambda: tta.tta_accumulate(acc_same, logits, ident, None, 1.0, "probabilities", "trilinear", size, "hwd"),
                      4 * ld * n_view + 2 * 4 * acc_ld * n_view),
        "same_grid_torch": (lambda: torch_accumulate(t_same, grid_same), None),
        "native_rotated": (lambda: tta.tta_accumulate(acc_native, logits, rotated, None, 1.0, "probabilities", "trilinear", native, "dhw"),
                           None),
        "native_rotated_torch": (lambda: torch_accumulate(t_native, grid_native), None),
        "finish": (lambda: tta.tta_finish(acc_same, C, "probabilities"), (4 * acc_ld + 1) * n_view),
        "finish_torch": (lambda: t_same.argmax(1).to(torch.uint8), None),
    }

    # what is timed computes what it should: the identity view's rows are softmaxes with weight 1; the rotated view's coverage
    variants["same_grid"][0]()
    assert bool((acc_same[:, C] == 1).all()) and float((acc_same[:, :C].sum(1) - 1).abs().max()) < 1e-5
    want = torch.softmax(store[..., :C], -1).reshape(-1, C)
    assert float((acc_same[:, :C] - want).abs().max()) < 1e-5
    labels = tta.tta_finish(acc_same, C, "probabilities")[0]
    assert torch.equal(labels.long(), want.argmax(1))
    variants["native_rotated"][0]()
    covered = int((acc_native[:, C] == 1).sum())
    assert 0.5 * n_native < covered <= n_native and int((acc_native[:, C] == 0).sum()) == n_native - covered
    variants["native_rotated"] = (variants["native_rotated"][0], 4 * ld * n_view + 2 * 4 * acc_ld * covered)

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
    res = {"size": list(size), "native": list(native), "classes": C, "ld": ld, "acc_ld": acc_ld, "reps": a.reps, "rounds": a.rounds,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "timing": "device events around reps back-to-back launches",
           "rotated_angles_rad": list(extreme["angles"]), "native_covered_share": covered / n_native, "variants": {}}
    for name, (_, nbytes) in variants.items():
        ms = statistics.median(times[name])
        res["variants"][name] = {"ms_per_launch": ms, "ms_min_max": [min(times[name]), max(times[name])]}
        if nbytes is not None:
            res["variants"][name].update(algorithmic_bytes=nbytes, floor_GB_per_s=nbytes / (ms * 1e-3) / 1e9)
    for name in ("same_grid", "native_rotated", "finish"):
        res[f"{name}_torch_over_hip"] = res["variants"][name + "_torch"]["ms_per_launch"] / res["variants"][name]["ms_per_launch"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
