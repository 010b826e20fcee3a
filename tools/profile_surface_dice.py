"""Timing of the surface Dice at tolerance (capstone_amd.surface.surface_dice): one sample of 256 x 256 x 96 with nine classes, the
balls-plus-shift input of tools/profile_surface_distance.py, per call.

In one process on one box, alternating over several rounds:
  surface_dice_tau1 / _tau3 / _tau8   surface_dice() in voxel units at tolerance 1, 3 and 8 (the radius limit)
  surface_dice_3mm                    surface_dice(tolerance=3, spacing=--spacing): the float32 rule
  kernel_tau3                         ctseg_surface_dice alone at tolerance 3 on preallocated tables: no allocation, no torch ops
  surface_distances                   surface_distances() on the same input: the only route to anything like this figure before
  label_copy                          copy_ of the two label maps into preallocated buffers
Device events around --reps calls after --warmup rounds; median round with the spread.  None is a kernel time from a profiler and no
threshold is attached to any figure.  The bytes floor is what the kernel must read, 2 bytes per voxel, at the bandwidth the copy
reached (which moves 2 bytes per voxel in and 2 out); the search is not bytes-bound, so the ratio is reported without a target.

  python tools/profile_surface_dice.py --out profiles/surface_dice.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd import surface  # noqa: E402
from profile_surface_distance import C, ball_labels  # noqa: E402


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 256, 96])
    ap.add_argument("--spacing", type=float, nargs=3, default=[0.977, 0.977, 2.5])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the commit the figures are taken on (default: git rev-parse)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev, shape = "cuda:0", tuple(a.shape)
    X, Y, Z = shape
    K = C - 1
    pred, target = (torch.from_numpy(ball_labels(shape, s))[None].to(dev) for s in ((0, 0, 0), (3, -2, 4)))
    copies = (torch.empty_like(pred), torch.empty_like(target))
    _, limit, radius = surface._dice_tables(3.0, K, None, 3, None)
    limit, radius = limit.contiguous().to(dev), radius.contiguous()
    tables = torch.zeros((2, 2, 1, K), dtype=torch.int32, device=dev)

    def kernel():
        tables.zero_()
        nat.call("ctseg_surface_dice", nat.ptr(pred), nat.ptr(target), 1, X, Y, Z, C, 7, nat.ptr(radius), nat.ptr(limit), None,
                 nat.ptr(tables[0]), nat.ptr(tables[1]))

    def label_copy():
        copies[0].copy_(pred)
        copies[1].copy_(target)

    stages = {"surface_dice_tau1": lambda: surface.surface_dice(pred, target, 1.0),
              "surface_dice_tau3": lambda: surface.surface_dice(pred, target, 3.0),
              "surface_dice_tau8": lambda: surface.surface_dice(pred, target, 8.0),
              "surface_dice_3mm": lambda: surface.surface_dice(pred, target, 3.0, spacing=a.spacing),
              "kernel_tau3": kernel,
              "surface_distances": lambda: surface.surface_distances(pred, target, C),
              "label_copy": label_copy}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    times = {n: [] for n in stages}
    for r in range(a.warmup + a.rounds):
        for n, fn in stages.items():
            ms = timed(fn)
            if r >= a.warmup:
                times[n].append(ms)
    ms = {n: statistics.median(v) for n, v in times.items()}
    S = X * Y * Z
    copy_bw = 4 * S / (ms["label_copy"] * 1e-3)                        # bytes read + written per second
    floor_ms = 2 * S / copy_bw * 1e3
    scores = {}
    for name, kw in (("tau1", dict(tolerance=1.0)), ("tau3", dict(tolerance=3.0)), ("tau8", dict(tolerance=8.0)),
                     ("3mm", dict(tolerance=3.0, spacing=a.spacing))):
        res = surface.surface_dice(pred, target, **kw)
        torch.cuda.synchronize()
        scores[name] = {"nsd": res.nsd[0].tolist(), "within": res.within[:, 0].tolist(), "radius": res.radius[0, 0].tolist()}
    prop = torch.cuda.get_device_properties(0)
    res = {"workload": {"sample": " x ".join(map(str, shape)) + " uint8 label maps, B = 1, one ball per class, truth shifted by (3, -2, 4)",
                        "classes": K, "voxels": S, "spacing": list(a.spacing), "surface_voxels": res.counts[:, 0].tolist(),
                        "reps": a.reps, "rounds": a.rounds, "warmup_rounds": a.warmup},
           "box": {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""),
                   "compute_units": prop.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip},
           "commit": a.commit or commit(),
           "method": "device events around `reps` back-to-back calls, one process, the stages alternating over `rounds` rounds after "
                     "`warmup_rounds`; median round, min and max given; surface_dice_* and surface_distances are whole calls with their "
                     "allocations and closing torch ops, kernel_tau3 is the entry point with the zeroing of its tables; no profiler, "
                     "no threshold",
           "ms_per_call": ms, "ms_min_max": {n: [min(v), max(v)] for n, v in times.items()},
           "surface_distances_over_surface_dice_tau3": ms["surface_distances"] / ms["surface_dice_tau3"],
           "bytes_floor": {"what": "2 bytes per voxel read, at the bandwidth label_copy reached (2 bytes per voxel read + 2 written)",
                           "copy_bytes_per_s": copy_bw, "floor_ms": floor_ms,
                           "kernel_tau3_over_floor": ms["kernel_tau3"] / floor_ms,
                           "surface_dice_tau3_over_floor": ms["surface_dice_tau3"] / floor_ms},
           "scores": scores}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
