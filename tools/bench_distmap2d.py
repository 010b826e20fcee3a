"""Timing of the device distance maps (ctseg_distmap2d_batch) at the reference's batch: 128 samples x 9 planes of 256 x 256.

Two inputs, alternating over several rounds in one process on one box:
  realistic    the synthetic ellipsoid masks of bench.py (synthetic_batch), one z slice per sample: about 1.3 % foreground, some
               classes absent from a slice
  adversarial  one foreground pixel in a corner of every plane: every outward search of the row pass runs the whole row
Two figures per input, device events around --reps calls after --warmup calls, median round with the spread: "launches" is the
two kernels on preallocated buffers, "whole_call" one compute_distance_map call (its three allocations on top).  Neither is a
kernel time from a profiler.  Bytes are algorithmic: 1 B in + 4 B out per pixel.

  python tools/bench_distmap2d.py --out profiles/distmap2d.json

--host-reference DIR times the reference's own compute_distance_map (DIR/capstone/data/utils.py, scipy on the host CPU, one
process, the loop its EnhancedMiccaiDataset2D.__getitem__ runs per sample) on the same realistic batch, and stores the figure under
"reference_host" in --out, next to the device figures; no GPU is needed for it.
"""
import argparse
import importlib.util
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))

import bench  # noqa: E402
from capstone_amd import _native as nat  # noqa: E402
from capstone_amd.data import utils as DU  # noqa: E402


def realistic_masks(B, side, device):
    """(B, 9, side, side) uint8: the z slices of one synthetic volume of bench.py"""
    _, masks, _ = bench.synthetic_batch(1, side, side, B, device, bench.SEED)
    return masks[0].permute(3, 0, 1, 2).contiguous()


def host_reference(a):
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(a.host_reference, "capstone", "data", "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    masks = realistic_masks(a.batch, a.side, "cpu").numpy()
    ref.compute_distance_map(masks[0])
    t0 = time.perf_counter()
    for m in masks:
        ref.compute_distance_map(m)
    dt = time.perf_counter() - t0
    import scipy
    return {"ms_per_batch": 1e3 * dt, "what": "reference compute_distance_map, one sample at a time in one process (18 scipy "
            "distance_transform_edt calls per sample with every class present), float64 result, no upload", "host": platform.processor()
            or platform.machine(), "cpus": os.cpu_count(), "numpy": np.__version__, "scipy": scipy.__version__,
            "measured_on": "the development host's CPU, not the GPU box"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-reference", default=None, help="root of a reference checkout: time its compute_distance_map on the host")
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.loads(f.read())
    if a.host_reference:
        res["reference_host"] = host_reference(a)
    else:
        assert torch.cuda.is_available(), "needs the MI355X"
        dev = "cuda:0"
        inputs = {"realistic": realistic_masks(a.batch, a.side, dev)}
        adv = torch.zeros_like(inputs["realistic"])
        adv[:, :, a.side - 1, 0] = 1
        inputs["adversarial"] = adv
        P, px = a.batch * 9, a.batch * 9 * a.side * a.side
        out = torch.empty((a.batch, 9, a.side, a.side), dtype=torch.float32, device=dev)
        ws = torch.empty((px,), dtype=torch.int32, device=dev)
        table = DU._byte_table(torch.device(dev))

        def launches(m):
            nat.call("ctseg_distmap2d_batch", nat.ptr(m), P, a.side, a.side, DU.REFERENCE, nat.ptr(table), nat.ptr(ws), 4 * px, nat.ptr(out),
                     None, None)

        def timed(fn, m):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.reps):
                fn(m)
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / a.reps

        for m in inputs.values():
            for _ in range(a.warmup):
                launches(m)
                DU.compute_distance_map(m)
        torch.cuda.synchronize()
        times = {k: {"launches": [], "whole_call": []} for k in inputs}
        for _ in range(a.rounds):
            for k, m in inputs.items():
                times[k]["launches"].append(timed(launches, m))
                times[k]["whole_call"].append(timed(DU.compute_distance_map, m))
        res["workload"] = {"batch": a.batch, "planes": P, "plane": f"{a.side} x {a.side} uint8", "mode": "REFERENCE", "reps": a.reps,
                           "rounds": a.rounds, "warmup": a.warmup}
        prop = torch.cuda.get_device_properties(0)
        res["box"] = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
                      "host": platform.node(), "torch": torch.__version__, "hip": torch.version.hip}
        res["method"] = ("device events around `reps` back-to-back calls after `warmup` calls, one process; the inputs alternate over "
                         "`rounds` rounds; median round, min and max given; bytes are algorithmic (1 B in + 4 B out per pixel)")
        res["inputs"] = {}
        for k, m in inputs.items():
            ms = statistics.median(times[k]["launches"])
            res["inputs"][k] = {"foreground_share": float((m != 0).float().mean()), "absent_plane_share": float((m.flatten(2).max(2).values == 0).float().mean()),
                                "ms_per_batch_launches": ms, "ms_launches_min_max": [min(times[k]["launches"]), max(times[k]["launches"])],
                                "ms_per_batch_whole_call": statistics.median(times[k]["whole_call"]),
                                "ms_whole_call_min_max": [min(times[k]["whole_call"]), max(times[k]["whole_call"])],
                                "bytes_algorithmic": 5 * px, "GBps_algorithmic": 5 * px / ms / 1e6}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
