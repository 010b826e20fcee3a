"""Timing of the device connected components (capstone_amd.components): one sample of 256 x 256 x 96 with nine classes.

Two inputs, alternating over several rounds in one process on one box:
  balls_noise  one ball per class plus salt noise: every class at 0.05 % of the voxels, scattered (the stray islands the
               post-processing exists for)
  comb         the worst case for the merge pass: class 1 is ONE component made of every fourth Z line of every fourth X plane,
               joined at alternating Z ends inside a plane and by bridges along X, so it crosses every tile face hundreds of
               times and the unions across faces form long chains; class 7 is the same comb in the gaps
Per input and entry (ctseg_components_label: three launches, ctseg_components_keep: four), device events around --reps calls on
preallocated buffers after --warmup rounds: median round with the spread; "whole_call" is one keep_largest_component() call, its
allocations and dtype conversions included.  None is a kernel time from a profiler; --kernel-times INPUT=FILE merges the
per-kernel averages of a kernel trace of `--only INPUT` taken in a run of its own (a CSV with "Name" and "AverageNs" or "Average"
columns) into that input's result under "kernel_ms_per_call": the per-launch times.  "floor_ms" is the bytes every launch must move at least, summed over the seven
launches, over 6.29 TB/s.  No threshold is attached to any figure.
The host figure is scipy.ndimage.label with the full structure per class plus np.bincount and the masking, on the machine the
script runs on; "scipy is not importable here" when it is not.

  python tools/profile_components.py --out profiles/components.json
"""
import argparse
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

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd import components  # noqa: E402

C = 10
HBM_BYTES_PER_S = 6.29e12
# bytes per voxel that each launch reads and writes whatever the labels are: local (labels 1, ids 4, sizes 4), merge (labels 1),
# flatten (ids 4, sizes 4), scan (sizes 4), apply (labels 1, out 1); the zero and table launches touch 16 bytes per class
FLOOR_BYTES_PER_VOXEL = {"local": 9, "merge": 1, "flatten": 8, "scan": 4, "apply": 2}


def balls_noise(shape, seed=12342):
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    xx, yy, zz = np.ogrid[:X, :Y, :Z]
    L = np.zeros(shape, np.uint8)
    for c in range(1, C):
        cx, cy, cz, r = rng.uniform(20, X - 20), rng.uniform(20, Y - 20), rng.uniform(20, Z - 20), rng.uniform(4, 20)
        L[(xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2 <= r * r] = c
    salt = rng.random(shape) < 0.0005 * (C - 1)
    L[salt] = rng.integers(1, C, shape, dtype=np.uint8)[salt]
    return L


def comb(shape, label, off, L):
    X, Y, Z = shape
    for x in range(off, X, 4):
        for j, y in enumerate(range(off, Y, 4)):
            L[x, y, :] = label
            if y + 4 < Y:
                L[x, y:y + 4, Z - 1 if j % 2 == 0 else 0] = label
        if x + 4 < X:
            L[x:x + 4, off, 0] = label
    return L


def host_scipy(L):
    try:
        import scipy
        from scipy import ndimage
    except ImportError:
        return "scipy is not importable here"
    t0 = time.perf_counter()
    out, counts = L.copy(), []
    full = ndimage.generate_binary_structure(3, 3)
    for c in range(1, C):
        lab, n = ndimage.label(L == c, full)
        counts.append(int(n))
        if n > 1:
            out[(lab != np.argmax(np.bincount(lab.ravel())[1:]) + 1) & (lab > 0)] = 0
    dt = time.perf_counter() - t0
    return {"ms_per_sample": 1e3 * dt, "components": counts, "voxels_kept": int((out > 0).sum()),
            "what": "scipy.ndimage.label (26 neighbours) per class, argmax(bincount), masking; one process, no upload",
            "host": platform.processor() or platform.machine(), "cpus_visible": os.cpu_count(), "numpy": np.__version__,
            "scipy": scipy.__version__}


def kernel_times(path):
    """a kernel-statistics CSV ("Name", "AverageNs" or "Average") -> {kernel name without signature: ms per call}"""
    import csv
    with open(path) as f:
        rows = list(csv.DictReader(f))
    return {r["Name"].split("(")[0].replace("void ", "").replace("ctseg::", ""): float(r.get("AverageNs") or r.get("Average")) / 1e6
            for r in rows if "components_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 256, 96])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only", default=None, help="time this input alone")
    ap.add_argument("--kernel-times", nargs="*", default=[], metavar="INPUT=FILE")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev, shape = "cuda:0", tuple(a.shape)
    X, Y, Z = shape
    S, K = X * Y * Z, C - 1
    host = {"balls_noise": balls_noise(shape), "comb": comb(shape, 7, 2, comb(shape, 1, 0, np.zeros(shape, np.uint8)))}
    if a.only:
        host = {a.only: host[a.only]}
    inputs = {k: torch.from_numpy(v)[None].to(dev) for k, v in host.items()}
    ids = torch.empty((1, X, Y, Z), dtype=torch.int32, device=dev)
    sizes = torch.empty_like(ids)
    out = torch.empty((1, X, Y, Z), dtype=torch.uint8, device=dev)
    table = torch.empty((1, K, 4), dtype=torch.int32, device=dev)
    ws = torch.empty((K * components.KEEP_ROW_BYTES // 8,), dtype=torch.int64, device=dev)
    mask = (1 << C) - 2

    def stage_label(lab):
        nat.call("ctseg_components_label", nat.ptr(lab), 1, X, Y, Z, C, 3, 7, nat.ptr(ids), nat.ptr(sizes))

    def stage_keep(lab):
        nat.call("ctseg_components_keep", nat.ptr(lab), nat.ptr(ids), nat.ptr(sizes), 1, X, Y, Z, C, mask, 1, 0, nat.ptr(ws),
                 K * components.KEEP_ROW_BYTES, nat.ptr(out), nat.ptr(table))

    def whole(lab):
        components.keep_largest_component(lab, C)

    stages = {"label": stage_label, "keep": stage_keep, "whole_call": whole}

    def timed(fn, lab):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn(lab)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    times = {k: {n: [] for n in stages} for k in inputs}
    for r in range(a.warmup + a.rounds):
        for k, lab in inputs.items():
            for n, fn in stages.items():                             # (in order: the keep reads what the label call left)
                ms = timed(fn, lab)
                if r >= a.warmup:
                    times[k][n].append(ms)
    prop = torch.cuda.get_device_properties(0)
    floor_ms = {n: 1e3 * b * S / HBM_BYTES_PER_S for n, b in FLOOR_BYTES_PER_VOXEL.items()}
    res = {"workload": {"sample": " x ".join(map(str, shape)) + " uint8 label map, B = 1", "classes": K, "voxels": S, "connectivity": 3,
                        "reps": a.reps, "rounds": a.rounds, "warmup_rounds": a.warmup,
                        "working_set_bytes": components.BYTES_PER_VOXEL * S, "launches": {"label": 3, "keep": 4}},
           "box": {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""),
                   "compute_units": prop.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip},
           "method": "device events around `reps` back-to-back calls of one entry on preallocated buffers, one process; the inputs "
                     "alternate over `rounds` rounds after `warmup_rounds`; median round, min and max given; whole_call is "
                     "keep_largest_component() with its allocations; no profiler, no threshold",
           "floor": {"bytes_per_voxel": FLOOR_BYTES_PER_VOXEL, "bytes_per_voxel_total": sum(FLOOR_BYTES_PER_VOXEL.values()),
                     "hbm_bytes_per_s": HBM_BYTES_PER_S, "floor_ms": floor_ms, "floor_ms_total": sum(floor_ms.values())},
           "inputs": {}}
    for k, lab in inputs.items():
        r = components.keep_largest_component(lab, C)
        torch.cuda.synchronize()
        res["inputs"][k] = {"foreground_voxels": int((host[k] > 0).sum()), "components": r.count[0].tolist(),
                            "largest": r.largest[0].tolist(), "removed": r.removed[0].tolist(),
                            "voxels_kept": int((r.labels > 0).sum().item()),
                            "ms_per_sample": {n: statistics.median(v) for n, v in times[k].items()},
                            "ms_min_max": {n: [min(v), max(v)] for n, v in times[k].items()}}
        ms = res["inputs"][k]["ms_per_sample"]
        res["inputs"][k]["label_plus_keep_over_floor"] = (ms["label"] + ms["keep"]) / sum(floor_ms.values())
    for pair in a.kernel_times:
        k, path = pair.split("=", 1)
        res["inputs"][k]["kernel_ms_per_call"] = kernel_times(path)
        res["kernel_ms_per_call_source"] = "per-kernel averages of a kernel trace of this script on that input alone, in a run of its own"
    res["host_scipy"] = "not measured" if a.no_host else {k: host_scipy(v) for k, v in host.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
