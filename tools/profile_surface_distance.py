"""Timing of the device surface metrics (capstone_amd.surface): one sample of 256 x 256 x 96 with nine classes, stage by stage.

Two inputs, alternating over several rounds in one process on one box:
  balls         one ball per class, the truth's centres a few voxels away from the prediction's
  select_worst  the same, but class 1 is a diagonal sheet of voxels in the prediction and one corner voxel in the truth: the
                distances of that row span the whole range, so its coarse histogram has many bins in use
Per input and stage (ctseg_surface_edges, ctseg_distmap3d_batch on the 18 surface masks, ctseg_surface_select), device events
around --reps calls on preallocated buffers after --warmup calls: median round with the spread; "whole_call" is one
surface_distances() call, its allocations and the closing torch ops included.  None is a kernel time from a profiler.  No threshold is
attached to any figure.
The host figure is the same metric with scipy on the machine the script runs on: binary_erosion for the surfaces, one
distance_transform_edt per surface, np.percentile and the means.
With --spacing SX SY SZ the same run also times the physical-unit path on the same surface masks: ctseg_distmap3d_weighted
("transform_weighted"), ctseg_surface_select_f32 ("select_f32") and surface_distances(spacing=...) ("whole_call_spacing"), so the two
transforms are compared on one box in one process.  The per-kernel split of a transform (sweep, Z lines, Y slabs) is not visible to
device events around an entry point; --kernel-times FILE merges the per-kernel averages of a kernel trace taken in a run of its own
(a CSV with "Name" and "AverageNs" or "Average" columns, such as a profiler's kernel statistics) into the result under
"kernel_ms_per_call".

  python tools/profile_surface_distance.py --spacing 0.9765625 0.9765625 2.5 --out profiles/surface_distance.json
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
from capstone_amd import surface  # noqa: E402
from capstone_amd.data import utils as DU  # noqa: E402

C = 10


def ball_labels(shape, shift, seed=12342):
    """(X, Y, Z) uint8 label map: one ball per class, radius 4..20 voxels, every centre moved by `shift`"""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    xx, yy, zz = np.ogrid[:X, :Y, :Z]
    L = np.zeros(shape, np.uint8)
    for c in range(1, C):
        cx, cy, cz, r = rng.uniform(20, X - 20), rng.uniform(20, Y - 20), rng.uniform(20, Z - 20), rng.uniform(4, 20)
        L[(xx - cx - shift[0]) ** 2 + (yy - cy - shift[1]) ** 2 + (zz - cz - shift[2]) ** 2 <= r * r] = c
    return L


def host_scipy(pred, target, q):
    import scipy
    from scipy.ndimage import binary_erosion, distance_transform_edt
    t0 = time.perf_counter()
    hd = np.full(C - 1, np.nan)
    assd = np.full(C - 1, np.nan)
    for c in range(1, C):
        s = []
        for L in (pred, target):
            m = L == c
            s.append(m ^ binary_erosion(m))
        if not s[0].any() or not s[1].any():
            continue
        d = [distance_transform_edt(~s[1])[s[0]], distance_transform_edt(~s[0])[s[1]]]
        hd[c - 1] = max(np.percentile(d[0], q), np.percentile(d[1], q))
        assd[c - 1] = (d[0].sum() + d[1].sum()) / (len(d[0]) + len(d[1]))
    dt = time.perf_counter() - t0
    return {"ms_per_sample": 1e3 * dt, "hd": hd.tolist(), "assd": assd.tolist(),
            "what": "scipy binary_erosion + distance_transform_edt per class and side, np.percentile, one process, no upload",
            "host": platform.processor() or platform.machine(), "cpus_visible": os.cpu_count(), "numpy": np.__version__,
            "scipy": scipy.__version__}


def kernel_times(path):
    """a kernel-statistics CSV ("Name", "AverageNs" or "Average") -> {kernel name without signature: ms per call} of this library's
    distance-map and surface kernels"""
    import csv
    with open(path) as f:
        rows = list(csv.DictReader(f))
    return {r["Name"].split("(")[0].replace("void ", "").replace("ctseg::", ""): float(r.get("AverageNs") or r.get("Average")) / 1e6
            for r in rows if "distmap3d" in r["Name"] or "surface_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 256, 96])
    ap.add_argument("--percentile", type=float, default=95.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--spacing", type=float, nargs=3, default=None)
    ap.add_argument("--kernel-times", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev, shape, q = "cuda:0", tuple(a.shape), a.percentile
    X, Y, Z = shape
    host = {"balls": (ball_labels(shape, (0, 0, 0)), ball_labels(shape, (3, -2, 4)))}
    p, t = (v.copy() for v in host["balls"])
    p[p == 1], t[t == 1] = 0, 0
    i = np.arange(min(X, Y))
    p[i, i, :] = 1                                                   # a diagonal sheet, one voxel thick
    t[0, 0, 0] = 1
    host["select_worst"] = (p, t)
    inputs = {k: tuple(torch.from_numpy(v)[None].to(dev) for v in pair) for k, pair in host.items()}
    S, K = X * Y * Z, C - 1
    P = 2 * K
    edges = torch.empty((P * S,), dtype=torch.uint8, device=dev)
    d2 = torch.empty((P * S,), dtype=torch.int32, device=dev)
    fmap = torch.empty((P * S,), dtype=torch.float32, device=dev)
    dm_ws = torch.empty((DU.WORKSPACE_BYTES_3D * P * S,), dtype=torch.uint8, device=dev)
    sel_ws = torch.empty((P * surface.SELECT_ROW_BYTES // 8,), dtype=torch.float64, device=dev)
    cnt = torch.zeros((2, 1, K), dtype=torch.int32, device=dev)
    st = torch.empty((2, 1, K, 4), dtype=torch.int32, device=dev)
    fs = torch.empty((2, 1, K, 2), dtype=torch.float64, device=dev)
    table = DU._byte_table(torch.device(dev))

    def stage_edges(pair):
        cnt.zero_()
        nat.call("ctseg_surface_edges", nat.ptr(pair[0]), nat.ptr(pair[1]), 1, X, Y, Z, C, 7, nat.ptr(edges), nat.ptr(cnt))

    def stage_transform(pair):
        nat.call("ctseg_distmap3d_batch", nat.ptr(edges), P, X, Y, Z, DU.REFERENCE, nat.ptr(table), nat.ptr(dm_ws), dm_ws.numel(),
                 nat.ptr(fmap), nat.ptr(d2), None)

    def stage_select(pair):
        nat.call("ctseg_surface_select", nat.ptr(edges), nat.ptr(d2), nat.ptr(cnt), 1, X, Y, Z, C, q, nat.ptr(sel_ws),
                 P * surface.SELECT_ROW_BYTES, nat.ptr(st), nat.ptr(fs))

    def whole(pair):
        surface.surface_distances(pair[0], pair[1], C, q)

    stages = {"edges": stage_edges, "transform": stage_transform, "select": stage_select, "whole_call": whole}
    if a.spacing:
        d2f = torch.empty((P * S,), dtype=torch.float32, device=dev)
        sel_ws_f = torch.empty((P * surface.SELECT_F32_ROW_BYTES // 8,), dtype=torch.float64, device=dev)
        w = surface._squared_spacing(a.spacing, 1, 3).to(dev).expand(P, 3).contiguous()

        def stage_transform_weighted(pair):
            nat.call("ctseg_distmap3d_weighted", nat.ptr(edges), P, X, Y, Z, nat.ptr(w), nat.ptr(dm_ws), dm_ws.numel(), nat.ptr(d2f),
                     None)

        def stage_select_f32(pair):
            nat.call("ctseg_surface_select_f32", nat.ptr(edges), nat.ptr(d2f), nat.ptr(cnt), 1, X, Y, Z, C, q, nat.ptr(sel_ws_f),
                     P * surface.SELECT_F32_ROW_BYTES, nat.ptr(st), nat.ptr(fs))

        def whole_spacing(pair):
            surface.surface_distances(pair[0], pair[1], C, q, spacing=a.spacing)

        # (after whole_call, which has buffers of its own: `edges` and `cnt` still hold this input's surfaces)
        stages.update(transform_weighted=stage_transform_weighted, select_f32=stage_select_f32, whole_call_spacing=whole_spacing)

    def timed(fn, pair):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn(pair)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    times = {k: {n: [] for n in stages} for k in inputs}
    for r in range(a.warmup + a.rounds):
        for k, pair in inputs.items():
            for n, fn in stages.items():                             # (in order: each stage reads what the one before it left)
                ms = timed(fn, pair)
                if r >= a.warmup:
                    times[k][n].append(ms)
    prop = torch.cuda.get_device_properties(0)
    res = {"workload": {"sample": " x ".join(map(str, shape)) + " uint8 label maps, B = 1", "classes": K, "surface_volumes": P,
                        "voxels_per_volume": S, "percentile": q, "reps": a.reps, "rounds": a.rounds, "warmup_rounds": a.warmup,
                        "working_set_bytes": surface.BYTES_PER_VOXEL * P * S},
           "box": {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""),
                   "compute_units": prop.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip},
           "method": "device events around `reps` back-to-back calls of one stage on preallocated buffers, one process; the inputs "
                     "alternate over `rounds` rounds after `warmup_rounds`; median round, min and max given; whole_call is "
                     "surface_distances() with its allocations; no profiler, no threshold",
           "inputs": {}}
    for k, pair in inputs.items():
        tab = surface.surface_distances(pair[0], pair[1], C, q)
        torch.cuda.synchronize()
        res["inputs"][k] = {"surface_voxels": tab.counts[:, 0].tolist(), "hd": tab.hd[0].tolist(), "assd": tab.assd[0].tolist(),
                            "d2_max": tab.d2_max[:, 0].tolist(),
                            "ms_per_sample": {n: statistics.median(v) for n, v in times[k].items()},
                            "ms_min_max": {n: [min(v), max(v)] for n, v in times[k].items()}}
        if a.spacing:
            tab = surface.surface_distances(pair[0], pair[1], C, q, spacing=a.spacing)
            torch.cuda.synchronize()
            ms = res["inputs"][k]["ms_per_sample"]
            res["inputs"][k]["spacing"] = {"hd": tab.hd[0].tolist(), "assd": tab.assd[0].tolist(), "d2_max": tab.d2_max[:, 0].tolist(),
                                           "transform_weighted_over_transform": ms["transform_weighted"] / ms["transform"]}
    if a.spacing:
        res["workload"]["spacing"] = list(a.spacing)
        res["workload"]["working_set_bytes_spacing"] = surface.BYTES_PER_VOXEL_WEIGHTED * P * S
    if a.kernel_times:
        res["kernel_ms_per_call"] = kernel_times(a.kernel_times)
        res["kernel_ms_per_call_source"] = "per-kernel averages of a kernel trace of this script, taken in a separate run"
    res["host_scipy"] = "not measured" if a.no_host else {k: host_scipy(*pair, q) for k, pair in host.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
