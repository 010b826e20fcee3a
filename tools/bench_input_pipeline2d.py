"""Timing of the 2-D device input pipeline (ctseg_pipeline2d_batch) at the reference's 2-D workload: a batch of 128 raw slices of
about 400 x 400 int16 with 9 masks -> 3 x 256 x 256, CROP (windowed_degree_2 "train") and RESIZE (every "test" side), with the 9
masks and with the squashed label map.  One process, device events; the four variants alternate over several rounds and the
median round is reported with the spread.  Two figures per variant: "launch" is one pipeline2d_batch call (the table upload, the
output allocation and the launch), "whole_call" one BatchPipeline2D call on top of it (explicit params: nothing is drawn, the
table is built and checked on the host).  Neither is a kernel time from a profiler.

Bytes are algorithmic: every source byte the outputs depend on, once, plus every output byte (CROP: the crop's pixels; RESIZE:
the whole raw slice for the bilinear image, one byte per output pixel and mask for the nearest masks).

  python tools/bench_input_pipeline2d.py --with-3d --out profiles/pipeline2d.json

--warped-out FILE also times the warping presets (predefined.warped: degree_0, windowed_degree_3, windowed_degree_4 "train";
ctseg_pipeline2d_warp_batch) under the same conditions, with the CROP preset alternating in the same rounds as the yardstick: the
whole call of three launches and each launch alone (bit 0 fields, bit 1 pass 1, bit 2 pass 2; each figure includes the table and
map-table uploads of a call, the intermediate is allocated once), and the share of samples of each kind in the drawn batch.

  python tools/bench_input_pipeline2d.py --warped-out profiles/pipeline2d_warp.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))

from capstone_amd.transforms import predefined  # noqa: E402
from capstone_amd.transforms import warp2d  # noqa: E402
from capstone_amd.transforms.pipeline2d import CROP, SliceStore2D, pipeline2d_batch  # noqa: E402


def bench_warped(a, store, idx, timed, crop_variant):
    """the warped presets and the CROP yardstick, alternating; ms per batch (median round) of the three launches and of each alone"""
    jobs = {}
    for name, preset in predefined.warped.items():
        pipe = preset["train"]
        rows = store.table[idx]
        params = pipe.draw_params(rows[:, 2:4], np.random.default_rng(1))
        table, xx, yy = pipe.build_table(rows, params)
        el = pipe.elastic
        kw = dict(sigma=el.sigma, alpha=el.alpha, xx=xx, yy=yy, want_masks=True, want_present=True)
        args = (store, table, pipe.size, pipe.windows, pipe.shift, pipe.mean, pipe.denom)
        buffers = warp2d.pipeline2d_warp_batch(*args, **kw)[5]
        kinds = np.bincount(table[:, 8], minlength=3) / len(table)
        jobs[name] = (args, kw, buffers, {"none": kinds[0], "elastic": kinds[1], "grid": kinds[2]})
    parts = {"three_launches": 7, "fields": warp2d.FIELDS, "pass1": warp2d.PASS1, "pass2": warp2d.PASS2}

    def run(job, launches):
        args, kw, buffers, _ = job
        return warp2d.pipeline2d_warp_batch(*args, launches=launches, buffers=buffers, **kw)

    for job in jobs.values():
        for _ in range(a.warmup):
            for launches in parts.values():
                run(job, launches)
    torch.cuda.synchronize()
    times = {name: {part: [] for part in parts} for name in jobs}
    crop_ms = []
    for _ in range(a.rounds):
        crop_ms.append(timed(crop_variant[0], crop_variant[1], crop_variant[2]))
        for name, job in jobs.items():
            for part, launches in parts.items():
                times[name][part].append(timed(lambda j, l: run(j, l), job, launches))
    res = {"crop_masks9_ms_per_batch_launch": statistics.median(crop_ms), "crop_ms_min_max": [min(crop_ms), max(crop_ms)], "presets": {}}
    for name, job in jobs.items():
        r = {"kind_share": job[3]}
        for part in parts:
            r[f"ms_{part}"] = statistics.median(times[name][part])
            r[f"ms_{part}_min_max"] = [min(times[name][part]), max(times[name][part])]
        r["times_crop"] = r["ms_three_launches"] / res["crop_masks9_ms_per_batch_launch"]
        res["presets"][name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--slices", type=int, default=256)
    ap.add_argument("--side", type=int, default=400, help="raw slices are side +- 10 % on each axis")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--with-3d", action="store_true", help="run tools/bench_input_pipeline.py (the 3-D kernel) in a child process too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--warped-out", default=None, help="also time the warping presets and write their figures here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(12342)
    lo, hi = int(a.side * 0.9), int(a.side * 1.1)
    shapes = [(int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for _ in range(a.slices)]
    raws = [rng.integers(-1000, 2200, s).astype(np.int16) for s in shapes]
    masks = [(rng.random((9,) + s) < 0.05).astype(np.uint8) for s in shapes]
    store = SliceStore2D(raws, masks, device="cuda:0")
    del raws, masks
    idx = rng.permutation(a.slices)[:a.batch]
    variants = {}
    for name, pipe in (("crop", predefined.windowed_degree_2["train"]), ("resize", predefined.windowed_degree_2["test"])):
        Ho, Wo = pipe.size
        table = np.zeros((a.batch, 8), dtype=np.int64)
        table[:, :4] = store.table[idx]
        if pipe.mode == CROP:
            table[:, 4:] = pipe.draw_params(table[:, 2:4], np.random.default_rng(1))
        src_px = Ho * Wo * a.batch if pipe.mode == CROP else int((table[:, 2] * table[:, 3]).sum())
        for squash in (False, True):
            p = pipe.squashing(squash)
            byts = 2 * src_px + Ho * Wo * a.batch * (9 + 3 * 4 + (1 if squash else 9))
            variants[f"{name}_{'squash' if squash else 'masks9'}"] = (p, table, byts)

    def bare(p, table):
        return pipeline2d_batch(store, table, p.mode, p.size, p.windows, p.shift, p.mean, p.denom, want_masks=not p.squash,
                                want_labels=p.squash, want_present=True)

    def whole(p, table):
        return p(store, idx, params=table[:, 4:] if p.mode == CROP else None)

    def timed(fn, p, table):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.reps):
            fn(p, table)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.reps

    for p, table, _ in variants.values():
        for _ in range(a.warmup):
            bare(p, table)
            whole(p, table)
    torch.cuda.synchronize()
    times = {k: {"launch": [], "call": []} for k in variants}
    for _ in range(a.rounds):
        for k, (p, table, _) in variants.items():
            times[k]["launch"].append(timed(bare, p, table))
            times[k]["call"].append(timed(whole, p, table))
    res = {"workload": {"batch": a.batch, "raw": f"{lo}..{hi} square-ish int16 + 9 uint8 masks", "out": "3 x 256 x 256 fp32",
                        "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup}, "variants": {}}
    for k, (p, table, byts) in variants.items():
        ms = statistics.median(times[k]["launch"])
        res["variants"][k] = {"ms_per_batch_launch": ms, "ms_launch_min_max": [min(times[k]["launch"]), max(times[k]["launch"])],
                              "ms_per_batch_whole_call": statistics.median(times[k]["call"]), "bytes_algorithmic": byts,
                              "GBps_algorithmic": byts / ms / 1e6, "us_per_slice": 1e3 * ms / a.batch}
    if a.with_3d:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_input_pipeline.py")], check=True, capture_output=True,
                             text=True, timeout=300).stdout
        res["resize3d_to_hwd_same_box"] = json.loads(out.strip().splitlines()[-1])
    if a.warped_out:
        p, table, _ = variants["crop_masks9"]
        res["warped"] = bench_warped(a, store, idx, timed, (bare, p, table))
        with open(a.warped_out, "w") as f:
            f.write(json.dumps({"workload": res["workload"], **res["warped"]}) + "\n")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
