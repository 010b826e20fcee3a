"""Times the two-target loss pass of the mixup step (ctseg_seg_loss_pair: statistics + gradient) against what it replaces, two
runs of the single-target passes (ctseg_seg_loss: statistics + gradient each, the second on a gathered label map), at the 2-D
training shape.  One process, device events, the two variants alternating; writes one JSON record.

  python tools/bench_mixup_loss_pass.py --out profiles/mixup_loss_pass.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))

from capstone_amd import segloss  # noqa: E402
from capstone_amd._native import BF16  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    B, S, C, ld, g_ld = a.batch, a.size * a.size, 10, 12, 12
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.zeros((B, S, ld), device=dev)
    logits[..., :C] = torch.randn((B, S, C), device=dev, generator=g)
    labels = torch.randint(0, C, (B, S), device=dev, generator=g).to(torch.uint8)
    index = torch.randint(0, B, (B,), device=dev, generator=g)
    gathered = labels[index].contiguous()
    hist = torch.zeros((B, C), dtype=torch.int64, device=dev)
    dl = torch.zeros((B, S, g_ld), dtype=torch.bfloat16, device=dev)
    pair = segloss.SegLossPairEngine(dev, B, S, C)
    pair.set_pair(labels, hist, index)
    single = segloss.SegLossEngine(dev, B, S, C)
    pair.coef2.uniform_(-1e-3, 1e-3)
    single.coef.uniform_(-1e-3, 1e-3)

    def run_pair():
        pair.stats_pair(logits.data_ptr(), ld)
        pair.grad_pair(logits.data_ptr(), ld, dl.data_ptr(), g_ld, BF16)

    def run_single_twice():
        for lab in (labels, gathered):
            single.set_labels(lab, hist)
            single.stats(logits.data_ptr(), ld)
            single.grad(logits.data_ptr(), ld, dl.data_ptr(), g_ld, BF16)

    times = {"pair": [], "single_twice": []}
    for i in range(a.warmup + a.reps):
        for name, fn in (("pair", run_pair), ("single_twice", run_single_twice)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    rec = {"shape": {"B": B, "H": a.size, "W": a.size, "C": C, "logits": "fp32 ld 12", "dlogits": "bf16 ld 12"},
           "reps": a.reps, "pair_ms_median": med["pair"], "single_twice_ms_median": med["single_twice"],
           "pair_ms_min_max": [min(times["pair"]), max(times["pair"])],
           "single_twice_ms_min_max": [min(times["single_twice"]), max(times["single_twice"])],
           "ratio_pair_over_single_twice": med["pair"] / med["single_twice"],
           "note": "single_twice leaves out the gather of the second label map and the add of the two gradients"}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
