#!/usr/bin/env python3
"""InstanceNorm vs BatchNorm training step of config B on one MI355X, in one process.

    python tools/bench_norm_kinds.py [--steps 24] [--warmup 3] [--rounds 4] [--only instance|batch]

Workload: UNet(3, 1, 10, (32, 64, 128, 256), (2, 2, 2, 2), num_res_units=2) with norm="INSTANCE" and norm="BATCH", bf16 storage,
on 2 x 1 x 512 x 512 x 48 (bench.py's synthetic batch).  A step = forward -> device cross-entropy (fused into the logits
convolution) -> backward -> Adam (BaseUNet3D.fit_step).  Both models warm up first; the timed steps then alternate between them
in `--rounds` blocks of steps / rounds each, so drift of the box (clocks, temperature) lands on both.  Prints one JSON line with
ms/step of both.  `--only` runs one of them alone (for a kernel trace of that step).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ct-image-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench import FILTERS, SEED, synthetic_batch  # noqa: E402


def make(norm, dev):
    from capstone_amd.models import UNet
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(SEED)
    m = BaseUNet3D(filters=list(FILTERS), loss_fx=["CrossEntropy"], precision="bf16", batch_size=2)
    if norm == "BATCH":
        torch.manual_seed(SEED)
        m.unet = UNet(3, 1, 10, list(FILTERS), [2, 2, 2, 2], num_res_units=2, norm="BATCH", precision="bf16")
    return m.to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", choices=["instance", "batch"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    batch = synthetic_batch(2, 512, 512, 48, dev, SEED)
    kinds = ["INSTANCE", "BATCH"] if a.only is None else [a.only.upper()]
    models = {k: make(k, dev) for k in kinds}
    for k in kinds:
        for _ in range(a.warmup):
            models[k].fit_step(batch, keep_logits=False)
    torch.cuda.synchronize()
    per = max(1, a.steps // a.rounds)
    total = {k: 0.0 for k in kinds}
    loss = {}
    for _ in range(a.rounds):
        for k in kinds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                out = models[k].fit_step(batch, keep_logits=False)
            torch.cuda.synchronize()
            total[k] += time.perf_counter() - t0
            loss[k] = float(out.item())
    n = per * a.rounds
    res = {"workload": "UNet(3,1,10,(32,64,128,256),(2,2,2,2),2) training step, 2x1x512x512x48 bf16, fwd+CE+bwd+Adam",
           "timed_steps_each": n, "warmup_each": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(dev)}
    for k in kinds:
        res[f"ms_per_step_{k.lower()}"] = round(total[k] / n * 1e3, 3)
        res[f"loss_last_{k.lower()}"] = loss[k]
    if len(kinds) == 2:
        res["batch_over_instance"] = round(total["BATCH"] / total["INSTANCE"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
