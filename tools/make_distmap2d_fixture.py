#!/usr/bin/env python
"""Writes tests/golden/distmap2d_reference.npz: a few (9, H, W) uint8 mask stacks and the float64 output of the REFERENCE's own
``compute_distance_map`` (capstone/data/utils.py, scipy's distance_transform_edt) for them.

    python tools/make_distmap2d_fixture.py --reference /path/to/reference/checkout

The reference module is loaded by file path; needs numpy and scipy.  Nothing under tests/ imports the reference: the tests read the
recorded arrays only.  No plane is all foreground (the reference has no defined value there).
"""
import argparse
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def discs(rng, shape, n, value=1):
    H, W = shape
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros(shape, np.uint8)
    for _ in range(n):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.0, max(2.0, min(H, W) / 3))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value
    return m


def stack_discs(rng, shape):
    """overlapping structures (plane 1 lies inside plane 5), an absent class (4), mask values other than 1"""
    m = np.stack([discs(rng, shape, int(rng.integers(1, 4)), value) for value in (1, 2, 1, 255, 1, 1, 7, 1, 1)])
    m[5] |= discs(rng, shape, 2)
    m[1] = np.where(discs(rng, shape, 3) > 0, m[5], 0) * 2
    m[4] = 0
    assert m[1].any() and not m.all(axis=(1, 2)).any()
    return m


def stack_long(rng):
    """40 x 330: distances pass 255 outside (a structure at one end) and the wrap shows inside too (a wide structure)"""
    shape = (40, 330)
    m = np.zeros((9,) + shape, np.uint8)
    m[0, 18:22, 2:6] = 1                                  # far end: floor(d) reaches 323
    m[1, 0, 0] = 1                                        # one corner pixel
    m[2, :, :300] = 3                                     # inside distances up to 20; outside up to 30
    m[3, 39, 329] = 1
    m[4] = 0                                              # absent
    m[5] = discs(rng, shape, 3)
    m[5, 10:30, 100:140] = 1
    m[6, 10:30, 120:160] = 1                              # overlaps 5
    m[7, :, ::2] = 1                                      # vertical stripes: ties
    m[8] = 1
    m[8, 20, 329] = 0                                     # everything foreground but one pixel: inside distances up to 329
    return m


def stack_patterns():
    shape = (17, 23)
    m = np.zeros((9,) + shape, np.uint8)
    m[0, 0, 0] = 1
    m[1, 16, 22] = 2
    m[2] = 1
    m[2, 8, 11] = 0
    m[3, ::2, :] = 1                                      # horizontal stripes
    m[4] = (np.add.outer(np.arange(17), np.arange(23)) % 2).astype(np.uint8)      # checkerboard
    m[5, 16, :] = 1                                       # last row
    m[6, :, 22] = 9                                       # last column
    m[7, 3:9, 4:15] = 1
    m[8, 5:12, 10:20] = 1                                 # overlaps 7
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds capstone/data/utils.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "distmap2d_reference.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(args.reference, "capstone", "data", "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20261019)
    stacks = {"discs": stack_discs(rng, (24, 31)), "discs_small": stack_discs(rng, (9, 13)), "long": stack_long(rng),
              "patterns": stack_patterns()}
    arrays = {}
    for name, m in stacks.items():
        assert m.dtype == np.uint8 and m.shape[0] == 9 and not m.all(axis=(1, 2)).any()
        out = ref.compute_distance_map(m)
        assert out.dtype == np.float64 and out.shape == m.shape
        arrays[f"{name}_masks"], arrays[f"{name}_maps"] = m, out
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
