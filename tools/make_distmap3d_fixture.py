#!/usr/bin/env python
"""Writes tests/golden/distmap3d_reference.npz: a few (9, X, Y, Z) uint8 mask stacks and the float64 output of the REFERENCE's own
``compute_distance_map`` (capstone/data/utils.py: rank-agnostic, scipy's N-D distance_transform_edt per class) for them.

    python tools/make_distmap3d_fixture.py --reference /path/to/reference/checkout

The reference module is loaded by file path; needs numpy and scipy.  Nothing under tests/ imports the reference: the tests read the
recorded arrays only.  No volume is all foreground (the reference has no defined value there).
"""
import argparse
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def balls(rng, shape, n, value=1):
    X, Y, Z = shape
    xx, yy, zz = np.mgrid[:X, :Y, :Z]
    m = np.zeros(shape, np.uint8)
    for _ in range(n):
        cx, cy, cz, r = rng.uniform(0, X), rng.uniform(0, Y), rng.uniform(0, Z), rng.uniform(1.0, max(2.0, min(shape) / 2.5))
        m[(xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2 <= r * r] = value
    return m


def stack_balls(rng, shape=(12, 15, 9)):
    """overlapping structures (volume 1 lies inside volume 5), an absent class (4), mask values other than 1"""
    m = np.stack([balls(rng, shape, int(rng.integers(1, 4)), value) for value in (1, 2, 1, 255, 1, 1, 7, 1, 1)])
    m[5] |= balls(rng, shape, 2)
    m[1] = np.where(balls(rng, shape, 3) > 0, m[5], 0) * 2
    m[4] = 0
    assert m[1].any() and all(v.any() for i, v in enumerate(m) if i != 4)
    return m


def stack_patterns(shape=(7, 9, 5)):
    X, Y, Z = shape
    m = np.zeros((9,) + shape, np.uint8)
    m[0, 0, 0, 0] = 1                                     # corner voxels
    m[0, X - 1, Y - 1, Z - 1] = 2
    m[1] = 1
    m[1, 3, 6, 2] = 0                                     # everything foreground but one voxel
    m[2, ::2] = 1                                         # stripes along each axis in turn
    m[3, :, 1::2] = 1
    m[4, :, :, ::2] = 3
    i, j, k = np.ogrid[:X, :Y, :Z]
    m[5] = ((i + j + k) % 2).astype(np.uint8)             # 3-D checkerboard
    m[6, X - 1] = 1                                       # the last slab on each axis
    m[7, :, Y - 1] = 9
    m[8, :, :, Z - 1] = 1
    return m


def stack_long(axis):
    """300 voxels along one axis: that axis's pass sees distances beyond 255, outside a structure and inside one"""
    shape = {0: (300, 3, 4), 1: (4, 300, 3), 2: (3, 4, 300)}[axis]
    m = np.zeros((9,) + shape, np.uint8)

    def along(lo, hi):                                    # a slice of the long axis, everything of the two short ones
        idx = [slice(None)] * 3
        idx[axis] = slice(lo, hi)
        return tuple(idx)
    m[0][along(2, 6)] = 1                                 # far end: floor(d) reaches 294
    m[1, 0, 0, 0] = 1                                     # one corner voxel
    m[2][along(0, 280)] = 3
    m[3][tuple(s - 1 for s in shape)] = 1                 # the opposite corner
    m[4] = 0                                              # absent
    m[5][along(100, 140)] = 1
    m[6][along(120, 160)] = 1                             # overlaps 5
    m[7][tuple(slice(None, None, 2) if a == axis else slice(None) for a in range(3))] = 1      # stripes across the long axis: ties
    m[8] = 1
    m[8][tuple(s - 1 if a == axis else 1 for a, s in enumerate(shape))] = 0    # all but one voxel: inside distances up to 299
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds capstone/data/utils.py)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "distmap3d_reference.npz"))
    args = ap.parse_args()
    if not hasattr(np, "bool"):                           # the reference was written for numpy < 1.24 (``astype(np.bool)``)
        np.bool = np.bool_
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(args.reference, "capstone", "data", "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20261019)
    stacks = {"balls": stack_balls(rng), "patterns": stack_patterns(), "long_z": stack_long(2), "long_y": stack_long(1),
              "long_x": stack_long(0)}
    arrays = {}
    for name, m in stacks.items():
        assert m.dtype == np.uint8 and m.ndim == 4 and m.shape[0] == 9 and not m.all(axis=(1, 2, 3)).any()
        out = ref.compute_distance_map(m)
        assert out.dtype == np.float64 and out.shape == m.shape
        arrays[f"{name}_masks"], arrays[f"{name}_maps"] = m, out
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
