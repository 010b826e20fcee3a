"""Numpy / plain Python oracle of the connected components: TEST INFRASTRUCTURE, independent of scipy and of the product.

A flood fill with an explicit stack over the neighbour offsets of the given connectivity and axes, started at every unvisited voxel
in raster order, so that the first voxel of a component is its representative.  It gives the canonical ``ids`` (smallest linear
index of the component within the sample, -1 off the classes) and ``sizes`` (voxel count at the representative, 0 elsewhere); the
table and the cleaned map follow from those by the rules of include/ctseg_hip.h.  That form is unique, so every comparison with it
is ``array_equal``.
"""
import itertools

import numpy as np

C = 10
ALL = (1 << C) - 2


def neighbour_offsets(connectivity, axes=7):
    return [d for d in itertools.product((-1, 0, 1), repeat=3)
            if any(d) and all((axes >> a) & 1 or d[a] == 0 for a in range(3)) and sum(map(abs, d)) <= connectivity]


_LABEL_CACHE = {}


def label_oracle(L, connectivity, n_classes=C, axes=7):
    """(B, X, Y, Z) uint8 -> (ids, sizes) int32 of that shape"""
    key = (L.tobytes(), L.shape, connectivity, n_classes, axes)
    if key in _LABEL_CACHE:
        return _LABEL_CACHE[key]
    B, X, Y, Z = L.shape
    ids, sizes = np.full(L.shape, -1, np.int32), np.zeros(L.shape, np.int32)
    sx, sy = (Y + 2) * (Z + 2), Z + 2
    steps = [dx * sx + dy * sy + dz for dx, dy, dz in neighbour_offsets(connectivity, axes)]
    for b in range(B):
        P = np.zeros((X + 2, Y + 2, Z + 2), np.uint8)                      # a border of zeros: no bounds checks, no wrap-around
        P[1:-1, 1:-1, 1:-1] = np.where(L[b] < n_classes, L[b], 0)
        flat = P.ravel().tolist()
        seen = bytearray(len(flat))
        idb, szb = ids[b].reshape(-1), sizes[b].reshape(-1)
        for start in np.flatnonzero(P.ravel()).tolist():                  # raster order of the padded and of the plain volume
            if seen[start]:
                continue
            v, stack, members = flat[start], [start], [start]
            seen[start] = 1
            while stack:
                p = stack.pop()
                for s in steps:
                    q = p + s
                    if flat[q] == v and not seen[q]:
                        seen[q] = 1
                        stack.append(q)
                        members.append(q)
            m = np.asarray(members)
            lin = ((m // sx - 1) * Y + (m % sx) // sy - 1) * Z + m % sy - 1
            rep = int(lin.min())
            assert rep == lin[0]
            idb[lin] = rep
            szb[rep] = len(lin)
    _LABEL_CACHE[key] = (ids, sizes)
    return ids, sizes


def keep_oracle(L, ids, sizes, n_classes=C, class_mask=ALL, keep_largest=True, min_size=0):
    """-> (cleaned map, table (B, C-1, 4) int32) by the rules of the header"""
    B = L.shape[0]
    out, table = L.copy(), np.zeros((B, n_classes - 1, 4), np.int32)
    table[:, :, 2] = -1
    for b in range(B):
        lb, ib, sb = L[b].reshape(-1), ids[b].reshape(-1), sizes[b].reshape(-1)
        ob = out[b].reshape(-1)
        for c in range(1, n_classes):
            reps = np.flatnonzero((sb > 0) & (lb == c))
            if not len(reps):
                continue
            winner = int(reps[np.argmax(sb[reps])])                        # the first of the largest: the smallest representative
            table[b, c - 1, :3] = [len(reps), sb[winner], winner]
            if (class_mask >> c) & 1:
                of_c = np.flatnonzero(lb == c)
                keep = sb[ib[of_c]] >= min_size
                if keep_largest:
                    keep &= ib[of_c] == winner
                ob[of_c[~keep]] = 0
                table[b, c - 1, 3] = int((~keep).sum())
    return out, table


def full_oracle(L, connectivity, n_classes=C, class_mask=ALL, keep_largest=True, min_size=0, axes=7):
    ids, sizes = label_oracle(L, connectivity, n_classes, axes)
    return (ids, sizes) + keep_oracle(L, ids, sizes, n_classes, class_mask, keep_largest, min_size)
