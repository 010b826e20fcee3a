"""Numpy oracle of the hole filling (ctseg_fill_holes, capstone_amd.components.fill_holes) and its entry-point emulator: TEST
INFRASTRUCTURE, independent of scipy and of the product.

The rule, restated from include/ctseg_hip.h.  A background component is a maximal set of voxels of label exactly 0 joined by neighbour
steps (+-1 along at most ``connectivity`` active axes, inside the sample).  It touches the boundary when one of its voxels has
coordinate 0 or side - 1 along an active axis.  Its border set holds the labels of all neighbours of its voxels that are not 0, a
label >= n_classes counting as one foreign label.  It is a hole of class c when it does not touch the boundary, its border set is
exactly {c} with 1 <= c < n_classes, c is in the class mask and max_size == 0 or it has at most max_size voxels; its voxels then
become c.  Everything else is copied.  One pass.

The components come from the flood fill of component_oracles.label_oracle run on the map ``L == 0``; the boundary test and the
border set are taken per component, as sets, from the definition.
"""
import numpy as np

from abi_emulator import mem
from component_oracles import C, label_oracle, neighbour_offsets

OTHER = -1                                 # the one foreign label that stands for every label >= n_classes


def background_components(L, connectivity, n_classes=C, axes=7):
    """-> a list per sample of dicts: ``voxels`` (linear indices within the sample, ascending), ``boundary`` (bool), ``border`` (a set
    of class indices and OTHER)"""
    B, X, Y, Z = L.shape
    ids, sizes = label_oracle((L == 0).astype(np.uint8), connectivity, 2, axes)
    offsets = neighbour_offsets(connectivity, axes)
    side, active = (X, Y, Z), [(axes >> a) & 1 for a in range(3)]
    res = []
    for b in range(B):
        P = np.zeros((X + 2, Y + 2, Z + 2), np.int32)                      # a border of zeros: outside the sample is no neighbour
        P[1:-1, 1:-1, 1:-1] = L[b]
        comps, flat = [], ids[b].reshape(-1)
        bg = np.flatnonzero(flat >= 0)
        order = bg[np.argsort(flat[bg], kind="stable")]                    # the voxels grouped by representative, ascending in each
        reps, starts = np.unique(flat[order], return_index=True)
        for rep, vox in zip(reps.tolist(), np.split(order, starts[1:]) if len(order) else []):
            assert vox[0] == rep and len(vox) == sizes[b].reshape(-1)[rep]
            co = np.stack(np.unravel_index(vox, (X, Y, Z)))
            boundary = any(active[a] and ((co[a] == 0) | (co[a] == side[a] - 1)).any() for a in range(3))
            border = set()
            for d in offsets:
                nb = P[co[0] + 1 + d[0], co[1] + 1 + d[1], co[2] + 1 + d[2]]
                border |= {int(v) if v < n_classes else OTHER for v in np.unique(nb[nb != 0]).tolist()}
            comps.append(dict(voxels=vox, boundary=bool(boundary), border=border))
        res.append(comps)
    return res


def fill_oracle(L, connectivity, n_classes=C, class_mask=None, max_size=0, axes=7, want_rejected=False):
    """(B, X, Y, Z) uint8 -> (filled map, table (B, n_classes - 1, 2) int32 of {holes filled, voxels filled}); with ``want_rejected``
    also the number of components that do not touch the boundary and whose border set has more than one member"""
    if class_mask is None:
        class_mask = (1 << n_classes) - 2
    B = L.shape[0]
    out, table, mixed = L.copy(), np.zeros((B, n_classes - 1, 2), np.int32), 0
    for b, comps in enumerate(background_components(L, connectivity, n_classes, axes)):
        ob = out[b].reshape(-1)
        for comp in comps:
            if comp["boundary"]:
                continue
            mixed += len(comp["border"]) > 1
            if len(comp["border"]) != 1:
                continue
            c = next(iter(comp["border"]))
            if c == OTHER or not (class_mask >> c) & 1 or (max_size != 0 and len(comp["voxels"]) > max_size):
                continue
            ob[comp["voxels"]] = c
            table[b, c - 1] += [1, len(comp["voxels"])]
    return (out, table, mixed) if want_rejected else (out, table)


class FillHolesEntries:
    """ctseg_fill_holes IS fill_oracle; composes with feature_emulators.ComponentsEntries and abi_emulator.Emulator, whose launch
    counter ``calls`` it shares: one call is one launch group"""
    calls = 0

    def fill_holes(self, labels, B, X, Y, Z, n_classes, connectivity, axes, class_mask, max_size, workspace, workspace_bytes, out,
                   table):
        n, K = B * X * Y * Z, n_classes - 1
        assert labels and workspace and out and table and workspace % 16 == 0 and workspace_bytes >= 13 * n and n < 1 << 31
        assert 1 <= connectivity <= 3 and 1 <= axes <= 7 and max_size >= 0 and class_mask & ~((1 << n_classes) - 2) == 0
        mem(workspace, workspace_bytes, np.uint8)[:] = 0xA5                # the call may leave anything there
        o, t = fill_oracle(mem(labels, n, np.uint8).reshape(B, X, Y, Z).copy(), connectivity, n_classes, class_mask, max_size, axes)
        mem(out, n, np.uint8)[:] = o.reshape(-1)
        mem(table, B * K * 2, np.int32)[:] = t.reshape(-1)
        self.calls += 1
