"""Connected components on the device: ctseg_components_label, ctseg_components_keep, capstone_amd.components
(connected_components, keep_largest_component, KeepLargestConnectedComponent) and the BaseUNet3D switch ``largest_component``.

Held to tests/component_oracles.py, a flood fill in numpy and plain Python that gives the canonical ``ids`` and ``sizes``; that form
is unique, so every comparison is ``array_equal``: there are no tolerances here.

CPU tests route the two entries through an emulator that IS the oracle; GPU tests hold the kernels to the oracle.

The kernels' tiles: the local pass labels tiles of 8 x 16 x 32 voxels (X, Y, Z) in LDS, a lane owning a run of 16 voxels along Z
(Z a multiple of 16 takes the 16-byte path); the merge pass unites across tile faces, the apply pass of the keep rewrites runs of 16
consecutive voxels of a sample.  (9, 17, 33) is one tile plus one voxel on every side; (40, 24, 40) is 5 x 2 x 2 tiles.  No kernel
is persistent, so CTSEG_MAX_WG does not bear on them.  Every volume here has at most 1e5 voxels.
"""
import os
import re

import numpy as np
import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import STRUCTURES, components, segloss, surface
from capstone_amd import _native as nat
from capstone_amd.training.utils import _squash_predictions
from capstone_amd.volumetric.metrics import DiceMetricWrapper3D
from component_oracles import ALL, C, full_oracle, keep_oracle, label_oracle, neighbour_offsets
from distance_oracles import ball_labels, check_tables, nan_reduce
from distance_oracles import surface_oracle
from feature_emulators import ComponentsEntries, SurfaceEntries
from helpers import as_numpy

DEV = "cuda:0"
TILE = (8, 16, 32)


class E(ComponentsEntries, SurfaceEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E()) as e:
        yield e


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def random_labels(shape, density, seed, hi=9):
    """labels 1..hi at `density` of the voxels, 0 elsewhere: samples and classes touch everywhere"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, hi + 1, shape), 0).astype(np.uint8)


def serpentine(shape, label, off, L=None):
    """one 6-connected component of `label`: full Z lines at y = off (mod 4) in the planes x = off (mod 4), joined at alternating
    Z ends inside a plane and by a bridge along X at (y, z) = (off, 0) between planes"""
    X, Y, Z = shape
    L = np.zeros(shape, np.uint8) if L is None else L
    xs, ys = range(off, X, 4), range(off, Y, 4)
    for x in xs:
        for j, y in enumerate(ys):
            L[x, y, :] = label
            if y + 4 < Y:
                L[x, y:y + 4, Z - 1 if j % 2 == 0 else 0] = label
        if x + 4 < X:
            L[x:x + 4, off, 0] = label
    return L


def island_pair():
    """(1, 24, 24, 48) prediction and truth of class 3: a ball of radius 3.2 around (8, 8, 8), moved by one voxel in the prediction,
    which also holds an island of 2 x 3 x 3 voxels at z >= 41: at least 29 voxels from the truth"""
    g = np.mgrid[:24, :24, :48]
    truth = np.zeros((1, 24, 24, 48), np.uint8)
    pred = truth.copy()
    truth[0][(g[0] - 8) ** 2 + (g[1] - 8) ** 2 + (g[2] - 8) ** 2 <= 3.2 ** 2] = 3
    pred[0][(g[0] - 9) ** 2 + (g[1] - 8) ** 2 + (g[2] - 8) ** 2 <= 3.2 ** 2] = 3
    pred[0, 20:22, 19:22, 41:44] = 3
    return pred, truth


# ---- CPU tests: the oracle ---------------------------------------------------------------------------------------------------
def test_the_oracle_on_hand_made_maps():
    assert [len(neighbour_offsets(k)) for k in (1, 2, 3)] == [6, 18, 26]
    assert [len(neighbour_offsets(k, axes=3)) for k in (1, 2, 3)] == [4, 8, 8]
    L = np.zeros((2, 3, 4, 5), np.uint8)
    L[0, 0, 0, 4] = L[0, 0, 1, 0] = 2                                      # the end of a Z row and the start of the next
    L[0, 2, 3, 4] = L[1, 0, 0, 0] = 5                                      # the end of a sample and the start of the next
    L[1, 1, 1, 1] = L[1, 2, 2, 2] = 7                                      # a corner step
    L[1, 1, 3, 3] = L[1, 1, 2, 4] = 8                                      # an edge step
    L[1, 0, 3, 0:3] = 12                                                   # past the classes
    for k in (1, 2, 3):
        ids, sizes, out, table = full_oracle(L, k)
        assert ids[0, 0, 0, 4] == 4 and ids[0, 0, 1, 0] == 5 and ids[0, 2, 3, 4] == 59 and ids[1, 0, 0, 0] == 0
        assert (ids[1, 2, 2, 2] == ids[1, 1, 1, 1]) == (k == 3) and (ids[1, 1, 3, 3] == ids[1, 1, 2, 4]) == (k >= 2)
        assert (ids[L >= C] == -1).all() and (ids[L == 0] == -1).all() and (out[L >= C] == 12).all()
        assert table[0, 1].tolist() == [2, 1, 4, 1] and table[1, 6].tolist() == ([1, 2, 26, 0] if k == 3 else [2, 1, 26, 1])
        assert table[0, 0].tolist() == [0, 0, -1, 0] and sizes.sum() == (L > 0).sum() - 3


def test_the_oracle_partitions_like_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    L = random_labels((1, 9, 10, 11), 0.6, 5, hi=3)
    for k in (1, 2, 3):
        ids, sizes = label_oracle(L, k, 4)
        for c in (1, 2, 3):
            lab, n = ndi.label(L[0] == c, ndi.generate_binary_structure(3, k))
            m = L[0] == c
            assert n == int(((sizes[0] > 0) & m).sum())
            pairs = np.unique(np.stack([lab[m], ids[0][m]]), axis=1)      # scipy's id <-> representative: one to one
            assert pairs.shape[1] == n and len(set(pairs[0])) == len(set(pairs[1])) == n
    tie = np.zeros((1, 4, 4, 12), np.uint8)                                # two largest of three voxels, then one of two
    tie[0, 2, 1, 5:8] = tie[0, 0, 3, 0:3] = tie[0, 3, 3, 9:11] = 1
    ids, sizes, out, table = full_oracle(tie, 3, 2, class_mask=2)
    lab, n = ndi.label(tie[0] == 1, ndi.generate_binary_structure(3, 3))
    winner = int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
    assert n == 3 and np.array_equal(out[0] != 0, lab == winner) and table[0, 0].tolist() == [3, 3, 36, 5]


# ---- CPU tests: the Python layer through the emulator ------------------------------------------------------------------------
def test_components_through_the_emulator(emu, monkeypatch):
    L = random_labels((3, 5, 6, 7), 0.5, 1, hi=11)
    t = torch.from_numpy(L)
    for k in (None, 1, 2, 3):
        ids, sizes, out, table = full_oracle(L, 3 if k is None else k)
        calls = emu.calls
        cc = components.connected_components(t, connectivity=k)
        assert emu.calls == calls + 2                                        # one launch group: a label and a keep call
        assert cc.ids.dtype == cc.sizes.dtype == torch.int32 and cc.count.dtype == torch.int64 and cc.count.shape == (3, 9)
        assert np.array_equal(cc.ids.numpy(), ids) and np.array_equal(cc.sizes.numpy(), sizes)
        assert np.array_equal(cc.count.numpy(), table[..., 0])
        res = components.keep_largest_component(t.long(), connectivity=k)
        assert res.labels.dtype == torch.int64 and np.array_equal(res.labels.numpy(), out)
        for name, col in (("count", 0), ("largest", 1), ("representative", 2), ("removed", 3)):
            got = getattr(res, name)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), table[..., col]), name
    # launch grouping: by request, and by the working-set bound
    ids, sizes, out, table = full_oracle(L, 3)
    calls = emu.calls
    one = components.keep_largest_component(t, samples_per_launch=1)
    assert emu.calls == calls + 6 and np.array_equal(one.labels.numpy(), out) and np.array_equal(one.removed.numpy(), table[..., 3])
    two = components.keep_largest_component(t, samples_per_launch=2)
    assert emu.calls == calls + 10 and np.array_equal(two.labels.numpy(), out) and np.array_equal(two.count.numpy(), table[..., 0])
    monkeypatch.setattr(components, "MAX_WORKING_SET", components.BYTES_PER_VOXEL * 5 * 6 * 7 * 2)
    calls = emu.calls
    assert np.array_equal(components.connected_components(t).ids.numpy(), ids) and emu.calls == calls + 4
    assert components.BYTES_PER_VOXEL == 10


def test_the_keep_switches_through_the_emulator(emu):
    L = random_labels((2, 6, 5, 9), 0.45, 2)
    t = torch.from_numpy(L)
    ids, sizes = label_oracle(L, 1)
    for kw, (mask, largest, size) in ((dict(applied_labels=[2, 5, 9]), (1 << 2 | 1 << 5 | 1 << 9, True, 0)),
                                      (dict(applied_labels=(c for c in (1,))), (2, True, 0)),
                                      (dict(applied_labels=[]), (0, True, 0)),
                                      (dict(min_size=3, keep_largest=False), (ALL, False, 3)),
                                      (dict(min_size=4), (ALL, True, 4)),
                                      (dict(applied_labels=np.array([3, 4]), min_size=2, keep_largest=False), (1 << 3 | 1 << 4, False, 2))):
        out, table = keep_oracle(L, ids, sizes, C, mask, largest, size)
        res = components.keep_largest_component(t, connectivity=1, **kw)
        assert np.array_equal(res.labels.numpy(), out) and np.array_equal(res.removed.numpy(), table[..., 3]), kw
    f = components.KeepLargestConnectedComponent(applied_labels=[1, 2], connectivity=2, min_size=2)
    out, table = full_oracle(L, 2, class_mask=6, min_size=2)[2:]
    assert np.array_equal(f(t).numpy(), out) and np.array_equal(f.last.largest.numpy(), table[..., 1])
    from capstone_amd.transforms import KeepLargestConnectedComponent
    assert KeepLargestConnectedComponent is components.KeepLargestConnectedComponent
    fewer = components.keep_largest_component(torch.from_numpy(np.minimum(L, 3)), n_classes=3)   # label 3 is past the classes
    assert fewer.count.shape == (2, 2) and np.array_equal(fewer.labels.numpy() == 3, L >= 3)


def test_planes_through_the_emulator(emu):
    L = random_labels((2, 9, 11), 0.55, 3, hi=4)
    for k, full in ((1, 1), (2, 2), (None, 2)):
        ids, sizes, out, table = full_oracle(L[..., None], full, axes=3)
        cc = components.connected_components(torch.from_numpy(L).short(), connectivity=k)
        assert cc.ids.shape == (2, 9, 11) and np.array_equal(cc.ids.numpy(), ids[..., 0]) and np.array_equal(cc.sizes.numpy(), sizes[..., 0])
        res = components.keep_largest_component(torch.from_numpy(L).short(), connectivity=k)
        assert res.labels.dtype == torch.int16 and np.array_equal(res.labels.numpy(), out[..., 0])
    assert not np.array_equal(label_oracle(L[..., None], 1, axes=3)[0], label_oracle(L[..., None], 2, axes=3)[0])


def test_bad_arguments_are_refused(emu):
    a = torch.zeros(2, 4, 4, 4, dtype=torch.uint8)
    calls = emu.calls
    for bad in (a[0, 0], a[None], a.float(), a.bool(), torch.zeros(1, 2, 1025, 2, dtype=torch.uint8),
                torch.zeros(0, 4, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 0, 4, dtype=torch.uint8)):
        for f in (components.connected_components, components.keep_largest_component):
            with pytest.raises(ValueError):
                f(bad)
    for kw in (dict(n_classes=1), dict(n_classes=17), dict(connectivity=0), dict(connectivity=4), dict(connectivity=True),
               dict(connectivity=1.5)):
        for f in (components.connected_components, components.keep_largest_component):
            with pytest.raises(ValueError):
                f(a, **kw)
    with pytest.raises(ValueError):
        components.connected_components(a[0], connectivity=3)             # planes have two axes
    for kw in (dict(applied_labels=[0]), dict(applied_labels=[10]), dict(applied_labels=[1.5]), dict(applied_labels=[-1]),
               dict(applied_labels=[3], n_classes=3), dict(min_size=-1), dict(min_size=1.5), dict(min_size=1 << 31)):
        with pytest.raises(ValueError):
            components.keep_largest_component(a, **kw)
    with pytest.raises(ValueError):
        components.KeepLargestConnectedComponent(applied_labels=[11])(a)
    assert emu.calls == calls


def test_a_cpu_tensor_is_refused():
    a = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    for f in (components.connected_components, components.keep_largest_component, components.KeepLargestConnectedComponent()):
        with pytest.raises(nat.NativeError):
            f(a)


def test_the_library_validates_before_any_launch():
    """ctseg_components_label and ctseg_components_keep themselves; no device is touched: every case fails validation"""
    L = nat.lib()
    err = L.ctseg_last_error

    def label(labels=4096, B=2, X=8, Y=8, Z=8, n=10, conn=3, axes=7, ids=1 << 20, sizes=1 << 21):
        return L.ctseg_components_label(labels, B, X, Y, Z, n, conn, axes, ids, sizes, None)

    def keep(labels=4096, ids=1 << 20, sizes=1 << 21, B=2, X=8, Y=8, Z=8, n=10, mask=ALL, largest=1, min_size=0, ws=1 << 22,
             ws_bytes=None, out=1 << 23, table=1 << 24):
        need = B * (n - 1) * components.KEEP_ROW_BYTES
        return L.ctseg_components_keep(labels, ids, sizes, B, X, Y, Z, n, mask, largest, min_size, ws,
                                       need if ws_bytes is None else ws_bytes, out, table, None)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctseg_hip.h")).read()
    assert int(re.search(r"#define CTSEG_COMPONENTS_KEEP_ROW_BYTES (\d+)", hdr).group(1)) == components.KEEP_ROW_BYTES
    assert "#define CTSEG_ABI_VERSION 3" in hdr
    for call, ptrs in ((label, ("labels", "ids", "sizes")), (keep, ("labels", "ids", "sizes", "ws", "out", "table"))):
        for p in ptrs:
            assert call(**{p: None}) < 0 and b"null pointer" in err(), p
        for kw in (dict(B=0), dict(X=0), dict(Y=0), dict(Z=0), dict(B=-1), dict(Z=-3)):
            assert call(**kw) < 0 and b">= 1" in err()
        for kw in (dict(X=1025), dict(Y=1025), dict(Z=1025)):
            assert call(**kw) < 0 and b"sides up to 1024" in err()
        for kw in (dict(B=2, X=1024, Y=1024, Z=1024), dict(B=2048, X=1024, Y=1024, Z=1), dict(B=65536, X=1, Y=1, Z=1)):
            assert call(**kw) < 0 and b"too many" in err()
        for n in (1, 0, 17, -4):
            assert call(n=n) < 0 and b"classes" in err()
    for conn in (0, 4, -1):
        assert label(conn=conn) < 0 and b"connectivity" in err()
    for axes in (0, 8, -1):
        assert label(axes=axes) < 0 and b"axes" in err()
    for kw in (dict(ids=(1 << 20) + 2), dict(sizes=(1 << 21) + 1), dict(Z=16, labels=4097), dict(Z=16, ids=(1 << 20) + 4),
               dict(Z=16, sizes=(1 << 21) + 8)):
        assert label(**kw) < 0 and b"unaligned" in err()
    for kw in (dict(min_size=-1), dict(largest=2), dict(largest=-1), dict(mask=1), dict(mask=1 << 10), dict(mask=-2)):
        assert keep(**kw) < 0 and (b"min_size" in err() or b"keep_largest" in err() or b"class_mask" in err())
    assert keep(ws_bytes=2 * 9 * 16 - 1) < 0 and b"workspace" in err()
    for kw in (dict(ws=(1 << 22) + 4), dict(ids=(1 << 20) + 2), dict(sizes=(1 << 21) + 1), dict(table=(1 << 24) + 2), dict(labels=4100),
               dict(out=(1 << 23) + 8)):
        assert keep(**kw) < 0 and b"unaligned" in err()
    assert {"ctseg_components_label", "ctseg_components_keep"} <= set(nat.EXPORTS)


# ---- the trainer switch ------------------------------------------------------------------------------------------------------
def _model_and_batches(dev="cpu", **switches):
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(7)
    m = BaseUNet3D(filters=[4, 8, 8], loss_fx=["CrossEntropy"], **switches).to(dev)
    g = torch.Generator().manual_seed(3)
    batches = []
    for s in (0, 1):
        L = ball_labels((16, 16, 8), 40 + s)
        masks = torch.from_numpy(np.stack([(L == c) for c in range(1, C)]).astype(np.uint8))[None]
        batches.append((torch.randn(1, 1, 16, 16, 8, generator=g).to(dev), masks.to(dev), torch.ones(1, 9).to(dev)))
    return m, batches


def _check_lcc_epoch(m, batches, dev="cpu"):
    """two validation steps against the oracle chain: squash -> flood fill -> keep -> Dice counts and surface oracle"""
    assert m.largest_component and "largest_component" not in m.hparams and "largest_component_connectivity" not in m.hparams
    dice, counts, cleaned, truths = [], [], [], []
    with torch.no_grad():
        for b in batches:
            assert m.validation_step(b) is None
            pred = _squash_predictions(m(b[0])).cpu().numpy().astype(np.uint8)
            truth = (b[1][0].cpu().numpy() * np.arange(1, C).reshape(-1, 1, 1, 1)).max(0)[None].astype(np.uint8)
            _, _, out, table = full_oracle(pred, 3)
            mean, per_class = DiceMetricWrapper3D()(torch.from_numpy(out).to(dev), torch.from_numpy(truth).to(dev))
            assert torch.equal(m.logged["Mean Dice Score (val LCC)"], mean)
            assert all(torch.equal(m.logged[f"{s} Dice (val LCC)"], per_class[i]) for i, s in enumerate(STRUCTURES))
            ref = segloss.dice_counts(torch.from_numpy(out).reshape(1, -1).to(dev), torch.from_numpy(truth).reshape(1, -1).to(dev))
            assert torch.equal(m.lcc_dice_score.last_counts, ref)          # exact integers
            assert np.array_equal(ref[0, 1].cpu().numpy(), np.bincount(out.ravel(), minlength=C)[:C])
            counts.append(table[..., 0])
            cleaned.append(out)
            truths.append(truth)
    if m.surface_metrics:
        assert set(m._surface_kept) == {"val", "val LCC"} and len(m._surface_kept["val LCC"]) == 2
        for (hd, assd), out, truth in zip(m._surface_kept["val LCC"], cleaned, truths):
            ref = surface.surface_distances(torch.from_numpy(out).to(dev), torch.from_numpy(truth).to(dev))
            assert torch.equal(hd.isnan(), ref.hd.isnan()) and torch.equal(hd.nan_to_num(-1.0), ref.hd.nan_to_num(-1.0))
            assert torch.equal(assd.nan_to_num(-1.0), ref.assd.nan_to_num(-1.0))
            o = surface_oracle(out, truth)
            assert np.allclose(hd.cpu().numpy(), o["hd"], rtol=0, atol=1e-9, equal_nan=True)
        got = m.epoch_surface_metrics("val LCC", reset=False)
        rm, rpc = nan_reduce(np.concatenate([surface_oracle(o, t)["hd"] for o, t in zip(cleaned, truths)]))
        assert np.allclose(got[1].cpu().numpy(), rpc, rtol=0, atol=1e-9, equal_nan=True)
    m.on_validation_epoch_end()
    mean_count = np.concatenate(counts).astype(np.float64).mean(0)
    for i, s in enumerate(STRUCTURES):
        assert m.logged[f"{s} components (val)"].item() == mean_count[i]
    if m.surface_metrics:
        finite = ~np.isnan(rpc)
        for i, s in enumerate(STRUCTURES):
            assert (f"{s} HD95 (val LCC)" in m.logged) == (f"{s} ASSD (val LCC)" in m.logged) == bool(finite[i])
        assert ("Mean HD95 (val LCC)" in m.logged) == ("Mean ASSD (val LCC)" in m.logged) == bool(finite.any())
        assert m.epoch_surface_metrics("val LCC") is None and m.epoch_surface_metrics("val") is None   # the hook reset both
    assert m._components_kept == []


def test_the_trainer_switch_through_the_emulator(emu):
    off, batches = _model_and_batches()
    assert off.largest_component is False and off.lcc_dice_score is None
    with torch.no_grad():
        off.validation_step(batches[0])
    assert emu.calls == 0 and off.on_validation_epoch_end() is None
    keys_off = set(off.logged)
    assert not any("LCC" in k or "components" in k for k in keys_off)
    surf, _ = _model_and_batches(surface_metrics=True)                     # the surface switch alone: as before, three calls a step
    with torch.no_grad():
        surf.validation_step(batches[0])
    surf.on_validation_epoch_end()
    assert emu.calls == 3 and not any("LCC" in k or "components" in k for k in surf.logged) and set(surf._surface_kept) == {"val"}
    emu.calls = 0
    m, batches = _model_and_batches(largest_component=True)
    _check_lcc_epoch(m, batches)
    assert emu.calls == 4                                                   # a label and a keep call per step, nothing else
    assert set(m.logged) - keys_off == ({f"{s} Dice (val LCC)" for s in STRUCTURES} | {"Mean Dice Score (val LCC)"} |
                                        {f"{s} components (val)" for s in STRUCTURES})
    loss = m.training_step(batches[0])                                      # training steps never run it
    assert emu.calls == 4 and torch.isfinite(loss)
    emu.calls = 0
    both, batches = _model_and_batches(surface_metrics=True, largest_component=True, largest_component_connectivity=3)
    _check_lcc_epoch(both, batches)
    assert emu.calls == 2 * (3 + 2 + 3) + 2 * 3                             # (the check itself scores the two cleaned maps again)
    assert {"Mean HD95 (val)", "Mean Dice Score (val)", "Mean Dice Score (val LCC)"} <= set(both.logged)


# ---- GPU tests: the kernels against the oracle -------------------------------------------------------------------------------
def gpu_run(L, connectivity, n_classes=C, class_mask=ALL, keep_largest=True, min_size=0, axes=7):
    """the two entries on one launch group, every output filled with another value first: -> ids, sizes, out, table"""
    B, X, Y, Z = L.shape
    lab = torch.from_numpy(L).to(DEV)
    ids = torch.full(L.shape, -7, dtype=torch.int32, device=DEV)
    sizes = torch.full(L.shape, -7, dtype=torch.int32, device=DEV)
    out = torch.full(L.shape, 77, dtype=torch.uint8, device=DEV)
    table = torch.full((B, n_classes - 1, 4), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((B * (n_classes - 1) * 2,), -1, dtype=torch.int64, device=DEV)          # the call zeroes it
    nat.call("ctseg_components_label", nat.ptr(lab), B, X, Y, Z, n_classes, connectivity, axes, nat.ptr(ids), nat.ptr(sizes))
    nat.call("ctseg_components_keep", nat.ptr(lab), nat.ptr(ids), nat.ptr(sizes), B, X, Y, Z, n_classes, class_mask, int(keep_largest),
             min_size, nat.ptr(ws), ws.numel() * 8, nat.ptr(out), nat.ptr(table))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (ids, sizes, out, table))


def check_gpu(L, connectivity, **kw):
    got, ref = gpu_run(L, connectivity, **kw), full_oracle(L, connectivity, **kw)
    for name, g, r in zip(("ids", "sizes", "out", "table"), got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r), (name, int((g != r).sum()))
    return ref


@pytest.mark.gpu
def test_gpu_smallest_shapes():
    one = np.full((1, 1, 1, 1), 4, np.uint8)
    for k in (1, 2, 3):
        ids, sizes, out, table = check_gpu(one, k)
        assert ids.item() == 0 and sizes.item() == 1 and out.item() == 4 and table[0, 3].tolist() == [1, 1, 0, 0]
        check_gpu(random_labels((1, 1, 1, 37), 0.6, 11, hi=3), k)
        check_gpu(random_labels((2, 8, 8, 16), 0.5, 12), k)                 # the aligned 16-byte path
    check_gpu(np.zeros((1, 1, 1, 1), np.uint8), 3)
    check_gpu(np.zeros((2, 8, 8, 16), np.uint8), 3)


RANDOM_SHAPES = [(2, 19, 21, 70), (1, 33, 9, 65), (1, 9, 17, 33), (1, 16, 32, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=["x".join(map(str, s)) for s in RANDOM_SHAPES])
def test_gpu_random_labels(shape, density, connectivity):
    """samples and classes touch everywhere, so nothing may merge across a sample, a class or a row end; (9, 17, 33) is a tile
    plus one voxel on every side, (16, 32, 64) whole tiles on the 16-byte path"""
    L = random_labels(shape, density, 100 + int(density * 10))
    ids, sizes, out, table = check_gpu(L, connectivity)
    assert table[..., 0].min() >= 1 and (ids >= 0).sum() == (L > 0).sum() == sizes.sum()


@pytest.mark.gpu
def test_gpu_row_ends_and_sample_ends_do_not_join():
    for shape in ((2, 19, 21, 70), (2, 8, 16, 32)):
        B, X, Y, Z = shape
        L = np.zeros(shape, np.uint8)
        L[0, 3, 4, Z - 1] = L[0, 3, 5, 0] = 6                               # (x, y, Z-1) and (x, y+1, 0)
        L[0, X - 1, Y - 1, Z - 1] = L[1, 0, 0, 0] = 2                       # the same two voxels across the sample boundary
        L[1, 2, Y - 1, Z - 1] = L[1, 3, 0, 0] = 3                           # and across a plane end
        for k in (1, 2, 3):
            ids, sizes, out, table = check_gpu(L, k)
            assert table[0, 5].tolist() == [2, 1, (3 * Y + 4) * Z + Z - 1, 1] and table[1, 2, 0] == 2
            assert table[0, 1].tolist() == [1, 1, X * Y * Z - 1, 0] and table[1, 1].tolist() == [1, 1, 0, 0]


@pytest.mark.gpu
def test_gpu_checkerboard():
    g = np.mgrid[:17, :18, :19]
    L = (((g[0] + g[1] + g[2]) % 2 == 0) * 4).astype(np.uint8)[None]
    n = int((L > 0).sum())
    ids, sizes, out, table = check_gpu(L, 1)                                # every voxel its own component: the most there can be
    assert table[0, 3].tolist() == [n, 1, 0, n - 1] and (out > 0).sum() == 1 and out[0, 0, 0, 0] == 4
    ids, sizes, out, table = check_gpu(L, 3)
    assert table[0, 3].tolist() == [1, n, 0, 0] and np.array_equal(out, L)
    ids, sizes, out, table = check_gpu(L, 2)
    assert table[0, 3].tolist() == [1, n, 0, 0]                             # (face diagonals join a checkerboard)


@pytest.mark.gpu
def test_gpu_serpentines_across_many_tiles():
    shape = (40, 24, 40)
    L = serpentine(shape, 7, 2, serpentine(shape, 1, 0))[None]              # a second class in the gaps of the first
    assert (L == 1).sum() > 2000 and (L == 7).sum() > 2000
    for k in (1, 2, 3):
        ids, sizes, out, table = check_gpu(L, k)
        assert table[0, 0].tolist() == [1, int((L == 1).sum()), 0, 0] and table[0, 6, :2].tolist() == [1, int((L == 7).sum())]
    cut = L.copy()
    cut[0, 20, 0, 17] = cut[0, 22, 2, 21] = 0                               # each class in two pieces: the smaller ones go
    ids, sizes, out, table = check_gpu(cut, 1)
    assert table[0, 0, 0] == table[0, 6, 0] == 2 and table[0, 0, 3] > 100 and table[0, 6, 3] > 100
    both = np.concatenate([L, cut])                                         # two samples in one launch
    check_gpu(both, 1)


@pytest.mark.gpu
def test_gpu_tile_corners_and_edges():
    tx, ty, tz = TILE
    L = np.zeros((1, 2 * tx, 2 * ty, 2 * tz), np.uint8)
    L[0, tx - 1, ty - 1, tz - 1] = L[0, tx, ty, tz] = 3                     # across a tile corner
    L[0, tx - 1, ty - 1, 5] = L[0, tx, ty, 5] = 4                           # across the tile edges along Z, Y and X
    L[0, tx - 1, 3, tz - 1] = L[0, tx, 3, tz] = 5
    L[0, 2, ty - 1, tz] = L[0, 2, ty, tz - 1] = 6                           # (the backward neighbour at +1 along Z)
    L[0, tx, 9, 9] = L[0, tx - 1, 9, 9] = 7                                 # across a tile face
    for k in (1, 2, 3):
        ids, sizes, out, table = check_gpu(L, k)
        assert table[0, 2, 0] == (1 if k == 3 else 2) and table[0, 6, 0] == 1
        assert table[0, 3, 0] == table[0, 4, 0] == table[0, 5, 0] == (1 if k >= 2 else 2)
    check_gpu(L[:, :tx + 1, :ty + 1, :tz + 1].copy(), 3)                    # one tile plus one voxel on every side


@pytest.mark.gpu
def test_gpu_ties_absent_classes_and_classes_passed_over():
    L = np.zeros((3, 9, 17, 33), np.uint8)
    L[0, 8, 16, 30:33] = L[0, 0, 0, 0:3] = 1                                # two equal largest, the later one written first
    L[0, 4, 4, 4:6] = 1
    L[1, 7, 2, 10:14] = L[1, 3, 16, 20:24] = L[1, 3, 2, 29:33] = 2          # three equal largest
    L[1, 0, 0, 0] = 2
    L[2, 2:5, 3, 3] = L[2, 2:5, 9, 3] = 5
    L[2, 6, 6, 6:9] = 13                                                    # past the classes
    L[2, 0, 5, 5] = L[2, 8, 5, 5] = 8
    for k in (1, 3):
        ids, sizes, out, table = check_gpu(L, k)
        assert table[0, 0].tolist() == [3, 3, 0, 5] and table[1, 1].tolist() == [4, 4, (3 * 17 + 2) * 33 + 29, 9]
        assert table[2, 4].tolist() == [2, 3, (2 * 17 + 3) * 33 + 3, 3] and table[0, 1].tolist() == [0, 0, -1, 0]
        assert (out[2] == 13).sum() == 3 and table[2, 7].tolist() == [2, 1, 5 * 33 + 5, 1]
        ids, sizes, out, table = check_gpu(L, k, class_mask=1 << 1 | 1 << 5)
        assert table[1, 1].tolist() == [4, 4, (3 * 17 + 2) * 33 + 29, 0] and np.array_equal(out[1], L[1])
        assert table[2, 7].tolist() == [2, 1, 5 * 33 + 5, 0] and table[0, 0, 3] == 5
        check_gpu(L, k, class_mask=0)
    check_gpu(np.minimum(L, 3), 3, n_classes=3, class_mask=6)
    check_gpu(L, 3, n_classes=16, class_mask=(1 << 16) - 2)


@pytest.mark.gpu
def test_gpu_min_size():
    L = np.zeros((1, 9, 17, 33), np.uint8)
    L[0, 1, 1, 1:4] = L[0, 3, 3, 1:5] = L[0, 5, 5, 1:6] = 2                 # sizes min_size - 1, min_size, min_size + 1
    L[0, 7, 7, 0:2] = 9
    for k in (1, 3):
        ids, sizes, out, table = check_gpu(L, k, keep_largest=False, min_size=4)
        assert table[0, 1].tolist() == [3, 5, (5 * 17 + 5) * 33 + 1, 3] and (out == 2).sum() == 9 and table[0, 8, 3] == 2
        check_gpu(L, k, keep_largest=False, min_size=0)
        check_gpu(L, k, keep_largest=False, min_size=1)
        ids, sizes, out, table = check_gpu(L, k, keep_largest=True, min_size=5)
        assert (out == 2).sum() == 5 and table[0, 1, 3] == 7
        ids, sizes, out, table = check_gpu(L, k, keep_largest=True, min_size=6)       # above the largest: the class vanishes
        assert not out.any() and table[0, 1].tolist() == [3, 5, (5 * 17 + 5) * 33 + 1, 12]
    check_gpu(random_labels((1, 19, 21, 70), 0.5, 21), 1, keep_largest=False, min_size=3)


@pytest.mark.gpu
def test_gpu_planes_through_the_python_entry():
    L = random_labels((3, 37, 41), 0.6, 31, hi=4)
    for k in (1, 2):
        ids, sizes, out, table = full_oracle(L[..., None], k, axes=3)
        cc = components.connected_components(torch.from_numpy(L).to(DEV), connectivity=k)
        res = components.keep_largest_component(torch.from_numpy(L).to(DEV), connectivity=k, samples_per_launch=2)
        torch.cuda.synchronize()
        assert np.array_equal(cc.ids.cpu().numpy(), ids[..., 0]) and np.array_equal(cc.sizes.cpu().numpy(), sizes[..., 0])
        assert np.array_equal(cc.count.cpu().numpy(), table[..., 0]) and np.array_equal(res.labels.cpu().numpy(), out[..., 0])
        assert np.array_equal(res.representative.cpu().numpy(), table[..., 2]) and np.array_equal(res.removed.cpu().numpy(), table[..., 3])


@pytest.mark.gpu
def test_gpu_two_runs_give_the_same_bits():
    L = random_labels((2, 19, 21, 70), 0.9, 109)
    first, second = gpu_run(L, 3), gpu_run(L, 3)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert all(np.array_equal(a, b) for a, b in zip(first, full_oracle(L, 3)))


@pytest.mark.gpu
def test_gpu_an_island_ruins_hd95_and_the_clean_up_repairs_it():
    """what the feature is for: a far-away island of false positives barely moves Dice and decides the raw HD95; after the clean-up
    the surface metrics are those of the oracle's cleaned map, and the Dice counts are exact"""
    pred, truth = island_pair()
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    raw = surface.surface_distances(p, t)
    assert raw.hd[0, 2].item() >= 29.0                                     # the island's distance
    kept = components.keep_largest_component(p)
    _, _, out, table = full_oracle(pred, 3)
    assert np.array_equal(kept.labels.cpu().numpy(), out) and table[0, 2].tolist() == [2, int((pred == 3).sum()) - 18, kept.representative[0, 2].item(), 18]
    assert not out[0, :, :, 30:].any() and kept.removed[0, 2].item() == 18
    check_tables(as_numpy(surface.surface_distances(kept.labels, t)), surface_oracle(out, truth), 1)
    assert surface_oracle(out, truth)["hd"][0, 2] <= 1.5
    cnt = segloss.dice_counts(kept.labels.reshape(1, -1).to(torch.uint8), t.reshape(1, -1)).cpu().numpy()
    assert cnt[0, :, 3].tolist() == [int(((out == 3) & (truth == 3)).sum()), int((out == 3).sum()), int((truth == 3).sum())]
    dice_raw, dice_kept = DiceMetricWrapper3D()(p, t)[1][2].item(), DiceMetricWrapper3D()(kept.labels, t)[1][2].item()
    assert 0 < dice_kept - dice_raw < 0.1
    m, batches = _model_and_batches(DEV, surface_metrics=True, largest_component=True)
    _check_lcc_epoch(m, batches, DEV)
