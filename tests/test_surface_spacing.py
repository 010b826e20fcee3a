"""Surface metrics in physical units: ctseg_distmap3d_weighted, ctseg_surface_select_f32, ``surface_distances(spacing=...)``, the
wrappers' ``spacing`` and the BaseUNet3D switch ``surface_spacing``.

The oracle is numpy and independent of the product.  Surfaces come from ``surface_of`` of tests/distance_oracles.py.  With
w = the float32 squares of the float32 voxel sizes, the squared distance of a voxel to a set is the brute-force minimum over the
set's voxels, offsets (dx, dy, dz), of the float32 expression the header pins,

    fl(fl(wy dy^2) + fl(fl(wz dz^2) + fl(wx dx^2)))          (numpy float32 arithmetic: one rounding per operation, no FMA)

which the kernels must match bit for bit.  np.percentile, means and sums are taken on the float64 roots of those float32 values:

  * Hausdorff values within 1e-9 * max(1, value): the interpolation's own rounding is a few ulp of float64
  * means and sums within 1e-11 relative: rows hold at most MAX_ROW = 1e4 surface voxels (asserted), so the order of the additions
    moves a sum by at most n * 2^-53 = 1.1e-12 relative.

A second tier computes the real weighted distances in float64, sqrt(wx dx^2 + wy dy^2 + wz dz^2) with the same table w (the
transform's input) cast to float64.  Three float32 roundings put the squared value within (1 + 2^-24)^3 of it, the root within
(1 + 2^-24)^1.5 < 1 + 2^-23; an order statistic of values each moved by at most that factor moves by no more, a convex
interpolation and a mean of them keep it: every Hausdorff and ASSD value within 2^-23 relative.

CPU tests route the entries through an emulator that is the oracle; GPU tests hold the kernels to it.  The transform's tiles: the
slab pass takes 64 columns of Z (Z = 70: a full tile and one of 6), the line pass 4096 // Z whole lines per workgroup (58 of the 99
lines of a 9 x 11 x 70 volume: workgroups straddle volumes, which have their own weights); the select takes 4096 voxels a step.
"""
import os
import re

import numpy as np
import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import STRUCTURES, surface
from capstone_amd import _native as nat
from capstone_amd.models.metrics import SurfaceDistanceMetricWrapper
from capstone_amd.training.utils import _squash_predictions
from capstone_amd.volumetric.metrics import SurfaceDistanceMetricWrapper3D
from distance_oracles import BRUTE_PAIRS, C, DEV, MAX_ROW, absent_batch, ball_labels, batch_of, d2w_between, d2w_to, nan_reduce, ranks, surface_of
from distance_oracles import surface_oracle as oracle
from feature_emulators import SpacingEntries, SurfaceEntries
from helpers import as_numpy

SPACING = (0.9765625, 1.1, 3.0)
ROWS3 = ((0.9765625, 1.1, 3.0), (3.0, 0.9765625, 1.1), (1.1, 2.5, 0.7))
F32, F64 = np.float32, np.float64


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def squares(spacing):
    """voxel sizes -> their float32 squares, squared in float32"""
    s = np.asarray(spacing, F64).astype(F32)
    return s * s


def table_for(spacing, B):
    w = squares(spacing)
    return np.broadcast_to(w, (B, 3)).copy() if w.ndim == 1 else w


_CACHE = {}


def oracle_w(pred, target, spacing, q=95.0, axes=7, dtype=F32):
    """as ``surface_oracle`` of tests/distance_oracles.py with per-sample voxel sizes; dtype = float64: the second tier"""
    w = table_for(spacing, pred.shape[0])
    key = (pred.tobytes(), target.tobytes(), pred.shape, w.tobytes(), q, axes, np.dtype(dtype).str)
    if key in _CACHE:
        return _CACHE[key]
    B, K = pred.shape[0], C - 1
    counts = np.zeros((2, B, K), np.int64)
    o = {k: np.zeros((2, B, K), dtype) for k in ("d2_lo", "d2_hi", "d2_max")}
    f = {k: np.full((2, B, K), np.nan) for k in ("hd_directed", "hd_max_directed", "asd_directed", "root_sum", "gamma")}
    assd = np.full((B, K), np.nan)
    for b in range(B):
        for k in range(K):
            s = [surface_of(pred[b], k + 1, axes), surface_of(target[b], k + 1, axes)]
            counts[:, b, k] = [s[0].sum(), s[1].sum()]
            if not s[0].any() or not s[1].any():
                continue
            tot = 0.0
            for d in (0, 1):
                d2 = np.sort(d2w_between(s[d], s[1 - d], w[b], dtype))
                lo, hi, g = ranks(len(d2), q)
                roots = np.sqrt(d2.astype(F64))
                o["d2_lo"][d, b, k], o["d2_hi"][d, b, k], o["d2_max"][d, b, k] = d2[lo], d2[hi], d2[-1]
                f["hd_directed"][d, b, k] = np.percentile(roots, q)
                f["hd_max_directed"][d, b, k] = roots[-1]
                f["asd_directed"][d, b, k] = roots.mean()
                f["root_sum"][d, b, k], f["gamma"][d, b, k] = roots.sum(), g
                tot += roots.sum()
            assd[b, k] = tot / (s[0].sum() + s[1].sum())
    res = dict(o, **f, counts=counts, assd=assd, hd=np.maximum(f["hd_directed"][0], f["hd_directed"][1]),
               valid=(counts > 0).all(0)[None].repeat(2, 0))
    _CACHE[key] = res
    return res


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_tables_w(got, ref, B, K=C - 1):
    for k in ("hd_directed", "hd_max_directed", "asd_directed", "gamma", "root_sum", "valid", "counts", "d2_lo", "d2_hi", "d2_max"):
        assert got[k].shape == (2, B, K), k
    assert got["hd"].shape == got["assd"].shape == (B, K)
    assert got["counts"].dtype == np.int64 and got["hd"].dtype == got["assd"].dtype == F64 and got["valid"].dtype == bool
    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["valid"], ref["valid"])
    assert ref["counts"].max() <= MAX_ROW
    for k in ("d2_lo", "d2_hi", "d2_max"):
        assert got[k].dtype == F32 and np.array_equal(bits(got[k]), bits(ref[k])), k
    ok = ref["valid"]
    for k in ("hd_directed", "hd", "hd_max_directed", "asd_directed", "assd"):
        assert np.array_equal(np.isnan(got[k]), ~ok[0] if got[k].ndim == 2 else ~ok), k
    for k in ("hd_directed", "hd_max_directed", "hd"):
        sel = ok if got[k].ndim == 3 else ok[0]
        err = np.abs(got[k][sel] - ref[k][sel]) / np.maximum(1.0, np.abs(ref[k][sel]))
        print(f"{k}: worst error {err.max() if err.size else 0.0:.3e} (bound 1e-9)")
        assert (err <= 1e-9).all(), (k, float(err.max()))
    for k in ("asd_directed", "assd", "root_sum"):
        sel = ok if got[k].ndim == 3 else ok[0]
        err = np.where(ref[k][sel] == 0, np.abs(got[k][sel]), np.abs(got[k][sel] - ref[k][sel]) / np.maximum(np.abs(ref[k][sel]), 1e-300))
        print(f"{k}: worst relative error {err.max() if err.size else 0.0:.3e} (bound 1e-11)")
        assert (err <= 1e-11).all(), (k, float(err.max()))
    # (r - lo with r = (n - 1) * (q / 100) <= 1e4: a fused multiply-subtract skips the product's rounding, half an ulp of r)
    assert (np.abs(got["gamma"][ok] - ref["gamma"][ok]) <= 2.0 ** -40).all()


def check_second_tier(got, true):
    ok = true["valid"]
    for k in ("hd_directed", "hd_max_directed", "asd_directed", "hd", "assd"):
        sel = ok if got[k].ndim == 3 else ok[0]
        err = np.where(true[k][sel] == 0, np.abs(got[k][sel]), np.abs(got[k][sel] - true[k][sel]) / np.maximum(true[k][sel], 1e-300))
        print(f"{k} against float64 distances: worst relative error {err.max() if err.size else 0.0:.3e} (bound 2^-23 = 1.19e-7)")
        assert (err <= 2.0 ** -23).all(), (k, float(err.max()))


class E(SpacingEntries, SurfaceEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E()) as e:
        yield e


def call(pred, target, dev="cpu", **kw):
    res = surface.surface_distances(torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev), **kw)
    if dev != "cpu":
        torch.cuda.synchronize()
    return as_numpy(res)


def same(a, b, keys=None):
    return all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in (keys or a))


# ---- CPU tests ---------------------------------------------------------------------------------------------------------------
def test_the_three_float32_passes_give_the_brute_force_minimum():
    """the kernel's structure restated in numpy float32: fl(w d^2) along X, then the lower envelope along Z, then along Y, each
    candidate one multiplication and one addition; array_equal to the minimum of the nested expression over all voxels of the set"""
    rng = np.random.default_rng(5)
    for shape, w in (((6, 7, 9), squares(SPACING)), ((9, 11, 30), squares(ROWS3[2]))):
        sel = rng.random(shape) < 0.03
        assert sel.any()
        f = np.where(sel, F32(0), F32(np.inf))
        for axis, wa in ((0, w[0]), (2, w[2]), (1, w[1])):
            n = shape[axis]
            t = np.arange(n).reshape([n if a == axis else 1 for a in range(3)])
            best = np.full(shape, np.inf, F32)
            for s in range(n):
                np.minimum(best, wa * ((t - s) ** 2).astype(F32) + np.take(f, [s], axis=axis), out=best)
            f = best
        assert f.dtype == F32 and np.array_equal(bits(f), bits(d2w_to(sel, w)))


@pytest.mark.parametrize("q", [50.0, 95.0])
def test_spacing_through_the_emulator(emu, q):
    pred, target = batch_of((5, 7, 3))
    got = call(pred, target, percentile=q, spacing=SPACING)
    check_tables_w(got, oracle_w(pred, target, SPACING, q), 2)
    check_second_tier(got, oracle_w(pred, target, SPACING, q, dtype=F64))
    assert emu.calls == 3                                                # one launch of each stage for the whole batch
    for sp in (np.array(SPACING), torch.tensor(SPACING), list(SPACING), torch.tensor([SPACING, SPACING], dtype=torch.float64)):
        assert same(call(pred, target, percentile=q, spacing=sp), got)
    assert not np.array_equal(got["hd"], call(pred, target, percentile=q)["hd"], equal_nan=True)


def test_unit_spacing_is_the_voxel_path_and_doubling_it_doubles_the_tables(emu):
    pred, target = batch_of((5, 7, 3))
    plain, one, two = call(pred, target), call(pred, target, spacing=(1, 1, 1)), call(pred, target, spacing=(2.0, 2.0, 2.0))
    assert same(one, plain, ("hd", "hd_directed", "hd_max_directed", "assd", "asd_directed", "root_sum", "gamma", "counts", "valid"))
    for k in ("d2_lo", "d2_hi", "d2_max"):
        assert one[k].dtype == F32 and plain[k].dtype == np.int32 and np.array_equal(one[k], plain[k].astype(F32)), k
        assert np.array_equal(two[k], 4 * one[k]), k
    for k in ("hd", "hd_directed", "hd_max_directed", "assd", "asd_directed", "root_sum"):
        assert np.array_equal(two[k], 2 * plain[k], equal_nan=True), k
    assert same(two, plain, ("counts", "valid", "gamma"))


def test_a_spacing_per_sample_equals_per_sample_calls(emu):
    pred, target = absent_batch()                                        # B = 3
    rows = np.array(ROWS3)
    got = call(pred, target, spacing=rows)
    check_tables_w(got, oracle_w(pred, target, rows), 3)
    assert same(call(pred, target, spacing=rows, samples_per_launch=2), got)
    for b in range(3):
        one = call(pred[b:b + 1], target[b:b + 1], spacing=ROWS3[b])
        for k in got:
            mine, theirs = (one[k][..., 0, :], got[k][..., b, :]) if got[k].ndim == 3 else (one[k][0], got[k][b])
            assert np.array_equal(mine, theirs, equal_nan=True), k
    assert not same(got, call(pred, target, spacing=ROWS3[0]), ("hd",))


def test_planes_take_a_pair(emu):
    pred, target = batch_of((9, 11, 1))
    sp = (0.7, 2.5)
    ref = oracle_w(pred, target, sp + (1.0,), axes=3)
    w = SurfaceDistanceMetricWrapper(spacing=sp)
    mean, _ = w(torch.from_numpy(pred[..., 0]), torch.from_numpy(target[..., 0]))
    check_tables_w(as_numpy(w.last), ref, 2)
    assert abs(mean.item() - nan_reduce(ref["hd"])[0]) <= 1e-9 * max(1.0, mean.item())
    per = np.array([[0.7, 2.5], [1.5, 0.5]])
    w(torch.from_numpy(pred[..., 0]), torch.from_numpy(target[..., 0]), spacing=per)     # the call's spacing wins
    check_tables_w(as_numpy(w.last), oracle_w(pred, target, np.concatenate([per, np.ones((2, 1))], 1), axes=3), 2)
    with pytest.raises(ValueError):
        w(torch.from_numpy(pred[..., 0]), torch.from_numpy(target[..., 0]), spacing=(1.0, 1.0, 1.0))


def test_the_wrapper_keeps_a_spacing_and_a_call_overrides_it(emu):
    pred, target = batch_of((5, 7, 3))
    w = SurfaceDistanceMetricWrapper3D(percentile=50.0, spacing=SPACING)
    w(torch.from_numpy(pred), torch.from_numpy(target))
    assert same(as_numpy(w.last), call(pred, target, percentile=50.0, spacing=SPACING))
    w(torch.from_numpy(pred), torch.from_numpy(target), spacing=ROWS3[1])
    assert same(as_numpy(w.last), call(pred, target, percentile=50.0, spacing=ROWS3[1]))
    plain = SurfaceDistanceMetricWrapper3D()
    assert plain.spacing is None
    plain(torch.from_numpy(pred), torch.from_numpy(target))
    assert plain.last.d2_lo.dtype == torch.int32


def test_bad_spacings_are_refused(emu):
    a = torch.zeros(2, 4, 4, 4, dtype=torch.uint8)
    for sp in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan")), (1.0, float("inf"), 1.0), (1e4, 1.0, 1.0), (1.0, 1.0, 9e-4),
               (1.0, 1.0), (1.0, 1.0, 1.0, 1.0), 1.0, np.ones((3, 3)), np.ones((2, 2)), np.ones((1, 2, 3)), torch.ones(1, 3)):
        with pytest.raises(ValueError):
            surface.surface_distances(a, a, spacing=sp)
    with pytest.raises(ValueError):
        surface.surface_distances(a[..., 0], a[..., 0], spacing=(1.0, 1.0, 1.0))
    assert emu.calls == 0
    surface.surface_distances(a, a, spacing=(1e-3, 1e3, 1.0))           # the ends of the range are in it
    assert emu.calls == 3


def test_the_library_validates_the_new_entries_before_any_launch():
    """ctseg_distmap3d_weighted and ctseg_surface_select_f32 themselves; no device is touched: every case fails validation"""
    L = nat.lib()
    err = L.ctseg_last_error

    def weighted(masks=4096, P=2, X=8, Y=8, Z=8, w=8192, ws=1 << 21, ws_bytes=None, fg=1 << 22, bg=None):
        return L.ctseg_distmap3d_weighted(masks, P, X, Y, Z, w, ws, 6 * P * X * Y * Z if ws_bytes is None else ws_bytes, fg, bg, None)

    def select(e=4096, d2=8192, counts=1 << 20, B=2, X=8, Y=8, Z=8, n=10, q=95.0, ws=1 << 21, ws_bytes=None, stats=1 << 22, fs=1 << 23):
        need = 2 * B * (n - 1) * surface.SELECT_F32_ROW_BYTES
        return L.ctseg_surface_select_f32(e, d2, counts, B, X, Y, Z, n, q, ws, need if ws_bytes is None else ws_bytes, stats, fs, None)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctseg_hip.h")).read()
    assert int(re.search(r"#define CTSEG_SURFACE_SELECT_F32_ROW_BYTES (\d+)", hdr).group(1)) == surface.SELECT_F32_ROW_BYTES
    assert surface.BYTES_PER_VOXEL_WEIGHTED == 11 and surface.BYTES_PER_VOXEL == 15
    for call_, ptrs in ((weighted, ("masks", "w", "ws", "fg")), (select, ("e", "d2", "counts", "ws", "stats", "fs"))):
        for p in ptrs:
            assert call_(**{p: None}) < 0 and b"null pointer" in err(), p
        for kw in (dict(X=0), dict(Y=0), dict(Z=0), dict(Z=-3)):
            assert call_(**kw) < 0 and b">= 1" in err()
        for kw in (dict(X=1025), dict(Y=1025), dict(Z=1025)):
            assert call_(**kw) < 0 and b"sides up to 1024" in err()
    # d2_bg alone passes the null-pointer check; the short workspace is what refuses the call
    assert weighted(fg=None, bg=1 << 22, ws_bytes=6 * 2 * 512 - 1) < 0 and b"workspace" in err()
    for kw in (dict(P=0), dict(P=-2)):
        assert weighted(**kw) < 0 and b">= 1" in err()
    assert weighted(ws_bytes=6 * 2 * 512 - 1) < 0 and b"workspace" in err()
    for kw in (dict(ws=(1 << 21) + 2), dict(w=8194), dict(fg=(1 << 22) + 2), dict(bg=(1 << 23) + 1)):
        assert weighted(**kw) < 0 and b"unaligned" in err()
    for kw in (dict(B=0), dict(B=-1)):
        assert select(**kw) < 0 and b">= 1" in err()
    for n in (1, 0, 17, -4):
        assert select(n=n) < 0 and b"classes" in err()
    assert select(B=4000) < 0 and b"too many" in err()
    for q in (-0.5, 100.5, float("nan")):
        assert select(q=q) < 0 and b"percentile" in err()
    assert select(ws_bytes=2 * 2 * 9 * surface.SELECT_F32_ROW_BYTES - 1) < 0 and b"workspace" in err()
    for kw in (dict(ws=(1 << 21) + 4), dict(fs=(1 << 23) + 4), dict(stats=(1 << 22) + 2), dict(counts=(1 << 20) + 1), dict(d2=8194),
               dict(e=4100, Z=16)):
        assert select(**kw) < 0 and b"unaligned" in err()


MM = (1.0, 1.0, 2.5)


def _model_and_batches(spacing, dev="cpu"):
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(7)
    m = BaseUNet3D(filters=[4, 8, 8], loss_fx=["CrossEntropy"], surface_metrics=True, surface_spacing=spacing).to(dev)
    g = torch.Generator().manual_seed(3)
    batches = []
    for s in (0, 1):
        L = ball_labels((16, 16, 8), 40 + s)
        masks = torch.from_numpy(np.stack([(L == c) for c in range(1, C)]).astype(np.uint8))[None]
        batches.append((torch.randn(1, 1, 16, 16, 8, generator=g).to(dev), masks.to(dev), torch.ones(1, 9).to(dev)))
    return m, batches


def _check_mm_epoch(m, batches):
    """the validation steps log the mm keys; their values are those of a direct call on the predictions the model made"""
    assert m.surface_spacing == MM and "surface_spacing" not in m.hparams and "surface_metrics" not in m.hparams
    hd, assd, preds = [], [], []
    with torch.no_grad():
        for b in batches:
            assert m.validation_step(b) is None
        for images, masks, _ in batches:
            pred = _squash_predictions(m(images))
            truth = (masks[0].cpu().numpy() * np.arange(1, C).reshape(-1, 1, 1, 1)).max(0)[None].astype(np.uint8)
            res = surface.surface_distances(pred, torch.from_numpy(truth).to(pred.device), spacing=MM)
            hd.append(res.hd)
            assd.append(res.assd)
            preds.append((pred.cpu().numpy().astype(np.uint8), truth))
    direct = surface.reduce_nan_mean(torch.cat(hd)) + surface.reduce_nan_mean(torch.cat(assd))
    ref_hd = np.concatenate([oracle_w(p, t, MM)["hd"] for p, t in preds])
    m.on_validation_epoch_end()
    finite = torch.isfinite(direct[1]).tolist()
    assert any(finite) and finite == (~np.isnan(nan_reduce(ref_hd)[1])).tolist()
    for i, s in enumerate(STRUCTURES):
        assert (f"{s} HD95 mm (val)" in m.logged) == (f"{s} ASSD mm (val)" in m.logged) == finite[i]
        if finite[i]:
            assert m.logged[f"{s} HD95 mm (val)"].item() == direct[1][i].item()
            assert m.logged[f"{s} ASSD mm (val)"].item() == direct[3][i].item()
    assert m.logged["Mean HD95 mm (val)"].item() == direct[0].item() and m.logged["Mean ASSD mm (val)"].item() == direct[2].item()
    assert abs(direct[0].item() - nan_reduce(ref_hd)[0]) <= 1e-9 * max(1.0, direct[0].item())
    assert not any(k.endswith("HD95 (val)") or k.endswith("ASSD (val)") for k in m.logged)


def test_the_trainer_logs_mm_keys_with_a_spacing_and_the_old_keys_without(emu):
    m, batches = _model_and_batches(MM)
    _check_mm_epoch(m, batches)
    assert emu.calls == 12                                               # two validation steps and two direct calls, three stages each
    old, batches = _model_and_batches(None)
    with torch.no_grad():
        for b in batches:
            old.validation_step(b)
    old.on_validation_epoch_end()
    assert old.surface_spacing is None and "Mean HD95 (val)" in old.logged and "Mean ASSD (val)" in old.logged
    assert not any(" mm " in k for k in old.logged)


# ---- GPU tests: the kernels against the oracle -------------------------------------------------------------------------------
def gpu_weighted(masks, w):
    """(P, X, Y, Z) uint8 masks, (P, 3) float32 -> (d2_fg, d2_bg) of ctseg_distmap3d_weighted: both at once, then each alone"""
    P, X, Y, Z = masks.shape
    m, wt = torch.from_numpy(masks).to(DEV), torch.from_numpy(np.ascontiguousarray(w, F32)).to(DEV)
    ws = torch.empty((6 * masks.size,), dtype=torch.uint8, device=DEV)
    out = [torch.full((2,) + masks.shape, 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]      # every value is to be written
    for (fg, bg) in ((out[0][0], out[0][1]), (out[1][0], None), (None, out[2][1])):
        nat.call("ctseg_distmap3d_weighted", nat.ptr(m), P, X, Y, Z, nat.ptr(wt), nat.ptr(ws), 6 * masks.size, nat.ptr(fg), nat.ptr(bg))
    torch.cuda.synchronize()
    both, fg, bg = (o.cpu().numpy() for o in out)
    assert np.array_equal(bits(both[0]), bits(fg[0])) and np.array_equal(bits(both[1]), bits(bg[1]))
    assert (fg[1] == 7.0).all() and (bg[0] == 7.0).all()                # an absent output is not written
    return both[0], both[1]


def check_transform(masks, w):
    sel = masks != 0
    pairs = 2 * sum(int(s.sum()) * int((~s).sum()) for s in sel)
    assert pairs <= BRUTE_PAIRS, pairs
    fg, bg = gpu_weighted(masks, w)
    for p, s in enumerate(sel):
        for name, got, ref in (("d2_fg", fg[p], d2w_to(s, w[p])), ("d2_bg", bg[p], d2w_to(~s, w[p]))):
            bad = bits(got) != bits(ref)
            assert not bad.any(), (name, p, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), ref[bad][:4].tolist())


def tables(P):
    return {"one spacing": np.broadcast_to(squares(SPACING), (P, 3)).copy(), "a row per volume": squares([ROWS3[p % 3] for p in range(P)])}


def random_masks(shape, seed, density=0.01):
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) < density).astype(np.uint8)
    assert all(v.any() for v in m)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["one spacing", "a row per volume"])
def test_gpu_weighted_transform_bit_for_bit(table):
    for shape, seed in (((3, 9, 11, 70), 11), ((2, 16, 16, 32), 12)):
        masks = random_masks(shape, seed)
        check_transform(masks, tables(shape[0])[table])
    corner = np.zeros((1, 40, 3, 130), np.uint8)                         # the search walks whole lines; unequal weights at the exit
    corner[0, 39, 0, 129] = 1
    check_transform(corner, tables(1)[table])
    for shape, at in (((2, 5, 1, 1), ([0, 1, 1], [3, 0, 4])), ((1, 1, 7, 1), ([0, 0], [2, 3]))):     # sides of 1
        ones = np.zeros(shape, np.uint8)
        ones[at[0], at[1] if shape[1] > 1 else 0, at[1] if shape[2] > 1 else 0] = 1
        check_transform(ones, tables(shape[0])[table])
    flat = np.zeros((2, 4, 5, 6), np.uint8)                              # nothing to find: -1 everywhere in the other class's output
    flat[1] = 1
    fg, bg = gpu_weighted(flat, tables(2)[table])
    assert (fg[0] == -1).all() and (bg[0] == 0).all() and (fg[1] == 0).all() and (bg[1] == -1).all()
    check_transform(flat, tables(2)[table])


def test_the_anisotropic_nearest_voxel_is_another_voxel():
    """a condition on the first GPU shape's input: for at least 10 % of the voxels the weighted nearest set voxel is not a nearest
    one in voxel units, so no rescaling of the integer transform passes the test above"""
    sel = random_masks((3, 9, 11, 70), 11)[0] != 0
    a, b = np.argwhere(~sel).astype(np.int64), np.argwhere(sel).astype(np.int64)
    d = (a[:, None, :] - b[None, :, :]) ** 2
    plain = d.sum(-1)
    w = squares(SPACING).astype(F64)
    nearest = (d * w).sum(-1).argmin(1)
    differs = plain[np.arange(len(a)), nearest] > plain.min(1)
    print(f"the weighted nearest voxel is not a voxel-unit nearest one for {differs.mean():.1%} of the voxels")
    assert differs.mean() >= 0.10


SELECT_SHAPES = {"two chunks": (3, 7, 211), "16-byte runs": (4, 8, 160)}


def select_rows():
    """name -> float32 values of a row"""
    rng = np.random.default_rng(21)
    base = np.array([1.5], F32).view(np.uint32)[0]
    low9 = (base + rng.choice(512, 300, replace=False).astype(np.uint32)).view(F32)
    mid = (base + (rng.integers(0, 1 << 20, 500).astype(np.uint32))).view(F32)
    span = np.geomspace(1e-6, 1e6, 1000).astype(F32)
    rows = {"the lowest 9 bits": low9, "one top bucket": mid, "equal": np.full(7, 2.25, F32), "one value": np.array([3.75], F32),
            "1e-6 to 1e6": span, "zeros and tiny": np.array([0.0, 0.0, 1e-38, 1e-30, 5.0], F32),
            "random": (rng.random(2000) * 4000).astype(F32)}
    assert len({int(v) >> 9 for v in low9.view(np.uint32)}) == 1 and len({int(v) >> 20 for v in mid.view(np.uint32)}) == 1
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SELECT_SHAPES), ids=list(SELECT_SHAPES))
@pytest.mark.parametrize("q", [0.0, 50.0, 95.0, 100.0])
def test_gpu_select_on_constructed_float_rows(q, shape):
    X, Y, Z = SELECT_SHAPES[shape]
    S, rows = X * Y * Z, select_rows()
    K = len(rows) + 1                                                    # and one row without values
    rng = np.random.default_rng(22)
    edges = np.zeros((2, 1, K, S), np.uint8)
    d2 = np.full((2, 1, K, S), -1.0, F32)                               # row (0, k) reads d2[1, k] where edges[0, k] is set
    d2[1, :, :, ::3] = 7.0                                               # values off the mask are not values of the row
    counts = np.zeros((2, 1, K), np.int32)
    for k, v in enumerate(rows.values()):
        at = rng.choice(S, len(v), replace=False)
        edges[0, 0, k, at], d2[1, 0, k, at] = 1, rng.permutation(v)
        edges[1, 0, k, 5], d2[0, 0, k, 5] = 1, 0.5                       # the partner: one voxel
        counts[:, 0, k] = [len(v), 1]
    edges[0, 0, K - 1, :9], counts[0, 0, K - 1] = 1, 9                   # its partner has no voxel
    dev = [torch.from_numpy(a).to(DEV) for a in (edges, d2, counts)]
    n_rows = 2 * K
    ws = torch.empty((n_rows * surface.SELECT_F32_ROW_BYTES // 8,), dtype=torch.float64, device=DEV)
    st = torch.full((n_rows, 4), 9, dtype=torch.int32, device=DEV)
    fs = torch.full((n_rows, 2), 9.0, dtype=torch.float64, device=DEV)
    res = []
    for _ in range(2):
        nat.call("ctseg_surface_select_f32", nat.ptr(dev[0]), nat.ptr(dev[1]), nat.ptr(dev[2]), 1, X, Y, Z, K + 1, q, nat.ptr(ws),
                 n_rows * surface.SELECT_F32_ROW_BYTES, nat.ptr(st), nat.ptr(fs))
        torch.cuda.synchronize()
        res.append((st.cpu().numpy(), fs.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1].view(np.uint64), res[1][1].view(np.uint64))
    st, fs = res[0]
    for k, (name, v) in enumerate(rows.items()):
        v = np.sort(v)
        lo, hi, g = ranks(len(v), q)
        want = np.array([v[lo], v[hi], v[-1]], F32).view(np.int32).tolist() + [1]
        assert st[k].tolist() == want, (name, st[k].view(F32)[:3].tolist(), [v[lo], v[hi], v[-1]])
        total = np.sqrt(v.astype(F64)).sum()
        assert abs(fs[k, 0] - total) <= 1e-11 * total and abs(fs[k, 1] - g) <= 2.0 ** -40, name
        assert st[K + k].tolist() == np.array([0.5, 0.5, 0.5], F32).view(np.int32).tolist() + [1] and fs[K + k, 0] == np.sqrt(0.5)
    assert not st[K - 1].any() and not st[2 * K - 1].any() and not fs[K - 1].any() and not fs[2 * K - 1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(20, 17, 33), (16, 16, 32)], ids=["20x17x33", "16x16x32"])
def test_gpu_surface_distances_with_a_spacing(shape):
    pred, target = batch_of(shape)
    for sp in (SPACING, np.array(ROWS3[1:])):
        got = call(pred, target, DEV, spacing=sp)
        check_tables_w(got, oracle_w(pred, target, sp), 2)
        check_second_tier(got, oracle_w(pred, target, sp, dtype=F64))
        assert same(call(pred, target, DEV, spacing=sp), got)            # integer atomics and fixed-order sums: the same bits
        assert same(call(pred, target, DEV, spacing=sp, samples_per_launch=1), got)
    for q in (0.0, 100.0):
        got = call(pred, target, DEV, spacing=SPACING, percentile=q)
        check_tables_w(got, oracle_w(pred, target, SPACING, q), 2)
    assert np.array_equal(got["hd_directed"], got["hd_max_directed"], equal_nan=True)


@pytest.mark.gpu
def test_gpu_unit_spacing_equals_the_unweighted_device_path():
    pred, target = batch_of((16, 16, 32))
    plain, one, two = call(pred, target, DEV), call(pred, target, DEV, spacing=(1, 1, 1)), call(pred, target, DEV, spacing=(2, 2, 2))
    assert same(one, plain, ("hd", "hd_directed", "hd_max_directed", "assd", "asd_directed", "root_sum", "gamma", "counts", "valid"))
    for k in ("d2_lo", "d2_hi", "d2_max"):
        assert one[k].dtype == F32 and np.array_equal(one[k], plain[k].astype(F32)) and np.array_equal(two[k], 4 * one[k]), k
    assert np.array_equal(two["hd"], 2 * plain["hd"], equal_nan=True) and np.array_equal(two["assd"], 2 * plain["assd"], equal_nan=True)
    assert np.array_equal(plain["counts"], oracle(pred, target)["counts"])


@pytest.mark.gpu
def test_gpu_absent_classes_stay_nan_with_a_spacing():
    pred, target = absent_batch()
    rows = np.array(ROWS3)
    got = call(pred, target, DEV, spacing=rows)                          # B = 3 in one launch, a spacing per sample
    check_tables_w(got, oracle_w(pred, target, rows), 3)
    assert np.isnan(got["hd"][:, 3]).all() and np.isnan(got["assd"][:, 3]).all() and not got["valid"][:, :, 3].any()
    w = SurfaceDistanceMetricWrapper3D(spacing=rows)
    mean, pc = w(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV))
    rm, rpc = nan_reduce(oracle_w(pred, target, rows)["hd"])
    assert np.isnan(pc[3].item()) and np.allclose(pc.cpu().numpy(), rpc, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert abs(mean.item() - rm) <= 1e-9 * max(1.0, rm)
    planes = batch_of((19, 33, 1))
    got = call(planes[0][..., 0], planes[1][..., 0], DEV, spacing=(0.7, 2.5))
    check_tables_w(got, oracle_w(planes[0], planes[1], (0.7, 2.5, 1.0), axes=3), 2)


@pytest.mark.gpu
def test_gpu_validation_steps_log_millimetres():
    m, batches = _model_and_batches(MM, DEV)
    _check_mm_epoch(m, batches)
