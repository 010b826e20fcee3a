"""Test-time augmentation and native-grid prediction of the 3-D U-Net: ctseg_tta_accumulate / ctseg_tta_finish,
capstone_amd.volumetric.tta (tta_accumulate, tta_finish, view_to_target_matrix, class_channel_src, mirror_views,
TestTimeAugmenter3D) and BaseUNet3D(tta=...).

Held to ``oracle_accumulate`` / ``oracle_finish`` / ``oracle_run`` of tests/resample_oracles.py.  Every mode-0 comparison is
``array_equal``; mode 1 goes through expf, whose last bit numpy does not share, and is held per element to ``helpers.check_elems``.

CPU tests route the two entries through an emulator that IS the oracle; GPU tests hold the kernels to the oracle.  Every check is
one function of the device, run by a CPU test (emulated) and by a GPU test.

The kernel's tile is one target h and 16 x 16 of (w, d), not the augment kernel's 64 x 32: view grid (D', H', W') = (33, 6, 70)
used as its own target is full tiles plus a ragged remainder on both tiled axes (33 = 2 * 16 + 1, 70 = 4 * 16 + 6), and so are
the native targets (13, 40, 37) and (70, 12, 130); (32, 4, 64) is exact tiles; (9, 33, 33) has the square h-w plane a quarter
turn needs.  Every grid has fewer than 2e5 voxels.
"""
import ctypes

import numpy as np
import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import STRUCTURES
from capstone_amd import _native as nat
from capstone_amd.training.utils import _squash_predictions
from capstone_amd.volumetric import transforms as T
from capstone_amd.volumetric import tta
from feature_emulators import Augment3dEntries, Distmap3dEntries, Tta3dEntries
from helpers import F32, check_elems, elem_bound
from resample_oracles import GENERAL, SWAPPED, flip_matrix, identity, oracle_finish, oracle_run, quarter_turn

DEV = "cuda:0"
VIEW_GRIDS = [(33, 6, 70), (9, 33, 33), (32, 4, 64)]                 # (D', H', W'): ragged, square, exact
NATIVE = [(13, 40, 37), (70, 12, 130)]                               # raw (D, H, W) targets, layout 1
CONFIGS = [(10, 12, 12), (3, 4, 4), (11, 12, 12), (12, 12, 16)]      # (C, ld, acc_ld); (11, 12, 12): the weight column is the last
CLASS_SWAPPED = [0] + [1 + s for s in SWAPPED]
GUARD = 3                                                            # rows of sentinel before and after the accumulator
SENTINEL = -12345.0


def _cases():
    """(view grid, target, layout, (C, ld, acc_ld)): every grid onto itself and onto both native shapes, the configurations
    rotating so that each of them meets both layouts"""
    out = []
    for i, vg in enumerate(VIEW_GRIDS):
        for j, (target, layout) in enumerate([(vg, 0)] + [(n, 1) for n in NATIVE]):
            out.append((vg, target, layout, CONFIGS[(i + j) % 4]))
    out.append((VIEW_GRIDS[0], VIEW_GRIDS[0], 0, CONFIGS[3]))
    assert {(c[2], c[3]) for c in out} == {(lay, cfg) for lay in (0, 1) for cfg in CONFIGS}
    return out


CASES = _cases()
CASE_IDS = [f"{c[0]}->{c[1]} C{c[3][0]}/{c[3][1]}/{c[3][2]}" for c in CASES]


class E(Tta3dEntries, Augment3dEntries, Distmap3dEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E()) as e:
        yield e


@pytest.fixture()
def calls(emu):
    """the names of the entries called directly, in order (a spy on nat.call, on top of the emulator)"""
    seen, inner = [], nat.call

    def spy(name, *args):
        seen.append(name)
        return inner(name, *args)
    nat.call = spy
    yield seen
    nat.call = inner


# ---- inputs and the product's side, computed once ----------------------------------------------------------------------------
_BLOCKS = {}


def block(vg, ld, kind="normal"):
    """one view's storage (H, W, D, ld) float32: 4 x standard normal, or small whole numbers with many ties"""
    key = (vg, ld, kind)
    if key not in _BLOCKS:
        rng = np.random.default_rng(sum(vg) * 13 + ld + len(kind))
        shape = (vg[1], vg[2], vg[0], ld)
        a = (4.0 * rng.standard_normal(shape)).astype(np.float32) if kind == "normal" else rng.integers(-2, 3, shape).astype(np.float32)
        a.setflags(write=False)
        _BLOCKS[key] = a
    return _BLOCKS[key]


def as_logits(blk, C, dev):
    """(H, W, D, ld) storage -> the (1, C, H, W, D) tensor a network returns: on the device its channels-last storage is read in
    place, the pad columns beyond C holding NaN, which must never reach a result"""
    a = np.array(blk)
    a[..., C:] = np.nan
    t = torch.from_numpy(a).to(dev)
    return t[..., :C].permute(3, 0, 1, 2).unsqueeze(0)


def product_run(dev, views, C, acc_ld, target, layout, mode, interp):
    """the views through tta_accumulate into a guarded accumulator -> (acc tensor (St, acc_ld), the whole guarded buffer)"""
    St = int(np.prod(target))
    whole = torch.full((St + 2 * GUARD, acc_ld), SENTINEL, dtype=torch.float32, device=dev)
    acc = whole[GUARD:GUARD + St]
    acc.zero_()
    for blk, M, src, weight in views:
        tta.tta_accumulate(acc, as_logits(blk, C, dev), M, src, weight, "probabilities" if mode else "logits",
                           "trilinear" if interp else "nearest", target, "dhw" if layout else "hwd")
    return acc, whole


def assert_guards(whole, acc, C):
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), "guard rows were written"
    assert bool((acc[:, C + 1:] == 0).all()), "pad columns beyond the weight column were written"
    assert bool(torch.isfinite(acc).all())


def general_matrix(vg, target, layout):
    return tta.view_to_target_matrix(vg, GENERAL, target if layout else None)


def mirror_matrix(vg, target, layout):
    return tta.view_to_target_matrix(vg, dict(T.Augment3D.identity_params(), flips=(False, False, True)), target if layout else None)


# ---- 1. one view, mode 0, weight 1 -------------------------------------------------------------------------------------------
def check_one_view_bit_for_bit(dev, case, interp):
    vg, target, layout, (C, ld, acc_ld) = case
    blk, M = block(vg, ld), general_matrix(vg, target, layout)
    want = oracle_run([(blk, M, None, 1.0)], C, target, layout, 0, interp)
    covered = float((want[:, C] != 0).mean())
    assert 0.1 < covered < 1.0, covered                                 # the view covers a part of the target and leaves a part
    acc, whole = product_run(dev, [(blk, M, None, 1.0)], C, acc_ld, target, layout, 0, interp)
    assert_guards(whole, acc, C)
    assert np.array_equal(acc[:, :C + 1].cpu().numpy(), want)
    labels, probs, hist = tta.tta_finish(acc, C, "logits")
    lab, _, hs, _ = oracle_finish(want, C, 0)
    assert probs is None and labels.dtype == torch.uint8 and np.array_equal(labels.cpu().numpy(), lab)
    assert np.array_equal(hist.cpu().numpy(), hs) and np.array_equal(hs, np.bincount(lab, minlength=C))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("interp", [0, 1])
def test_one_view_bit_for_bit(emu, case, interp):
    check_one_view_bit_for_bit("cpu", case, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("interp", [0, 1])
def test_gpu_one_view_bit_for_bit(case, interp):
    check_one_view_bit_for_bit(DEV, case, interp)


# ---- 2. identity and integer matrices ----------------------------------------------------------------------------------------
def check_integer_matrices(dev, vg, cfg):
    C, ld, acc_ld = cfg
    blk = block(vg, ld)
    base = torch.from_numpy(np.array(blk[..., :C]))                      # (H, W, D, C): the d, h, w axes are 2, 0, 1
    axis = (2, 0, 1)
    cases = [(identity(), None, base)]
    cases += [(flip_matrix(a, vg), None, torch.flip(base, [axis[a]])) for a in range(3)]
    if vg[1] == vg[2]:
        cases.append((quarter_turn(vg), None, torch.rot90(base, 1, (0, 1))))
    if C == 10:
        cases.append((flip_matrix(2, vg), CLASS_SWAPPED, torch.flip(base, [1])[..., CLASS_SWAPPED]))
    for M, src, want in cases:
        for interp in (0, 1):
            acc, whole = product_run(dev, [(blk, M, src, 1.0)], C, acc_ld, vg, 0, 0, interp)
            assert_guards(whole, acc, C)
            assert torch.equal(acc[:, :C].cpu().view(want.shape), want) and bool((acc[:, C] == 1).all())


@pytest.mark.parametrize("vg,cfg", list(zip(VIEW_GRIDS, CONFIGS)) + [(VIEW_GRIDS[1], CONFIGS[3])])
def test_integer_matrices_are_flip_and_rot90(emu, vg, cfg):
    check_integer_matrices("cpu", vg, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("vg,cfg", list(zip(VIEW_GRIDS, CONFIGS)) + [(VIEW_GRIDS[1], CONFIGS[3])])
def test_gpu_integer_matrices_are_flip_and_rot90(vg, cfg):
    check_integer_matrices(DEV, vg, cfg)


# ---- 3. the mirror group -----------------------------------------------------------------------------------------------------
def check_mirror_group(dev, vg):
    C, ld, acc_ld = CONFIGS[0]
    base = block(vg, ld, "integers")[..., :C]                            # whole numbers in -2..2: ties at most voxels
    views = []
    params = tta.mirror_views(("h", "w"))
    assert [p["flips"] for p in params] == [(False, False, False), (False, False, True), (False, True, False), (False, True, True)]
    for p in params:
        # what the network shows for the mirrored scan: the mirrored block, its paired structures swapped under the w mirror
        v = base
        if p["flips"][1]:
            v = np.flip(v, 0)
        if p["flips"][2]:
            v = np.flip(v, 1)[..., CLASS_SWAPPED]
        padded = np.zeros(v.shape[:3] + (ld,), np.float32)
        padded[..., :C] = v
        views.append((padded, tta.view_to_target_matrix(vg, p), tta.class_channel_src(p), 1.0))
    assert (np.sort(base, axis=-1)[..., -1] == np.sort(base, axis=-1)[..., -2]).mean() > 0.3
    for interp in (0, 1):
        acc, whole = product_run(dev, views, C, acc_ld, vg, 0, 0, interp)
        assert_guards(whole, acc, C)
        got = acc.cpu().numpy()
        assert np.array_equal(got[:, :C], 4 * base.reshape(-1, C)) and np.array_equal(got[:, C], np.full(len(got), 4, np.float32))
        labels = tta.tta_finish(acc, C, "logits")[0]
        assert np.array_equal(labels.cpu().numpy(), np.argmax(base.reshape(-1, C), axis=1))
    # a plain flip ensemble, without the class map, averages the pairs into each other: this check would see it
    wrong = [(v[0], v[1], None, 1.0) for v in views]
    assert not np.array_equal(oracle_run(wrong, C, vg, 0, 0, 0)[:, :C], 4 * base.reshape(-1, C))


@pytest.mark.parametrize("vg", VIEW_GRIDS)
def test_mirror_group_sums_to_four_times_the_base(emu, vg):
    check_mirror_group("cpu", vg)


@pytest.mark.gpu
@pytest.mark.parametrize("vg", VIEW_GRIDS)
def test_gpu_mirror_group_sums_to_four_times_the_base(vg):
    check_mirror_group(DEV, vg)


# ---- 4. coverage -------------------------------------------------------------------------------------------------------------
def check_coverage(dev, vg, layout):
    C, ld, acc_ld = CONFIGS[2]
    target = vg
    w1, w2 = 1.0, 0.5
    A, B = identity(), identity()
    A[0, 3], B[2, 3] = 3.3, -4.6            # view A runs off the far end of d, view B off the near end of w
    views = [(block(vg, ld), A, None, w1), (block(vg, ld, "integers"), B, None, w2)]
    want = oracle_run(views, C, target, layout, 0, 1)
    d, h, w = np.meshgrid(*(np.arange(n) for n in target), indexing="ij")
    in_a, in_b = d <= target[0] - 1 - 3, w >= 5        # floor(d + 3.3 + .5) <= D - 1;  floor(w - 4.6 + .5) >= 0
    by_hand = (w1 * in_a + w2 * in_b).astype(np.float32)
    by_hand = (np.transpose(by_hand, (1, 2, 0)) if layout == 0 else by_hand).reshape(-1)
    assert np.array_equal(want[:, C], by_hand) and set(np.unique(by_hand)) == {0.0, w1, w2, w1 + w2}
    acc, whole = product_run(dev, views, C, acc_ld, target, layout, 0, 1)
    assert_guards(whole, acc, C)
    assert np.array_equal(acc[:, :C + 1].cpu().numpy(), want)
    labels, probs, hist = tta.tta_finish(acc, C, "logits", want_probs=True)
    lab, pr, hs, uncovered = oracle_finish(want, C, 0)
    none = by_hand == 0
    assert uncovered == int(none.sum()) > 0 and int((acc[:, C] == 0).sum()) == uncovered
    labels, probs = labels.cpu().numpy(), probs.cpu().numpy()
    assert np.array_equal(labels, lab) and not labels[none].any() and not probs[none].any() and np.array_equal(hist.cpu().numpy(), hs)
    assert np.abs(probs[~none].sum(1) - 1).max() < 1e-5


@pytest.mark.parametrize("vg,layout", [(VIEW_GRIDS[0], 0), (VIEW_GRIDS[1], 1), (VIEW_GRIDS[2], 1)])
def test_coverage_of_two_shifted_views(emu, vg, layout):
    check_coverage("cpu", vg, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("vg,layout", [(VIEW_GRIDS[0], 0), (VIEW_GRIDS[1], 1), (VIEW_GRIDS[2], 1)])
def test_gpu_coverage_of_two_shifted_views(vg, layout):
    check_coverage(DEV, vg, layout)


# ---- 5. and 6. per-element bounds against float64 ----------------------------------------------------------------------------
_REFS = {}


def two_view_refs(case, mode):
    """the general view with weight 1 and the w mirror with weight 0.5 and the class map (C = 10) -> for float64 and float32:
    acc, labels, probs"""
    key = (CASES.index(case), mode)
    if key not in _REFS:
        vg, target, layout, (C, ld, acc_ld) = case
        views = [(block(vg, ld), general_matrix(vg, target, layout), None, 1.0),
                 (block(vg, ld), mirror_matrix(vg, target, layout), CLASS_SWAPPED if C == 10 else None, 0.5)]
        out = {"views": views}
        for dt in (np.float64, np.float32):
            acc = oracle_run(views, C, target, layout, mode, 1, dt)
            out[dt] = (acc,) + oracle_finish(acc, C, mode)[:2]
        _REFS[key] = out
    return _REFS[key]


def decided(ref, C, mode, what):
    """voxels whose float64 top-two margin, in the accumulator the labels are read from, exceeds twice its per-element bound, and
    the voxels no view covers (label 0 by the float32 coverage rule, which both oracles share); at most 1 % may be left out"""
    a64 = torch.from_numpy(ref[np.float64][0])
    bound, _ = elem_bound(a64[:, :C], torch.from_numpy(ref[np.float32][0][:, :C]), F32)
    top = torch.sort(a64[:, :C], dim=1, descending=True).values
    keep = ((top[:, 0] - top[:, 1]) > 2 * bound.max(dim=1).values) | (a64[:, C] == 0)
    left_out = 1.0 - float(keep.double().mean())
    print(f"{what}: {left_out:.3%} of the voxels are within twice the bound of a tie")
    assert left_out <= 0.01, (what, left_out)
    return keep.numpy()


def check_against_float64(dev, case, mode):
    vg, target, layout, (C, ld, acc_ld) = case
    ref = two_view_refs(case, mode)
    tag = f"mode {mode} {vg}->{target}"
    acc, whole = product_run(dev, ref["views"], C, acc_ld, target, layout, mode, 1)
    assert_guards(whole, acc, C)
    got = acc[:, :C + 1].cpu()
    if mode == 0:
        assert np.array_equal(got.numpy(), ref[np.float32][0])
    else:
        assert np.array_equal(got[:, C].numpy(), ref[np.float32][0][:, C])             # the weight sums are exact either way
        check_elems(tag + " acc", got[:, :C], torch.from_numpy(ref[np.float64][0][:, :C]), torch.from_numpy(ref[np.float32][0][:, :C]), F32)
    labels, probs, hist = tta.tta_finish(acc, C, "probabilities" if mode else "logits", want_probs=True)
    check_elems(tag + " probs", probs.cpu(), torch.from_numpy(ref[np.float64][2]), torch.from_numpy(ref[np.float32][2]), F32)
    labels = labels.cpu().numpy()
    keep = decided(ref, C, mode, tag)
    assert np.array_equal(labels[keep], ref[np.float64][1][keep])
    if mode == 0:
        assert np.array_equal(labels, ref[np.float32][1])
    assert np.array_equal(hist.cpu().numpy(), np.bincount(labels, minlength=C))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode", [0, 1])
def test_oracle_alone_decides_all_but_one_percent(case, mode):
    """the condition of the label comparison, on the oracle alone: with logits = 4 x standard normal at most 1 % of the voxels lie
    within twice the per-element bound of a tie, and the float32 oracle agrees with the float64 one on all others"""
    ref = two_view_refs(case, mode)
    keep = decided(ref, case[3][0], mode, f"mode {mode} {case[0]}->{case[1]}")
    assert np.array_equal(ref[np.float32][1][keep], ref[np.float64][1][keep])


@pytest.mark.parametrize("case", CASES[:4], ids=CASE_IDS[:4])
@pytest.mark.parametrize("mode", [0, 1])
def test_two_views_against_float64(emu, case, mode):
    check_against_float64("cpu", case, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_two_views_against_float64(case, mode):
    check_against_float64(DEV, case, mode)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def refusals(logits, acc):
    """every rejected argument of both entries, on pointers that a launch would reach: each returns < 0 with a message"""
    L = nat.lib()

    def accumulate(logits=logits, ld=12, C=10, matrix=None, src=None, weight=1.0, mode=1, interp=1, layout=0, acc=acc, acc_ld=12,
                   no_matrix=False):
        A = (ctypes.c_float * 12)(*(identity().reshape(-1).tolist() if matrix is None else matrix))
        held = (ctypes.c_int32 * C)(*(src if src is not None else range(C)))
        rc = L.ctseg_tta_accumulate(logits, ld, C, 2, 2, 2, None if no_matrix else ctypes.addressof(A),
                                    None if src is None else ctypes.addressof(held), weight, mode, interp, 2, 2, 2, layout, acc, acc_ld, None)
        return rc, L.ctseg_last_error().decode()

    def finish(acc=acc, acc_ld=12, C=10, St=8, mode=1, labels=acc):
        rc = L.ctseg_tta_finish(acc, acc_ld, C, St, mode, labels, None, None, None)
        return rc, L.ctseg_last_error().decode()
    for kw in ({"logits": None}, {"acc": None}, {"no_matrix": True}):
        rc, msg = accumulate(**kw)
        assert rc < 0 and "null pointer" in msg, msg
    for bad in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 6, 11):
            A = identity().reshape(-1).tolist()
            A[at] = bad
            rc, msg = accumulate(matrix=A)
            assert rc < 0 and "matrix" in msg and "finite" in msg, msg
    A = identity().reshape(-1).tolist()
    A[5] = 3e38
    rc, msg = accumulate(matrix=A)
    assert rc < 0 and "1e30" in msg, msg
    for weight in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = accumulate(weight=weight)
        assert rc < 0 and "weight" in msg, msg
    for src in ([0, 1, 2, 3, 4, 5, 6, 7, 8, 8], [0, 1, 2, 3, 4, 5, 6, 7, 8, 10], [-1, 1, 2, 3, 4, 5, 6, 7, 8, 9]):
        rc, msg = accumulate(src=src)
        assert rc < 0 and "permutation" in msg, msg
    for kw, word in (({"mode": 2}, "mode"), ({"mode": -1}, "mode"), ({"interp": 2}, "interp"), ({"interp": -1}, "interp"),
                     ({"layout": 2}, "layout"), ({"layout": -1}, "layout"), ({"ld": 10}, "ld"), ({"ld": 8}, "ld"),
                     ({"acc_ld": 10}, "acc_ld"), ({"acc_ld": 8}, "acc_ld"), ({"C": 12, "acc_ld": 12}, "acc_ld"),
                     ({"C": 17, "ld": 20, "acc_ld": 20}, "C ="), ({"C": 0}, "C =")):
        rc, msg = accumulate(**kw)
        assert rc < 0 and word in msg, msg
    for kw, word in (({"acc": None}, "null pointer"), ({"labels": None}, "null pointer"), ({"acc_ld": 10}, "acc_ld"), ({"acc_ld": 8}, "acc_ld"),
                     ({"C": 17, "acc_ld": 20}, "C ="), ({"mode": 2}, "mode"), ({"St": 0}, "St"), ({"St": 1 << 31}, "St")):
        rc, msg = finish(**kw)
        assert rc < 0 and word in msg, msg


def test_entries_reject_bad_arguments_without_a_device():
    held = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(held) + 15) // 16 * 16
    refusals(p, p + 1024)
    assert {"ctseg_tta_accumulate", "ctseg_tta_finish"} <= set(nat.EXPORTS) and nat.ABI_VERSION == 3


@pytest.mark.gpu
def test_gpu_refusals_launch_nothing():
    logits = torch.randn(8 * 12, device=DEV)
    acc = torch.full((8 * 12,), SENTINEL, device=DEV)
    refusals(logits.data_ptr(), acc.data_ptr())
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all())


# ---- 8. host logic -----------------------------------------------------------------------------------------------------------
def test_view_to_target_matrix_inverts_the_view():
    rng = np.random.default_rng(4)
    aug = T.Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), translate=(2, 8, 8), flip_prob=(0.5, 0.5, 0.5))
    for size in VIEW_GRIDS + [(96, 256, 256)]:
        for params in [GENERAL, T.Augment3D.identity_params()] + [aug.draw(rng) for _ in range(4)]:
            A = np.vstack([T.Augment3D.matrix(size, params, dtype=np.float64), [0, 0, 0, 1]])
            M = tta.view_to_target_matrix(size, params, dtype=np.float64)
            assert M.dtype == np.float64 and np.abs(A @ np.vstack([M, [0, 0, 0, 1]]) - np.eye(4)).max() < 1e-12
            m32 = tta.view_to_target_matrix(size, params)
            assert m32.dtype == np.float32 and np.array_equal(m32, M.astype(np.float32))
            native = (140, 512, 500)
            N = tta.view_to_target_matrix(size, params, native, dtype=np.float64)
            S = np.diag([size[a] / native[a] for a in range(3)] + [1.0])
            assert np.abs(A @ np.vstack([N, [0, 0, 0, 1]]) - S).max() < 1e-12
    assert np.array_equal(tta.view_to_target_matrix((9, 33, 33), T.Augment3D.identity_params()), identity())
    flip_w = dict(T.Augment3D.identity_params(), flips=(False, False, True))
    assert np.array_equal(tta.view_to_target_matrix((9, 33, 33), flip_w), flip_matrix(2, (9, 33, 33)))


def test_augment_matrix_without_the_keyword_keeps_its_bits():
    """Augment3D.matrix((33, 6, 70), GENERAL) as recorded before the dtype keyword existed: the float32 bit patterns"""
    recorded = [0x3F684021, 0x3D6A4ED8, 0x3D1428BF, 0x3F4B1CFA, 0xBD14B83B, 0x3F894255, 0xBE7C65D9, 0x40D351C6,
                0xBD3A1AB0, 0x3E921147, 0x3F6B5214, 0x408CD1DE]
    got = T.Augment3D.matrix((33, 6, 70), GENERAL)
    assert got.dtype == np.float32 and got.reshape(-1).view(np.uint32).tolist() == recorded
    assert np.array_equal(got, T.Augment3D.matrix((33, 6, 70), GENERAL, dtype=np.float64).astype(np.float32))


def test_class_map_and_mirror_views():
    ident = T.Augment3D.identity_params()
    assert tta.class_channel_src(ident) == list(range(10))
    assert tta.class_channel_src(dict(ident, flips=(True, True, False))) == list(range(10))
    assert tta.class_channel_src(dict(ident, flips=(False, False, True))) == [0, 1, 2, 3, 5, 4, 7, 6, 9, 8] == CLASS_SWAPPED
    assert tta.class_channel_src(dict(ident, flips=(False, False, True)), T.Augment3D(swap_pairs=((0, 1),)), 3) == [0, 2, 1, 3]
    assert tta.mirror_views(()) == [ident]
    assert [v["flips"] for v in tta.mirror_views()] == [(False, False, False), (False, False, True)]
    group = tta.mirror_views(("d", "h", "w"))
    assert len(group) == 8 and group[0] == ident and len({v["flips"] for v in group}) == 8
    assert [v["flips"] for v in group[:3]] == [(False, False, False), (False, False, True), (False, True, False)]
    assert all(v["applied"] == any(v["flips"]) and v["angles"] == (0.0, 0.0, 0.0) for v in group)
    from capstone_amd import volumetric
    assert volumetric.TestTimeAugmenter3D is tta.TestTimeAugmenter3D and volumetric.mirror_views is tta.mirror_views


def test_cpu_tensors_raise():
    aug = tta.TestTimeAugmenter3D(tta.mirror_views(), size=(8, 16, 16))
    with pytest.raises(nat.NativeError):
        aug.predict(lambda x: x, torch.zeros(8, 16, 16))
    with pytest.raises(nat.NativeError):
        aug.predict_batch(lambda x: x, torch.zeros(1, 1, 16, 16, 8))
    with pytest.raises(nat.NativeError):
        tta.tta_accumulate(torch.zeros(8, 4), torch.zeros(1, 3, 2, 2, 2), identity())
    with pytest.raises(nat.NativeError):
        tta.tta_finish(torch.zeros(8, 4), 3)
    with pytest.raises(ValueError):
        tta.TestTimeAugmenter3D([], size=(8, 16, 16))
    with pytest.raises(ValueError):
        tta.TestTimeAugmenter3D(tta.mirror_views(), weights=[1.0, 0.0])


def _model_and_batch(dev="cpu", **switches):
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(7)
    m = BaseUNet3D(filters=[4, 8, 8], loss_fx=["CrossEntropy"], **switches).to(dev)
    g = torch.Generator().manual_seed(3)
    masks = torch.zeros(2, 9, 16, 16, 8, dtype=torch.uint8)
    for c in range(9):
        masks[:, c, c:c + 6, 2:12, 1:6] = 1
    return m, (torch.randn(2, 1, 16, 16, 8, generator=g).to(dev), masks.to(dev), torch.ones(2, 9).to(dev))


NEW_ENTRIES = {"ctseg_augment3d_to_hwd", "ctseg_tta_accumulate", "ctseg_tta_finish"}


def test_trainer_switch_through_the_emulator(calls):
    off, batch = _model_and_batch()
    assert off.tta is None and off.tta_dice_score is None
    with torch.no_grad():
        off.validation_step(batch)
    plain = list(calls)
    assert not NEW_ENTRIES & set(plain) and not any("TTA" in k for k in off.logged)
    with pytest.raises(ValueError):
        off.predict_volume(torch.zeros(8, 16, 16))
    del calls[:]
    # the identity view alone, nearest: the ensemble is the plain prediction, and scores the same
    one = tta.TestTimeAugmenter3D([T.Augment3D.identity_params()], size=(8, 16, 16), interp="nearest")
    m, batch = _model_and_batch(tta=one)
    assert "tta" not in m.hparams
    with torch.no_grad():
        m.validation_step(batch)
    assert calls[:len(plain)] == plain                                    # what ran before still runs, first and unchanged
    assert [c for c in calls if c in NEW_ENTRIES] == ["ctseg_augment3d_to_hwd", "ctseg_tta_accumulate", "ctseg_tta_finish"] * 2
    keys = {f"{s} Dice (val TTA)" for s in STRUCTURES} | {"Mean Dice Score (val TTA)"}
    assert set(m.logged) - set(off.logged) == keys
    assert torch.equal(m.logged["Mean Dice Score (val TTA)"], m.logged["Mean Dice Score (val)"])
    with torch.no_grad():
        want = _squash_predictions(m(batch[0]))
        got = one.predict_batch(m, batch[0])
    assert got.labels.dtype == torch.uint8 and torch.equal(got.labels.long(), want) and got.uncovered.tolist() == [0, 0]
    acc = one._acc
    assert acc.shape == (8 * 16 * 16, 12) and one.predict_batch(m, batch[0]) is not None and one._acc is acc      # reused
    del calls[:]
    loss = m.training_step(batch)                                         # training steps never run it
    assert torch.isfinite(loss) and not NEW_ENTRIES & set(calls)
    # the mirror pair: two views a sample, the keys again; a raw scan goes back to its own grid
    pair = tta.TestTimeAugmenter3D(tta.mirror_views(), size=(8, 16, 16))
    m2, batch = _model_and_batch(tta=pair)
    del calls[:]
    with torch.no_grad():
        m2.validation_step(batch)
    assert [c for c in calls if c in NEW_ENTRIES] == (["ctseg_augment3d_to_hwd", "ctseg_tta_accumulate"] * 2 + ["ctseg_tta_finish"]) * 2
    assert keys <= set(m2.logged)
    scan = torch.from_numpy(np.random.default_rng(0).integers(-1000, 1000, (11, 20, 19)).astype(np.int16))
    res = m2.predict_volume(scan, want_probs=True)
    assert res.labels.shape == (11, 20, 19) and res.labels.dtype == torch.uint8 and res.probs.shape == (11, 20, 19, 10)
    assert int(res.uncovered) == 0 and int(res.hist.sum()) == scan.numel()
    assert m2.predict_volume(scan, native=False).labels.shape == (16, 16, 8)


# ---- 9. GPU end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_end_to_end_identity_view_and_native_grid():
    from capstone_amd.models import UNet
    torch.manual_seed(5)
    net = UNet(3, 1, 10, (4, 8), (2,), num_res_units=2).to(DEV)
    size = (8, 16, 16)
    scan = torch.from_numpy(np.random.default_rng(1).integers(-1000, 1000, (13, 40, 37)).astype(np.int16)).to(DEV)
    ident = T.Augment3D.identity_params()
    with torch.no_grad():
        x = T.augment3d_to_hwd(scan, None, size, identity(), 1)[0][None, None]
        logits = net(x).clone()
        want = _squash_predictions(logits)[0]
    one = tta.TestTimeAugmenter3D([ident], size=size, interp="nearest")
    res = one.predict(net, scan)
    assert res.labels.shape == (16, 16, 8) and res.labels.dtype == torch.uint8 and torch.equal(res.labels.long(), want)
    assert int(res.uncovered) == 0 and int(res.hist.sum()) == want.numel()
    # the scan's own grid, mean of logits so that the comparison is exact: the oracle on the same logits
    blk = logits[0].permute(1, 2, 3, 0).contiguous().cpu().numpy()
    for interp in ("nearest", "trilinear"):
        native = tta.TestTimeAugmenter3D([ident], size=size, mode="logits", interp=interp).predict(net, scan, native=True, want_probs=True)
        M = tta.view_to_target_matrix(size, ident, tuple(scan.shape))
        acc = oracle_run([(blk, M, None, 1.0)], 10, tuple(scan.shape), 1, 0, int(interp == "trilinear"))
        lab, pr, hs, uncovered = oracle_finish(acc, 10, 0)
        assert native.labels.shape == scan.shape and native.labels.dtype == torch.uint8
        # (h: 39 * 16 / 40 + .5 rounds to 16, one past the view, and w likewise: the scan's last h row and w column are covered by
        # no view and keep label 0)
        assert np.array_equal(native.labels.cpu().numpy().reshape(-1), lab) and int(native.uncovered) == uncovered == 13 * (40 + 37 - 1)
        assert not native.labels[:, 39].any() and not native.labels[:, :, 36].any()
        assert np.array_equal(native.hist.cpu().numpy(), hs) and native.probs.shape == tuple(scan.shape) + (10,)
        assert np.abs(native.probs.cpu().numpy().reshape(-1, 10) - pr).max() < 1e-5


@pytest.mark.gpu
def test_gpu_trainer_logs_the_ensemble_scores():
    pair = tta.TestTimeAugmenter3D(tta.mirror_views(), size=(8, 16, 16))
    m, batch = _model_and_batch(DEV, tta=pair, surface_metrics=True)
    with torch.no_grad():
        m.validation_step(batch)
    m.on_validation_epoch_end()
    assert {f"{s} Dice (val TTA)" for s in STRUCTURES} | {"Mean Dice Score (val TTA)"} <= set(m.logged)
    assert set(m._surface_kept) == {"val", "val TTA"}
    assert any(k.endswith("HD95 (val TTA)") for k in m.logged) == any(k.endswith("HD95 (val)") for k in m.logged)
    merged = pair.predict_batch(m, batch[0]).labels
    assert merged.shape == (2, 16, 16, 8) and int(merged.max()) <= 9
