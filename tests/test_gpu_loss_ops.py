"""GPU: the loss and metric kernels at op level against float64 — ctseg_seg_loss / ctseg_seg_loss_pair (statistics records, Dice
counts, predictions, gradients), ctseg_squash_masks(_present), ctseg_dice_counts, ctseg_reduce_partials_f64,
ctseg_loss_dice_summary, and ctseg_conv_logits_ce (the logits convolution with the cross-entropy fused into its epilogue).

The references are reference_ops.seg_loss_terms / seg_loss_grad (checked against F.cross_entropy and autograd on the CPU) and
numpy; the inputs come from loss_cases.py, whose promises (exact logits, margins, the four regions of the fused-head case, the sum
bound inside its cap) tests/test_reference_ops.py asserts on the CPU.  Bounds: helpers.sum_bound for every sum (16 x the error of
the plain float32 torch evaluation, normalised by the sum of |terms|, under 1 / (4 rows)), helpers.check_elems for every gradient
element (u |ref| + 16 e32), exact equality for counts, predictions, labels and histograms.  ctseg_reduce_partials_f64: 16 x the
error of numpy's own float64 pairwise sum against math.fsum.  ctseg_loss_dice_summary keeps the figures of the check it extends
(tests/test_gpu_parity.py: 1e-6 relative on the loss and the scores against the float32 torch expressions).

ctseg_conv_logits_ce.  The grid of the pass is min(2 x compute units, tiles), so it never exceeds the tile count; a workgroup
without tiles exists all the same: a grid that is a multiple of 8 walks the tiles in 8 chunks of ceil(tiles / 8), and with 9 tiles
under CTSEG_MAX_WG = 8 the chunks of workgroups 5, 6 and 7 are empty (test_fused_head_workgroups_without_tiles).  Columns 12 to 15
of a 16-wide d loss / d logits row: the pass stores columns 0 to 11 only; the plan allocates the buffer zeroed (plan.py:
plan_act -> engine.new_act, zero=True) and every writer either stores zeros there (ctseg_seg_loss) or leaves them (this pass, the
copy of an upstream gradient into columns [0, C)), so the state the plan guarantees is 0: the test prepares that state and asserts
it after the launch.  (The same guarantee for the assembled step, where this row is the next pass's gathered operand:
tests/test_plan_buffers.py runs the whole step over a poisoned workspace and asserts every range the buffer registry declares
zero, capstone_amd.engine.ZERO_PAD / ZERO_UNWRITTEN, after it; DESIGN.md "Buffer roles" lists them.)

Every test prints its worst error / bound before it asserts.  Measured on an MI355X, worst of each group:
  ctseg_seg_loss record sums 0.15, ctseg_seg_loss_pair (13 classes) 0.005; gradients fp32 0.08 (cross-entropy only 0.07), bf16 0.99
  (the u |ref| term: round-to-nearest at the bottom of a binade is half a bf16 ulp = 2^-8 relative);
  ctseg_reduce_partials_f64 0.13; fused head (ce, weight) sums 0.06, gradient bf16 0.99, fp16 0.50.
The fused-head cases of three samples found a bug, fixed with them: a workgroup that walks the tiles with a stride above one
(a grid that is no multiple of 8, as under CTSEG_MAX_WG = 3, or 6 tiles on 6 workgroups) wrote no record for a sample lying between
or behind the samples of its tiles, where the host expects zeros; only a buffer that was zero before the launch hid it.

The regimes (loss_cases.py).  The cases above are the first step of training: logits a few units around zero.  A trained network
is confident on most voxels (the label's logit 6 to 10 above the rest, cross-entropy 1e-3 and below, "confident"), its head bias
has moved off zero ("shifted+64", "shifted+250", "shifted-64"), and some voxels saturate the softmax ("saturated": leads of 30 to
120 and of 3e4, a row of equal logits at -3e4, a label probability of exactly 1.0); the fused head has a variant with every bias
64 higher and one with a block that predicts class 0 with a lead of about 6.  That is where log-sum-exp code loses digits: the
kernels formed the cross-entropy as (m + log(sum)) - x_t, a sum rounded at the magnitude of m before the subtraction cancels it.
Worst error / bound on an MI355X, the parent commit's library -> this one:
  ctseg_seg_loss record sums: confident 0.24 -> 0.07, shifted+64 0.50 -> 0.07, shifted+250 0.77 -> 0.07, shifted-64 0.22 -> 0.07,
  saturated 0.06 -> 0.04; ctseg_seg_loss_pair: confident 0.015 -> 0.013, shifted+64 0.019 -> 0.005;
  gradients, cross-entropy only: fp32 0.10 -> 0.10 (that path has no logarithm), bf16 0.99; soft path, confident and shifted: fp32
  0.43 -> 0.08, bf16 0.99 -> 0.99; soft path, saturated: fp32 52.3 -> 0.12, bf16 3.4 -> 0.96;
  fused head (ce, weight) sums: shifted 0.19 -> 0.02, confident 0.03 -> 0.04; gradients bf16 0.98, fp16 0.50, unchanged.
The sums of the parent are inside the bound: sum_bound takes torch's float32 sum of the terms as its measure, whose own error
(1e-8) is above that of the rounding at m.  Seven of the twelve saturated soft-path gradient cases are outside it.
Fixed here: log p_t = x_t - (m + log(sum)) of the row of equal logits at -3e4 carried the rounding of -3e4 + log C (up to 1e-3)
into the focal gradient term f (2 (1 - p_t) p_t log p_t - (1 - p_t)^2).  All three kernels now form log(sum) + (m - x_t) and
(x_t - m) - log(sum), the order of torch's float32 cross_entropy, with the same instructions."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd import segloss  # noqa: E402
from capstone_amd._native import BF16, F16, F32  # noqa: E402
from helpers import ACT_SENTINEL, CAP_IDS, CAPS, HALO_X, ConvPassDriver, cap_env, check_elems, sum_bound  # noqa: E402
from loss_cases import (HEAD_CASES, HEAD_EMPTY_WG_CASE, HEAD_IDS, HEAD_LOSS_SCALE, HEAD_VARIANT_CASES, HEAD_VARIANT_IDS, SEG_B,  # noqa: E402
                        SEG_REGIME_SHAPES, SEG_REGIMES, SEG_S, SEG_SHAPES, head_reference, partials_case, partials_reference,
                        seg_class_weight, seg_loss_case, seg_stats_reference)
from reference_ops import conv_module, dice_count_table, seg_loss_grad, seg_loss_records, seg_loss_terms  # noqa: E402

DEV = "cuda:0"
PART_SENTINEL = -7.0e300         # no record entry of any case comes near it
GUARD = 8                        # guard rows on both sides of a gradient buffer (8 rows of 12 or 16 elements: a multiple of 16 bytes)
DT = {"bf16": BF16, "fp16": F16}


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _sum_ratio(tag, got, ref):
    """|got - float64 sums| / sum |terms| against the case's bound, entry by entry (an entry without a nonzero term: exactly 0)"""
    err = (got.cpu().double() - ref["sums"]).abs() / ref["norm"]
    ratio = float(err.max() / ref["bound"])
    print(f"{tag}: worst error / bound {ratio:.3f} (bound {ref['bound']:.2e})")
    assert bool((got.cpu()[~ref["live"]] == 0).all()), (tag, "a sum without a term")
    assert ratio <= 1.0, (tag, ratio)
    return ratio


def _reduce(part, B, P, R):
    red = torch.full((B, R), PART_SENTINEL, dtype=torch.float64, device=DEV)
    nat.call("ctseg_reduce_partials_f64", part.data_ptr(), B, P, R, red.data_ptr())
    return red


def _seg_loss(x, ld, labels, B, S, C, cw, do_stats, P, do_grad=0, coef=None, dl_ptr=None, g_ld=0, gdt=F32):
    """one ctseg_seg_loss launch on sentinel-filled outputs -> (part (B, P, R), cnt (B, 3, C), pred (B, S))"""
    R = 2 + 3 * C
    part = torch.full((B, P, R), PART_SENTINEL, dtype=torch.float64, device=DEV)
    cnt = torch.zeros((B, 3, C), dtype=torch.int64, device=DEV)
    pred = torch.full((B, S), 255, dtype=torch.uint8, device=DEV)
    nat.call("ctseg_seg_loss", x.data_ptr(), ld, labels.data_ptr(), B, S, C, nat.ptr(cw), do_stats, part.data_ptr(), P, cnt.data_ptr(),
             do_grad, nat.ptr(coef), dl_ptr, g_ld, gdt, pred.data_ptr())
    torch.cuda.synchronize()
    return part, cnt, pred


# ---- ctseg_seg_loss: statistics ------------------------------------------------------------------------------------------------
def _check_stats(tag, ref, part, cnt, pred, B, P, C, ce_only):
    R = 2 + 3 * C
    assert not bool((part == PART_SENTINEL).any()), "every workgroup writes its whole record"
    assert torch.equal(cnt.cpu(), ref["cnt"]), "Dice counts"
    assert torch.equal(pred.cpu().long(), ref["pred"]), "predictions"
    red = _reduce(part, B, P, R)
    torch.cuda.synchronize()
    if ce_only:
        assert bool((red[:, 2:] == 0).all()) and bool((part[..., 2:] == 0).all()), "cross-entropy only: entries 2 and up are 0"
    return _sum_ratio(tag, red, ref)


@pytest.mark.parametrize("do_stats", [1, 2], ids=["full", "ce-only"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("S", SEG_S)
@pytest.mark.parametrize("C,ld", SEG_SHAPES)
def test_seg_loss_statistics_vs_float64(C, ld, S, weighted, do_stats):
    ref = seg_stats_reference(C, ld, S, weighted, do_stats == 2)
    case = ref["case"]
    P = segloss.SegLossEngine(torch.device(DEV), SEG_B, S, C).P
    assert P == (3 if S == 4221 else 1)
    x, labels, cw = _dev(case["x"]), _dev(case["labels"]), _dev(ref["cw"])
    part, cnt, pred = _seg_loss(x, ld, labels, SEG_B, S, C, cw, do_stats, P)
    _check_stats(f"seg_loss statistics C={C} ld={ld} S={S} weighted={weighted} do_stats={do_stats}", ref, part, cnt, pred, SEG_B, P, C,
                 do_stats == 2)


@pytest.mark.parametrize("do_stats", [1, 2], ids=["full", "ce-only"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("S", SEG_S)
@pytest.mark.parametrize("C,ld", SEG_REGIME_SHAPES)
@pytest.mark.parametrize("regime", SEG_REGIMES)
def test_seg_loss_statistics_by_regime_vs_float64(regime, C, ld, S, weighted, do_stats):
    """the logits of a trained network (loss_cases.py: confident, shifted, saturated).  Saturated: every record entry finite; an
    entry whose float64 terms are all zero is exactly 0 (_sum_ratio asserts that of every case)"""
    ref = seg_stats_reference(C, ld, S, weighted, do_stats == 2, regime=regime)
    case = ref["case"]
    P = 3 if S == 4221 else 1
    part, cnt, pred = _seg_loss(_dev(case["x"]), ld, _dev(case["labels"]), SEG_B, S, C, _dev(ref["cw"]), do_stats, P)
    assert bool(torch.isfinite(part).all()), "a record entry that is not finite"
    _check_stats(f"seg_loss statistics {regime} C={C} ld={ld} S={S} weighted={weighted} do_stats={do_stats}", ref, part, cnt, pred, SEG_B,
                 P, C, do_stats == 2)


@pytest.mark.parametrize("do_stats", [1, 2], ids=["full", "ce-only"])
def test_seg_loss_workgroups_without_voxels_write_zero_records(do_stats):
    """S = 10 over P = 7 workgroups of two voxels: workgroups 5 and 6 start at or behind the end of the sample"""
    C, ld, S, P = 10, 12, 10, 7
    ref = seg_stats_reference(C, ld, S, True, do_stats == 2)
    case = ref["case"]
    part, cnt, pred = _seg_loss(_dev(case["x"]), ld, _dev(case["labels"]), SEG_B, S, C, _dev(ref["cw"]), do_stats, P)
    assert bool((part[:, 5:] == 0).all()), "empty workgroups: zero records"
    assert bool((part[:, :5, 1] > 0).all()), "the others hold two voxels each"
    _check_stats(f"seg_loss statistics S=10 P=7 do_stats={do_stats}", ref, part, cnt, pred, SEG_B, P, C, do_stats == 2)


def test_seg_loss_pair_statistics_at_13_classes_vs_two_float64_sides():
    """seg_loss_pair_kernel<float, 16, false>: side 0 of sample b is labels[b], side 1 labels[perm[b]].  Its records are 2 x 41
    doubles, more than ctseg_reduce_partials_f64 takes, so the P = 3 partial records are added in float64 on the host"""
    _pair_statistics("initial")


@pytest.mark.parametrize("regime", ["confident", "shifted+64"])
def test_seg_loss_pair_statistics_by_regime(regime):
    """the same launch on the logits of a trained network.  Confident: the logits lead at the labels of side 0, so side 1 (the labels
    of another sample) is wrong on most voxels: one side with a cross-entropy of 1e-3, one of about 10 per voxel"""
    _pair_statistics(regime)


def _pair_statistics(regime):
    C, ld, S, B, P = 13, 16, 4221, SEG_B, 3
    R = 2 + 3 * C
    perm = [1, 1, 0]
    case = seg_loss_case(C, ld, S, regime=regime)
    cw2 = torch.stack([seg_class_weight(C), seg_class_weight(C).flip(0)])
    x, labels = _dev(case["x"]), _dev(case["labels"])
    part = torch.full((B, P, 2, R), PART_SENTINEL, dtype=torch.float64, device=DEV)
    cnt = torch.zeros((B, 2, 3, C), dtype=torch.int64, device=DEV)
    perm_d, cw_d = _dev(torch.tensor(perm, dtype=torch.int32)), _dev(cw2)
    nat.call("ctseg_seg_loss_pair", x.data_ptr(), ld, labels.data_ptr(), perm_d.data_ptr(), B, S, C, cw_d.data_ptr(), 0, part.data_ptr(), P,
             cnt.data_ptr(), None, None, 0, F32)
    torch.cuda.synchronize()
    assert not bool((part == PART_SENTINEL).any())
    for s, lab in enumerate((case["labels"], case["labels"][perm])):
        t64 = seg_loss_terms(case["x"].double(), lab, C, cw2[s].double())
        t32 = seg_loss_terms(case["x"], lab, C, cw2[s])
        s64, norm, live, bound = sum_bound(f"pair side {s} {regime}", seg_loss_records(t64), seg_loss_records(t32), (1,), rows=S)
        assert torch.equal(cnt[:, s].cpu(), t64["cnt"]), ("Dice counts", s)
        _sum_ratio(f"seg_loss_pair statistics {regime} C=13 side {s}", part[:, :, s].cpu().sum(1), dict(sums=s64, norm=norm, live=live, bound=bound))


# ---- ctseg_seg_loss: gradients -----------------------------------------------------------------------------------------------------
def _guarded_rows(rows, g_ld, dt, pad_state=None):
    """(whole buffer, pointer to row GUARD): rows + 2 GUARD rows of g_ld elements holding ACT_SENTINEL; ``pad_state``: what
    columns 12 .. of the inner rows hold instead"""
    buf = torch.full((rows + 2 * GUARD, g_ld), ACT_SENTINEL, dtype=nat.torch_dtype(dt), device=DEV)
    if pad_state is not None and g_ld > 12:
        buf[GUARD:-GUARD, 12:] = pad_state
    assert (GUARD * g_ld * buf.element_size()) % 16 == 0
    return buf, buf.data_ptr() + GUARD * g_ld * buf.element_size()


def _check_guards(buf):
    assert bool((buf[:GUARD] == ACT_SENTINEL).all()) and bool((buf[-GUARD:] == ACT_SENTINEL).all()), "rows outside the B * S rows changed"


GRAD_CASES = [(10, 12, F32), (8, 8, BF16), (10, 12, BF16), (10, 16, BF16), (13, 16, F32), (16, 16, BF16)]


@pytest.mark.parametrize("path", ["ce-only", "full"])
@pytest.mark.parametrize("S", SEG_S)
@pytest.mark.parametrize("C,g_ld,gdt", GRAD_CASES, ids=[f"C{c}-g{g}-{'fp32' if d == F32 else 'bf16'}" for c, g, d in GRAD_CASES])
def test_seg_loss_gradient_vs_float64(C, g_ld, gdt, S, path):
    _gradient(C, g_ld, gdt, S, path, "initial")


# every (C, ld) of SEG_REGIME_SHAPES in fp32 and bf16, 12- and 16-wide gradient rows
REGIME_GRAD_CASES = [(10, 12, F32), (10, 16, BF16), (13, 16, F32), (13, 16, BF16), (2, 12, BF16), (2, 16, F32)]


@pytest.mark.parametrize("path", ["ce-only", "full"])
@pytest.mark.parametrize("S", SEG_S)
@pytest.mark.parametrize("C,g_ld,gdt", REGIME_GRAD_CASES, ids=[f"C{c}-g{g}-{'fp32' if d == F32 else 'bf16'}" for c, g, d in REGIME_GRAD_CASES])
@pytest.mark.parametrize("regime", SEG_REGIMES)
def test_seg_loss_gradient_by_regime_vs_float64(regime, C, g_ld, gdt, S, path):
    """the logits of a trained network through both gradient paths; every stored element is finite.  A voxel whose label has the
    float32 probability 1.0 (the right voxels of the saturated regime), as measured on an MI355X: with fp32 stores the row has
    exactly the zero pattern of the float32 evaluation (every such row of all twelve cases); with bf16 stores it has not (a fifth
    to a quarter of the rows differ: the conversion rounds an element below the bf16 subnormals to 0, where the evaluation keeps
    1e-40).  What holds for both, and is asserted: the row lies within the element bound, as every row does (check_elems), and on
    the cross-entropy-only path the label's own element, s w (p_t - 1), is exactly 0.  The fp32 zero pattern is printed, not
    asserted: which elements are zero rests on how the host's float32 exp rounds a subnormal (8e-40 at a lead of 90), a property
    of the reference, not of the kernel."""
    _gradient(C, g_ld, gdt, S, path, regime)


def _gradient(C, g_ld, gdt, S, path, regime):
    ld = (C + 3) // 4 * 4
    assert (C, ld) in SEG_SHAPES
    case = seg_loss_case(C, ld, S, regime=regime)
    B = SEG_B
    if path == "ce-only":            # what fused_ce launches: do_stats = 2 and do_grad = 2 in one pass, one scale per sample
        coef = torch.zeros(B, 1 + 3 * C)
        coef[:, 0] = (torch.arange(B) + 1.0) / float(B * S)
        cw, do_stats, do_grad = seg_class_weight(C), 2, 2
    else:                            # what grad launches: the coefficient tables of every loss, no statistics
        coef, cw, do_stats, do_grad = case["coef"], case["cw"], 0, 1
    ref64 = seg_loss_grad(case["x"].double(), case["labels"], C, coef.double(), cw.double())
    ref32 = seg_loss_grad(case["x"], case["labels"], C, coef, cw)
    buf, dl_ptr = _guarded_rows(B * S, g_ld, gdt)
    P = 3 if S == 4221 else 1
    part, cnt, pred = _seg_loss(_dev(case["x"]), ld, _dev(case["labels"]), B, S, C, _dev(cw), do_stats, P, do_grad, _dev(coef), dl_ptr, g_ld,
                                gdt)
    got = buf[GUARD:-GUARD].float().cpu().double().reshape(B, S, g_ld)
    assert bool(torch.isfinite(got).all()), "a stored element that is not finite"
    tag = f"seg_loss gradient {path} C={C} g_ld={g_ld} dtype={gdt} S={S}" + ("" if regime == "initial" else " " + regime)
    check_elems(tag, got[..., :C], ref64, ref32, gdt)
    if g_ld > C:
        assert float(got[..., C:].abs().max()) == 0.0, "the padding columns of every written row read 0"
    _check_guards(buf)
    if do_stats:
        assert torch.equal(cnt.cpu(), seg_stats_reference(C, ld, S, False, True, regime=regime)["cnt"])
    if regime == "saturated":
        lab = case["labels"].long()
        one = seg_loss_terms(case["x"], lab, C)["py"].sum(-1) == 1.0
        assert bool(one[case["label_leads"]].all()) and int(one.sum()) > S // 2
        same = ((got[..., :C] == 0) == (ref32 == 0)).all(-1)[one]
        print(f"{tag}: {int(one.sum())} rows with a float32 label probability of 1.0, zero pattern of the float32 evaluation on "
              f"{int(same.sum())} of them")
        if path == "ce-only":
            assert float(got[..., :C].gather(-1, lab[..., None])[..., 0][one].abs().max()) == 0.0, "s w (p_t - 1) at p_t = 1.0"


# ---- ctseg_squash_masks / ctseg_squash_masks_present ------------------------------------------------------------------------------
def _squash_check(masks_np, B, K, S, masks_dev):
    lab_ref = (masks_np.astype(np.int64) * np.arange(1, K + 1)[None, :, None]).max(1)
    hist_ref = np.stack([np.bincount(lab_ref[b], minlength=K + 1) for b in range(B)])
    pres_ref = (masks_np == 1).any(2)
    for want_present in (False, True):
        lab = torch.full((16 + B * S + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        lab64 = torch.full((B, S), -1, dtype=torch.int64, device=DEV)
        hist = torch.zeros((B, K + 1), dtype=torch.int64, device=DEV)
        args = [masks_dev.data_ptr(), B, K, S, lab.data_ptr() + 16, lab64.data_ptr(), hist.data_ptr()]
        if want_present:
            present = torch.zeros((B, K), dtype=torch.int32, device=DEV)
            nat.call("ctseg_squash_masks_present", *args, present.data_ptr())
        else:
            nat.call("ctseg_squash_masks", *args)
        torch.cuda.synchronize()
        assert np.array_equal(lab[16:-16].cpu().numpy().reshape(B, S), lab_ref), "labels"
        assert bool((lab[:16] == 0xEE).all()) and bool((lab[-16:] == 0xEE).all()), "bytes around the label map"
        assert np.array_equal(lab64.cpu().numpy(), lab_ref), "int64 map"
        assert np.array_equal(hist.cpu().numpy(), hist_ref), "histogram"
        if want_present:
            assert np.array_equal(present.cpu().numpy().astype(bool), pres_ref) and int(present.max()) <= 1, "present"


def _masks(B, K, S, seed, density):
    rng = np.random.default_rng(seed)
    m = (rng.random((B, K, S)) < density).astype(np.uint8)
    if K > 2:
        m[0, 1] = 0                     # a structure absent from a sample
        m[B - 1, K - 1] = 0
        m[B - 1, 0] = 1                 # a structure present everywhere ...
        if K > 3:
            m[B - 1, 2, :] = m[B - 1, 3, :]      # ... and one wholly under a higher-numbered one: present, yet not in the histogram
    return m


@pytest.mark.parametrize("S", [7, 16, 4221, 1536])
@pytest.mark.parametrize("K", [1, 9, 15, 31])
def test_squash_masks_vs_numpy(K, S):
    B = 2
    m = _masks(B, K, S, 100 * K + S, 0.08)
    _squash_check(m, B, K, S, torch.from_numpy(m).to(DEV))


@pytest.mark.parametrize("K", [1, 9, 31])
def test_squash_masks_with_a_base_pointer_off_by_one_byte(K):
    """S % 16 == 0 with masks at an odd address: the scalar path"""
    B, S = 2, 1536
    m = _masks(B, K, S, 7 * K, 0.08)
    flat = torch.zeros(B * K * S + 1, dtype=torch.uint8, device=DEV)
    view = flat[1:]
    view.copy_(torch.from_numpy(m).flatten())
    assert view.data_ptr() % 16 == 1
    _squash_check(m, B, K, S, view)


def test_squash_masks_grid_stride_loop():
    """2048 * 256 chunks of 16 voxels fill the capped grid once; 5 more chunks take the loop's second round"""
    B, K, S = 1, 1, 2048 * 256 * 16 + 80
    m = _masks(B, K, S, 5, 0.3)
    _squash_check(m, B, K, S, torch.from_numpy(m).to(DEV))


# ---- ctseg_dice_counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4221, 1024 * 4096 + 5])
@pytest.mark.parametrize("C", [2, 10, 16])
def test_dice_counts_vs_numpy(C, S):
    """labels >= C (255 among them) in both maps, also equal ones at the same voxel: they count nowhere.  The largest S is past the
    1024-workgroup cap: the grid-stride loop"""
    B = 2
    g = torch.Generator().manual_seed(10 * C + S % 11)
    pred = torch.randint(0, C, (B, S), generator=g)
    true = torch.where(torch.rand(B, S, generator=g) < 0.6, pred, torch.randint(0, C, (B, S), generator=g))
    if S > 1:
        for t, sel in ((pred, torch.rand(B, S, generator=g) < 0.05), (true, torch.rand(B, S, generator=g) < 0.05)):
            t[sel] = torch.randint(C, 256, (int(sel.sum()),), generator=g)
        pred[:, 0], true[:, 0] = 255, 255
        pred[:, 1], true[:, 1] = C, C
    else:
        pred[0, 0], true[0, 0] = 255, 255                 # sample 0: nothing to count; sample 1: one voxel
        true[1, 0] = pred[1, 0]
    want = dice_count_table(pred, true, C)
    got = segloss.dice_counts(_dev(pred.to(torch.uint8)), _dev(true.to(torch.uint8)), C)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


# ---- ctseg_reduce_partials_f64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 32, 64])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 2048])
def test_reduce_partials_vs_fsum(P, R):
    B = 2
    part = partials_case(P, R, B)
    exact, mag, bound = partials_reference(part)
    pd = _dev(part)
    a, b = _reduce(pd, B, P, R), _reduce(pd, B, P, R)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "two runs: bit-identical"
    err = float(((a.cpu() - exact).abs() / mag).max())
    print(f"reduce_partials P={P} R={R}: error {err:.2e}, bound {bound:.2e}" + (f", ratio {err / bound:.3f}" if bound else " (exact)"))
    assert err <= bound


# ---- ctseg_loss_dice_summary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,absent_all,absent_one", [(2, None, 1), (2, 1, None), (10, 3, 5), (16, 3, 5), (16, 15, 1)])
def test_loss_dice_summary_vs_the_torch_expressions(C, absent_all, absent_one):
    """the check of tests/test_gpu_parity.py at 2, 10 and 16 classes: a class absent from every sample scores 0, one absent from one
    sample is averaged over the others"""
    B, S = 3, 4096
    le = segloss.SegLossEngine(torch.device(DEV), B, S, C)
    g = torch.Generator().manual_seed(31 + C)
    le.red.copy_(torch.rand(B, le.R, generator=g, dtype=torch.float64) * 100 + 1)
    cnt = torch.randint(1, 500, (B, 3, C), generator=g, dtype=torch.int64)
    if absent_all is not None:
        cnt[:, 2, absent_all] = 0
    if absent_one is not None:
        cnt[1, 2, absent_one] = 0
    cnt[:, 0] = torch.minimum(cnt[:, 0], torch.minimum(cnt[:, 1], cnt[:, 2]))
    le.cnt.copy_(cnt)
    le.hist = cnt[:, 2].clone().to(DEV)
    want_loss = le.loss_values(["CrossEntropy"])["CrossEntropy"]
    want_mean, want_pc = le.dice_metric()
    loss, dm, dpc = le.ce_summary()
    torch.cuda.synchronize()
    # float64, written out: 2 |A & B| / (|A| + |B|) averaged over the samples whose truth holds the class
    c64 = cnt.double()
    ok = c64[:, 2, 1:] > 0
    score = torch.where(ok, 2 * c64[:, 0, 1:] / (c64[:, 1, 1:] + c64[:, 2, 1:]).clamp(min=1), torch.zeros(()).double())
    pc64 = torch.where(ok.sum(0) > 0, score.sum(0) / ok.sum(0).clamp(min=1), torch.zeros(()).double())
    assert abs(float(loss) - float(want_loss)) <= 1e-6 * abs(float(want_loss))
    assert abs(float(loss) - float(le.red[:, 0].sum() / le.red[:, 1].sum())) <= 1e-6 * abs(float(want_loss))
    assert torch.allclose(dpc.cpu(), want_pc.cpu(), rtol=1e-6, atol=1e-7)
    assert torch.allclose(dpc.cpu().double(), pc64, rtol=1e-6, atol=1e-7)
    assert abs(float(dm) - float(want_mean)) <= 1e-6 and abs(float(dm) - float(pc64.mean())) <= 1e-6
    if absent_all is not None:
        assert float(dpc[absent_all - 1]) == 0.0
    if absent_one is not None:
        others = [b for b in range(B) if b != 1]
        assert abs(float(dpc[absent_one - 1]) - float(score[others, absent_one - 1].mean())) <= 1e-6


# ---- ctseg_conv_logits_ce -----------------------------------------------------------------------------------------------------------
def _fused_head(case, monkeypatch, max_wg):
    C, cin, residual, g_ld, dtn, weighted, shape = case[:7]
    variant = case[7] if len(case) > 7 else "base"
    cap_env(monkeypatch, max_wg)
    dt = DT[dtn]
    ref = head_reference(C, cin, residual, weighted, shape, HEAD_LOSS_SCALE[dtn], variant)
    hc = ref["case"]
    N, S, R = shape[0], shape[1] * shape[2] * shape[3], 2 + 3 * C
    tag = f"fused head C={C} cin={cin} residual={residual} g_ld={g_ld} {dtn} weighted={weighted} N={N} max_wg={max_wg}"
    tag += "" if variant == "base" else " " + variant
    mod = conv_module("conv", cin, C)
    with torch.no_grad():
        mod.weight.copy_(hc.w)
        mod.bias.copy_(hc.b)
    drv = ConvPassDriver(mod, dt, DEV, cg=16 if cin == 10 else None)
    xa = drv.act(hc.x, ld=12 if cin == 10 else None)
    # the precondition, on the device: the plain forward's fp32 logits are the float64 logits
    out, _ = drv.fwd(HALO_X, xa, out_f32=True, add=xa if residual else None)
    ld = out.t.shape[-1]
    assert out.t.dtype == torch.float32 and drv.desc.g_ld == (12 if cin == 10 else 16)
    assert torch.equal(out.t[..., :C].cpu().double().reshape(N, S, C), ref["y64"]), "device logits are not the exact logits"
    # the fused launch on the recorded descriptor
    slots = nat.lib().ctseg_conv_logits_ce_slots(drv.desc, C)
    tiles = N * math.ceil(shape[1] / 4) * math.ceil(shape[2] / 8) * math.ceil(shape[3] / 8)
    assert slots == (min(tiles, int(max_wg)) if max_wg else tiles), (slots, tiles)
    labels = _dev(hc.labels.reshape(N, S))
    cw = _dev(ref["cw"])
    coef = torch.zeros(N, 1 + 3 * C)
    coef[:, 0] = ref["coef"]
    coef = _dev(coef)
    part = torch.full((N, slots, R), PART_SENTINEL, dtype=torch.float64, device=DEV)
    cnt = torch.zeros((N, 3, C), dtype=torch.int64, device=DEV)
    buf, dl_ptr = _guarded_rows(N * S, g_ld, dt, pad_state=0.0)
    nat.call("ctseg_conv_logits_ce", drv.desc, labels.data_ptr(), C, nat.ptr(cw), coef.data_ptr(), 1 + 3 * C, dl_ptr, g_ld, part.data_ptr(),
             slots, R, cnt.data_ptr())
    torch.cuda.synchronize()
    assert not bool((part == PART_SENTINEL).any()), "every workgroup writes a whole record for every sample"
    assert bool((part[..., 2:] == 0).all()), "entries 2 and up are 0"
    assert torch.equal(cnt.cpu(), ref["cnt"]), "Dice counts"
    red = _reduce(part, N, slots, R)
    torch.cuda.synchronize()
    _sum_ratio(tag + " (ce, weight) sums", red[:, :2], ref)
    got = buf[GUARD:-GUARD].float().cpu().double().reshape(N, S, g_ld)
    check_elems(tag + " gradient", got[..., :C], ref["g64"], ref["g32"], dt)
    if C < 12:
        assert float(got[..., C:12].abs().max()) == 0.0, "columns C to 11 are exactly 0"
    if g_ld == 16:
        assert float(got[..., 12:].abs().max()) == 0.0, "columns 12 to 15 keep the 0 the plan allocates them with"
    _check_guards(buf)
    # the two-pass kernel on the same device logits: same predictions, same counts
    _, cnt2, pred2 = _seg_loss(out.t, ld, labels, N, S, C, cw, 2, 1)
    assert torch.equal(pred2.cpu().long(), ref["pred"]), "ctseg_seg_loss predictions on the device logits"
    assert torch.equal(cnt2, cnt), "ctseg_seg_loss counts on the device logits"
    return part


@pytest.mark.parametrize("max_wg", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("case", HEAD_CASES, ids=HEAD_IDS)
def test_fused_head_cross_entropy_vs_float64(monkeypatch, case, max_wg):
    _fused_head(case, monkeypatch, max_wg)


@pytest.mark.parametrize("max_wg", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("case", HEAD_VARIANT_CASES, ids=HEAD_VARIANT_IDS)
def test_fused_head_cross_entropy_of_a_trained_head_vs_float64(monkeypatch, case, max_wg):
    """every bias 64 higher / a block that predicts class 0 with a lead of about 6 (loss_cases.py): the same checks"""
    _fused_head(case, monkeypatch, max_wg)


def test_fused_head_workgroups_without_tiles(monkeypatch):
    """9 tiles under CTSEG_MAX_WG = 8: workgroups 5, 6 and 7 have no tile and write zero records for every sample"""
    part = _fused_head(HEAD_EMPTY_WG_CASE, monkeypatch, "8")
    assert part.shape[1] == 8 and bool((part[:, 5:] == 0).all())
    assert bool((part[:, :5, 1].sum(0) > 0).all()), "workgroups 0 to 4 hold tiles"
