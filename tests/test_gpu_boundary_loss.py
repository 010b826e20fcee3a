"""GPU: the Boundary loss on the MI355X — ctseg_boundary_stats / ctseg_boundary_grad at op level, then MultipleLossWrapper(...,
device_boundary=True), LossEntry("Boundary", ...), forward_mixed and the two 2-D trainers.

The comparison target is the reference's formula (capstone/models/losses.py:139-148) restated in float64 torch on the CPU (boundary64 /
boundary_weights64 of reference_ops.py):
    p = softmax(x, 1);  T[b, c] = (1 / S) sum_v p[b, c + 1, v] D[b, c, v];  "mean": T.mean();  exclude_missing: the non-Focal branch
    of apply_missing_mask;  gradient d_k = p_k (g_k - sum_j g_j p_j), g_0 = 0, g_c = W[b, c - 1] D[b, c - 1] with W = weight of the
    table entry in the scalar / S;  mixup: g_c = W0 D[b] + W1 D[perm[b]].

Bounds (stated before any run, from the arithmetic):
  * statistics: |T - T64| <= 2^-20 * (1 / S) sum_v |p D|.  The fp32 softmax is a few ulp off per voxel, a thread adds at most 9
    products in fp32 (2048 voxels per workgroup at most, 256 threads), everything after that is fp64.
  * gradient (fp32 rows): |d - d64| <= 2^-19 * sum_j |g_j| p_j + 2^-22 * |d64|.  The first term is the rounding of the products,
    of the dot product and of the cancelling difference g_k - dot, all of size <= sum_j |g_j| p_j; the second the final product.
  * accumulate = 1 into fp32 rows: one fp32 add of the stored value and the value accumulate = 0 stores -> within 1 ulp of that
    sum.  Into bf16 rows: the bf16 rounding (nearest even) of that fp32 sum, bit for bit.
  * a scalar loss value: 2^-18 * sum_bc w_bc (1 / S) sum_v |p D|: the table's 2^-20, its cast to fp32 (2^-24), the fp32 weights
    (2^-23) and an fp32 sum of at most 42 terms (< 2^-18.6 of the sum of magnitudes).

The trainer step runs filters [4, 8, 8, 8, 8] in fp32 storage; 16-bit storage takes channel counts that are multiples of 8 only
(capstone_amd.plan refuses others), so the bf16 case runs [8, 8, 8, 8, 8], the smallest network it accepts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd import segloss  # noqa: E402
from capstone_amd._native import BF16, F32  # noqa: E402
from helpers import ulp32  # noqa: E402
from reference_ops import boundary64, boundary_weights64, softmax64  # noqa: E402

DEV = "cuda:0"
B = 3
PERM = [2, 0, 0]                 # no bijection (0 drawn twice, 1 never), no fixed point
H, W = 47, 45                    # S = 2115: two workgroups per sample, a ragged second range, odd plane stride
SHAPES = {"C10-ld12": (10, 12, H, W), "C5-ld8": (5, 8, H, W), "C14-ld16": (14, 16, H, W), "C10-S7": (10, 12, 7, 1)}
_CASE = {}


def _case(key):
    """inputs and the float64 reference of one shape, computed once and shared; nothing in it is modified afterwards"""
    if key in _CASE:
        return _CASE[key]
    C, ld, h, w = SHAPES[key]
    S = h * w
    g = torch.Generator().manual_seed(1000 + 17 * C + S)
    x = torch.zeros(B, S, ld)
    x[..., :C] = (torch.rand(B, S, C, generator=g) * 2 - 1) * 8                      # logits spread over +-8
    D = torch.rand(B, C - 1, S, generator=g) * 2 - 1                                 # both signs (signed=True); [0, 1] is inside
    bw = (torch.rand(B, 2, C - 1, generator=g) * 2 - 1) * 1e-3
    perm = torch.tensor(PERM)
    p = softmax64(x[..., :C])                                                        # (B, S, C)
    pf = p[..., 1:].permute(0, 2, 1)                                                  # (B, C-1, S)
    sides = [D.double(), D[perm].double()]
    T = torch.stack([(pf * Ds).sum(-1) / S for Ds in sides], 1)                       # (B, 2, C-1)
    Tabs = torch.stack([(pf * Ds).abs().sum(-1) / S for Ds in sides], 1)
    ref = {}
    for ns in (1, 2):
        gk = torch.zeros(B, S, C, dtype=torch.float64)
        for s in range(ns):
            gk[..., 1:] += (bw[:, s].double()[:, :, None] * sides[s]).permute(0, 2, 1)
        d = p * (gk - (gk * p).sum(-1, keepdim=True))
        ref[ns] = (d, (gk.abs() * p).sum(-1, keepdim=True))
    xd, Dd = x.to(DEV), D.to(DEV)
    _CASE[key] = dict(C=C, ld=ld, S=S, h=h, w=w, x=x, xd=xd, D=D, Dd=Dd, bw=bw, T=T, Tabs=Tabs, ref=ref, r0={})
    return _CASE[key]


def _engine(case, ns):
    """the engine's Boundary calls at op level.  The two-sided form is put on the base engine here (SegLossPairEngine's label
    tables stop at 10 classes; the Boundary passes do not): the same native calls with NS = 2 and a device perm"""
    C, S = case["C"], case["S"]
    eng = segloss.SegLossEngine(torch.device(DEV), B, S, C)
    if ns == 2:
        eng.NS, eng.perm = 2, torch.tensor(PERM, dtype=torch.int32, device=DEV)
        eng._boundary_perm = lambda: eng.perm
    eng.set_dist_maps(case["Dd"].view(B, C - 1, case["h"], case["w"]))
    eng.bw.copy_(case["bw"][:, :ns].to(DEV))
    return eng


def _grad_f32(case, ns):
    """the accumulate = 0 result in fp32 rows of the logits' own width (shared by the accumulate tests)"""
    if ns not in case["r0"]:
        eng = _engine(case, ns)
        dl = torch.full((B, case["S"], case["ld"]), 7.0, device=DEV)
        eng.boundary_grad(case["xd"].data_ptr(), case["ld"], dl.data_ptr(), case["ld"], F32, accumulate=False)
        case["r0"][ns] = dl.cpu()
    return case["r0"][ns]


@pytest.mark.parametrize("ns", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("key", list(SHAPES))
def test_statistics_vs_float64_and_bit_identical_twice(key, ns):
    case = _case(key)
    eng = _engine(case, ns)
    assert eng.P == (2 if case["S"] == 2115 else 1)
    eng.boundary_stats(case["xd"].data_ptr(), case["ld"])
    first_part, first = eng.b_part.clone(), eng.b_red.clone()
    eng.b_part.fill_(-1.0)
    eng.boundary_stats(case["xd"].data_ptr(), case["ld"])
    assert torch.equal(eng.b_part, first_part) and torch.equal(eng.b_red, first)       # no atomics: the same bits
    got = first.cpu() / case["S"]
    err = (got - case["T"][:, :ns]).abs()
    bound = 2.0 ** -20 * case["Tabs"][:, :ns]
    print(f"boundary stats {key} ns={ns}: worst error / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("ns", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("key", list(SHAPES))
def test_gradient_fp32_rows_vs_float64(key, ns):
    case = _case(key)
    C = case["C"]
    got = _grad_f32(case, ns).double()
    ref, gabs = case["ref"][ns]
    err = (got[..., :C] - ref).abs()
    bound = 2.0 ** -19 * gabs + 2.0 ** -22 * ref.abs()
    print(f"boundary gradient {key} ns={ns}: worst error / bound = {float((err / bound).max()):.3e}, max |ref| = {float(ref.abs().max()):.3e}")
    assert bool((err <= bound).all())
    assert float(ref.abs().max()) > 0 and float(ref[..., 0].abs().max()) > 0           # the background logit gets a gradient
    assert case["ld"] > C and float(got[..., C:].abs().max()) == 0.0                   # pad columns written as zeros (over the 7.0)


@pytest.mark.parametrize("ns", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("key", list(SHAPES))
def test_accumulate_into_fp32_rows(key, ns):
    case = _case(key)
    C, ld, S = case["C"], case["ld"], case["S"]
    r0 = _grad_f32(case, ns)
    buf0 = torch.randn(B, S, ld, generator=torch.Generator().manual_seed(3)) * 1e-3
    dl = buf0.to(DEV)
    _engine(case, ns).boundary_grad(case["xd"].data_ptr(), ld, dl.data_ptr(), ld, F32, accumulate=True)
    got = dl.cpu()
    s = buf0[..., :C].double() + r0[..., :C].double()
    assert bool(((got[..., :C].double() - s).abs() <= ulp32(s)).all())
    assert torch.equal(got[..., C:], buf0[..., C:])                                    # pad columns unchanged


BF16_ROWS = [("C10-ld12", 12), ("C10-ld12", 16), ("C5-ld8", 8), ("C5-ld8", 12), ("C14-ld16", 16), ("C10-S7", 12)]


@pytest.mark.parametrize("ns", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("key,g_ld", BF16_ROWS, ids=[f"{k}-g{g}" for k, g in BF16_ROWS])
def test_bf16_rows_store_and_accumulate_bit_exact(key, g_ld, ns):
    """the fp32 value both variants form is the accumulate = 0 fp32 result itself (the same expressions): the stored row is its bf16
    rounding, the accumulated row the bf16 rounding of fp32(stored bf16 + that value)"""
    case = _case(key)
    C, ld, S = case["C"], case["ld"], case["S"]
    r0 = torch.zeros(B, S, g_ld)
    r0[..., :C] = _grad_f32(case, ns)[..., :C]
    eng = _engine(case, ns)
    dl = torch.full((B, S, g_ld), 7.0, dtype=torch.bfloat16, device=DEV)
    eng.boundary_grad(case["xd"].data_ptr(), ld, dl.data_ptr(), g_ld, BF16, accumulate=False)
    assert torch.equal(dl.cpu(), r0.to(torch.bfloat16))                                # (zeros in the pad columns)
    buf0 = (torch.randn(B, S, g_ld, generator=torch.Generator().manual_seed(4)) * 1e-3).to(torch.bfloat16)
    dl = buf0.to(DEV)
    eng.boundary_grad(case["xd"].data_ptr(), ld, dl.data_ptr(), g_ld, BF16, accumulate=True)
    want = (buf0.float() + r0).to(torch.bfloat16)
    got = dl.cpu()
    assert torch.equal(got[..., :C], want[..., :C])
    assert torch.equal(got[..., C:].view(torch.int16), buf0[..., C:].view(torch.int16))  # pad columns: the same bits


def test_exact_integer_case():
    """all-equal logits: p = 1/4 exactly with C = 4; small-integer maps and weights: every sum is exact in fp32, so the statistics
    and the gradient equal the float64 values"""
    C, ld, S = 4, 4, H * W
    g = torch.Generator().manual_seed(11)
    x = torch.full((B, S, ld), 3.0)
    D = torch.randint(-3, 4, (B, C - 1, S), generator=g).float()
    bw = torch.randint(-2, 3, (B, 2, C - 1), generator=g).float()
    perm = torch.tensor(PERM)
    eng = segloss.SegLossPairEngine(torch.device(DEV), B, S, C)
    eng.perm = perm.to(torch.int32).to(DEV)
    eng.set_dist_maps(D.view(B, C - 1, H, W).to(DEV))
    eng.bw.copy_(bw.to(DEV))
    xd = x.to(DEV)
    eng.boundary_stats(xd.data_ptr(), ld)
    want = torch.stack([0.25 * D.double().sum(-1), 0.25 * D[perm].double().sum(-1)], 1)
    assert torch.equal(eng.b_red.cpu(), want)
    dl = torch.full((B, S, ld), 7.0, device=DEV)
    eng.boundary_grad(xd.data_ptr(), ld, dl.data_ptr(), ld, F32, accumulate=False)
    gk = torch.zeros(B, S, C, dtype=torch.float64)
    gk[..., 1:] = (bw[:, 0].double()[:, :, None] * D.double() + bw[:, 1].double()[:, :, None] * D[perm].double()).permute(0, 2, 1)
    d = 0.25 * (gk - 0.25 * gk.sum(-1, keepdim=True))
    assert torch.equal(dl.cpu().double(), d) and float(d.abs().max()) > 0


# ---- the loss surface ---------------------------------------------------------------------------------------------------------
def _surface_inputs(seed=7, C=10):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g) * 2
    target = torch.randint(0, C, (B, H, W), generator=g)
    D = torch.rand(B, C - 1, H, W, generator=g) * 2 - 1
    return logits, target, D


@pytest.mark.parametrize("exclude_missing", [False, True])
def test_wrapper_on_a_foreign_tensor(exclude_missing):
    from capstone_amd.models.losses import MultipleLossWrapper
    logits, target, D = _surface_inputs()
    ind = torch.ones(B, 9)
    ind[1, 3] = 0
    ind[:, 6] = 0                                # a zero column: 1 / 0 -> the isinf branch (used under exclude_missing only)
    Wt = boundary_weights64(ind, exclude_missing, B, 9)
    val, mag, gb, gabs = boundary64(logits, [(D, Wt)])
    old = MultipleLossWrapper(["Dice", "Focal"], exclude_missing=exclude_missing)
    xo = logits.to(DEV).requires_grad_(True)
    vo = old(xo, target.to(DEV), mask_indicator=ind.to(DEV))
    torch.stack(list(vo.values())).sum().backward()
    wrap = MultipleLossWrapper(["Boundary", "Dice", "Focal"], exclude_missing=exclude_missing, device_boundary=True)
    x = logits.to(DEV).requires_grad_(True)
    v = wrap(x, target.to(DEV), mask_indicator=ind.to(DEV), dist_maps=D.to(DEV))
    assert list(v) == ["Boundary", "Dice", "Focal"]
    print(f"Boundary value {v['Boundary'].item():.9g} vs {val:.9g}, magnitude {mag:.3e}")
    assert abs(v["Boundary"].item() - val) <= 2.0 ** -18 * mag
    assert v["Dice"].item() == vo["Dice"].item() and v["Focal"].item() == vo["Focal"].item()
    torch.stack(list(v.values())).sum().backward()
    total = xo.grad.cpu().double() + gb
    err = (x.grad.cpu().double() - total).abs()
    bound = 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs() + 2.0 ** -23 * total.abs()      # (+ the one fp32 add of the two gradients)
    print(f"wrapper gradient: worst error / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    # Boundary alone: the storing variant, no label pass
    x1 = logits.to(DEV).requires_grad_(True)
    only = MultipleLossWrapper(["Boundary"], exclude_missing=exclude_missing, device_boundary=True)
    v1 = only(x1, target.to(DEV), mask_indicator=ind.to(DEV), dist_maps=D.to(DEV).double())["Boundary"]
    assert v1.item() == v["Boundary"].item()
    v1.backward()
    err = (x1.grad.cpu().double() - gb).abs()
    assert bool((err <= 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs()).all())
    with pytest.raises(TypeError):
        only(x1, target.to(DEV), dist_maps=D.to(DEV).to(torch.int32))
    with pytest.raises(nat.NativeError):
        only(x1, target.to(DEV), dist_maps=D)                                          # maps on the host


def test_unreduced_entry_and_forward_mixed():
    from capstone_amd.models.losses import LossEntry, MultipleLossWrapper
    logits, target, D = _surface_inputs(seed=8)
    gT = torch.randn(B, 9, generator=torch.Generator().manual_seed(9))
    val, mag, gb, gabs = boundary64(logits, [(D, gT.double())])
    x = logits.to(DEV).requires_grad_(True)
    T = LossEntry("Boundary", "none")(x, D.to(DEV))
    assert T.shape == (B, 9) and T.dtype == torch.float32
    p = torch.softmax(logits.double(), dim=1)[:, 1:] * D.double()
    T64, Tabs = p.mean(dim=(2, 3)), p.abs().mean(dim=(2, 3))
    assert bool(((T.cpu().double() - T64).abs() <= 2.0 ** -20 * Tabs + 2.0 ** -24 * T64.abs()).all())
    (T * gT.to(DEV)).sum().backward()
    err = (x.grad.cpu().double() - gb).abs()
    assert bool((err <= 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs()).all())
    m = LossEntry("Boundary", "mean")(logits.to(DEV), D.to(DEV))
    assert abs(m.item() - T64.mean().item()) <= 2.0 ** -18 * Tabs.mean().item()

    # forward_mixed: lambda * A + (1 - lambda) * B of two single-target evaluations, each side under its own indicator
    index, lam = torch.tensor(PERM), 0.3
    ind = torch.ones(B, 9)
    ind[2, 4] = 0                                # sample 0's partner is sample 2: their indicators differ; sample 1's is sample 0
    ind[1, 1] = 0
    for exclude_missing in (False, True):
        sides = [(D, lam * boundary_weights64(ind, exclude_missing, B, 9)), (D[index], (1 - lam) * boundary_weights64(ind[index], exclude_missing, B, 9))]
        val, mag, gb, gabs = boundary64(logits, sides)
        old = MultipleLossWrapper(["Dice"], exclude_missing=exclude_missing)
        xo = logits.to(DEV).requires_grad_(True)
        vo = old.forward_mixed(xo, target.to(DEV), index.to(DEV), lam, mask_indicator=ind.to(DEV))
        vo["Dice"].backward()
        wrap = MultipleLossWrapper(["Boundary", "Dice"], exclude_missing=exclude_missing, device_boundary=True)
        x = logits.to(DEV).requires_grad_(True)
        v = wrap.forward_mixed(x, target.to(DEV), index.to(DEV), lam, mask_indicator=ind.to(DEV), dist_maps=D.to(DEV))
        print(f"mixed Boundary value {v['Boundary'].item():.9g} vs {val:.9g}, magnitude {mag:.3e}")
        assert abs(v["Boundary"].item() - val) <= 2.0 ** -18 * mag
        assert v["Dice"].item() == vo["Dice"].item()
        torch.stack(list(v.values())).sum().backward()
        total = xo.grad.cpu().double() + gb
        err = (x.grad.cpu().double() - total).abs()
        bound = 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs() + 2.0 ** -23 * total.abs()
        print(f"forward_mixed gradient: worst error / bound = {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all())


# ---- the trainers -------------------------------------------------------------------------------------------------------------
def _batch():
    g = torch.Generator().manual_seed(12)
    images = torch.randn(2, 1, 32, 32, generator=g)
    masks = torch.zeros(2, 9, 32, 32, dtype=torch.uint8)
    for b in range(2):
        for k in range(9):
            masks[b, k, 3 * k + 2:3 * k + 5, 4 + 2 * b:28] = 1
    D = torch.rand(2, 9, 32, 32, generator=g) * 2 - 1
    return images, masks, torch.ones(2, 9), D


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("mixup", [False, True], ids=["BaseUNet2D", "MixupUNet2D"])
def test_trainer_step_with_the_boundary_loss(monkeypatch, mixup, precision):
    from capstone_amd.training import mixup_trainer as MT
    from capstone_amd.training.base_trainer import BaseUNet2D
    from capstone_amd.training.utils import weighted_mixup
    cls = MT.MixupUNet2D if mixup else BaseUNet2D
    # 16-bit storage needs channel counts that are multiples of 8 (capstone_amd.plan): the smallest such network there
    filters = [4, 8, 8, 8, 8] if precision == "fp32" else [8, 8, 8, 8, 8]
    images, masks, ind, D = _batch()
    index, lam = torch.tensor([1, 0]), 0.3
    monkeypatch.setattr(MT, "weighted_mixup", functools.partial(weighted_mixup, index=index.to(DEV), lambda_=lam))
    torch.manual_seed(5)
    m = cls(filters=list(filters), loss_fx=["Boundary", "Dice"], transform_degree=0, device_boundary=True, precision=precision)
    m.to(DEV)
    seen, fwd = {}, m.forward

    def recording_forward(x_):
        seen["y"] = fwd(x_)
        return seen["y"]
    m.forward = recording_forward
    batch3 = (images.to(DEV), masks.to(DEV), ind.to(DEV))
    loss = m.training_step(batch3 + (D.to(DEV),))
    loss.backward()
    assert "Boundary Loss (train)" in m.logged and "Dice Loss (train)" in m.logged
    y = seen["y"].detach().float().cpu()
    Wm = torch.full((2, 9), 1.0 / 18, dtype=torch.float64)
    sides = [(D, lam * Wm), (D[index], (1 - lam) * Wm)] if mixup else [(D, Wm)]
    p = torch.softmax(y.double(), dim=1)[:, 1:]
    val = sum(((p * Ds.double()).mean(dim=(2, 3)) * Wt).sum().item() for Ds, Wt in sides)
    mag = sum(((p * Ds.double()).abs().mean(dim=(2, 3)) * Wt).sum().item() for Ds, Wt in sides)
    got = m.logged["Boundary Loss (train)"].item()
    print(f"trainer Boundary value {got:.9g} vs {val:.9g}, magnitude {mag:.3e}")
    assert abs(got - val) <= 2.0 ** -18 * mag
    np.testing.assert_allclose(loss.item(), got + m.logged["Dice Loss (train)"].item(), rtol=1e-6)
    grads = [q.grad.detach().float().cpu().clone() for q in m.unet.parameters()]
    assert all(bool(torch.isfinite(g_).all()) for g_ in grads) and sum(float(g_.abs().max()) > 0 for g_ in grads) >= len(grads) // 2
    # the same network (same seed, same initial weights) under ["Dice"] alone: other gradients
    torch.manual_seed(5)
    d = cls(filters=list(filters), loss_fx=["Dice"], transform_degree=0, precision=precision)
    d.to(DEV)
    assert all(torch.equal(a, b) for a, b in zip(m.unet.state_dict().values(), d.unet.state_dict().values()))
    d.training_step(batch3).backward()
    other = [q.grad.detach().float().cpu() for q in d.unet.parameters()]
    assert any(not torch.equal(a, b) for a, b in zip(grads, other))
    with pytest.raises(NotImplementedError):
        d.training_step(batch3 + (D.to(DEV),))                                         # flag off: a 4-tuple batch raises as before
    if not mixup:
        with torch.no_grad():
            m.validation_step(batch3 + (D.to(DEV),))
            m.test_step(batch3 + (D.to(DEV),))
        assert "Boundary Loss (val)" in m.logged and "Boundary Loss (test)" in m.logged
