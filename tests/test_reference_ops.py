"""CPU: the float64 specification of the op-level GPU tests (reference_ops.py) against torch.autograd, and the shared bounds
(helpers.elem_bound / sum_bound) on inputs whose float32 error is known."""
import pytest
import torch
import torch.nn.functional as F

from capstone_amd._native import BF16, F32
from helpers import check_elems, elem_bound, sum_bound
from reference_ops import (boundary64, boundary_weights64, conv_dgrad, conv_fwd, conv_module, conv_out_shape, conv_wgrad, norm_prelu_dy,
                           norm_prelu_terms)

F64 = torch.float64
# an odd and an even extent per axis: stride 2 needs output_padding 1 for the even ones and 0 for the odd ones
X_SHAPES = {3: (2, 3, 5, 6, 7), 2: (1, 2, 4, 4)}
KINDS = ["conv", "conv_s2", "convT"]


def _layer(kind, k, dims, integers):
    """(x, w, b, gy) of a layer with 4 output channels, float64; ``integers``: small integer values (every sum exact)"""
    g = torch.Generator().manual_seed(100 * dims + 10 * k + KINDS.index(kind))
    xs = X_SHAPES[dims]
    mod = conv_module(kind, xs[1], 4, k, dims)
    ys = (xs[0], 4) + conv_out_shape(kind, k, xs[2:])

    def draw(shape):
        return torch.randint(-4, 5, shape, generator=g).double() if integers else torch.randn(shape, generator=g, dtype=F64)
    return draw(xs), draw(tuple(mod.weight.shape)), draw((4,)), draw(ys)


@pytest.mark.parametrize("integers", [False, True], ids=["normal", "integers"])
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_conv_gradients_equal_autograd(kind, k, dims, integers):
    x, w, b, gy = _layer(kind, k, dims, integers)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = conv_fwd(kind, k, xr, wr, br)
    assert tuple(y.shape) == tuple(gy.shape), "conv_out_shape"
    ax, aw, ab = torch.autograd.grad(y, (xr, wr, br), gy)
    with torch.no_grad():
        gx = conv_dgrad(kind, k, gy, w, x.shape)
    gw, gb = conv_wgrad(kind, k, x, gy, tuple(w.shape), F64)
    for what, got, want in (("input gradient", gx, ax), ("weight gradient", gw, aw), ("bias gradient", gb, ab)):
        assert got.shape == want.shape, what
        if integers:
            assert torch.equal(got, want), what
        else:       # float64 round-off of sums of at most a few hundred terms
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), what


# ---- norm + PReLU -------------------------------------------------------------------------------------------------------------
def _norm_case():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(2, 3, 4, 5, 3, generator=g, dtype=F64) * 1.3 + 0.4
    gy = torch.randn(2, 3, 4, 5, 3, generator=g, dtype=F64)
    gamma = torch.tensor([0.7, 2.0 ** -6, -0.75], dtype=F64)
    beta = torch.tensor([0.3, -0.2, 0.1], dtype=F64)
    return y, gy, gamma, beta


def test_instance_norm_prelu_dy_equals_autograd():
    y, gy, _, _ = _norm_case()
    yr = y.clone().requires_grad_(True)
    out = F.prelu(F.instance_norm(yr, eps=1e-5), torch.tensor([0.2], dtype=F64))
    want, = torch.autograd.grad(out, yr, gy)
    mean = y.mean((2, 3, 4), keepdim=True)
    rstd = (y.var((2, 3, 4), unbiased=False, keepdim=True) + 1e-5).rsqrt()
    xh, dz, terms = norm_prelu_terms(gy, y, mean, rstd, 0.2)
    assert bool((xh > 0).any()) and bool((xh < 0).any()), "both sides of the PReLU kink"
    got = norm_prelu_dy(gy, y, mean, rstd, 0.2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the three summed terms, written out
    slope = torch.where(xh > 0, torch.ones_like(xh), torch.full_like(xh, 0.2))
    assert torch.equal(dz, gy * slope) and torch.equal(terms[0], dz) and torch.equal(terms[1], gy * slope * xh)
    assert torch.equal(terms[2], gy * xh.clamp(max=0)), "g * min(xhat, 0)"
    # d alpha of the same expression is the sum of the third term
    al = torch.tensor([0.2], dtype=F64, requires_grad=True)
    da, = torch.autograd.grad(F.prelu(F.instance_norm(y, eps=1e-5), al), al, gy)
    assert abs(float(da) - float(terms[2].sum())) <= 1e-12 * float(terms[2].abs().sum())


def test_batch_norm_prelu_dy_equals_autograd():
    y, gy, gamma, beta = _norm_case()
    N, C = y.shape[:2]
    yr, gr, br = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    al = torch.tensor([0.2], dtype=F64, requires_grad=True)
    out = F.prelu(F.batch_norm(yr, None, None, gr, br, training=True, eps=1e-5), al)
    want, dgamma, dbeta, da = torch.autograd.grad(out, (yr, gr, br, al), gy)
    # the layout of the GPU tests: (N, C, S) rows, one set of statistics per channel over (0, 2)
    y3, g3 = y.reshape(N, C, -1), gy.reshape(N, C, -1)
    mean = y3.mean((0, 2), keepdim=True)
    rstd = (y3.var((0, 2), unbiased=False, keepdim=True) + 1e-5).rsqrt()
    ga, be = gamma.reshape(1, C, 1), beta.reshape(1, C, 1)
    xh, dz, terms = norm_prelu_terms(g3, y3, mean, rstd, 0.2, ga, be)
    pre = ga * xh + be
    assert bool((pre > 0).any()) and bool((pre < 0).any()), "both sides of the PReLU kink"
    got = norm_prelu_dy(g3, y3, mean, rstd, 0.2, ga, be, dims=(0, 2))
    assert float((got.reshape(y.shape) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(terms[2], g3 * pre.clamp(max=0)), "g * min(gamma * xhat + beta, 0)"
    for what, got_s, want_s, mag in (("d beta", terms[0].sum((0, 2)), dbeta, terms[0].abs().sum((0, 2))),
                                     ("d gamma", terms[1].sum((0, 2)), dgamma, terms[1].abs().sum((0, 2))),
                                     ("d alpha", terms[2].sum().reshape(1), da, terms[2].abs().sum().reshape(1))):
        assert bool(((got_s - want_s).abs() <= 1e-12 * mag).all()), what
    # per-sample statistics are another function
    assert not torch.allclose(got, norm_prelu_dy(g3, y3, mean, rstd, 0.2, ga, be, dims=(2,)))


# ---- Boundary loss ------------------------------------------------------------------------------------------------------------
def test_boundary64_does_not_depend_on_the_rank():
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 3, 5, 6, 7
    logits = torch.randn(B, C, H, W, generator=g) * 2
    D = torch.rand(B, C - 1, H, W, generator=g) * 2 - 1
    Wt = torch.randn(B, C - 1, generator=g).double()
    perm = torch.tensor([2, 0, 0])
    sides = [(D, 0.3 * Wt), (D[perm], 0.7 * Wt[perm])]
    v2, m2, g2, a2 = boundary64(logits, sides)
    v3, m3, g3, a3 = boundary64(logits.unsqueeze(2), [(d.unsqueeze(2), w) for d, w in sides])
    assert v2 == v3 and m2 == m3 and m2 > abs(v2) > 0
    assert torch.equal(g3.squeeze(2), g2) and torch.equal(a3.squeeze(2), a2) and float(g2.abs().max()) > 0
    # the gradient is p_k (g_k - sum_j g_j p_j): bounded by the magnitude term the tests scale their bounds with
    assert bool((g2.abs() <= 2 * a2 + 1e-18).all())


def test_boundary_weights64():
    B, K = 2, 4
    ind = torch.ones(B, K)
    assert torch.equal(boundary_weights64(ind, False, B, K), torch.full((B, K), 1.0 / 8, dtype=F64))
    ind[1, 2] = 0
    w = boundary_weights64(ind, True, B, K)          # 1 / count per class, normalised over the classes, / B
    per_class = torch.tensor([0.5, 0.5, 1.0, 0.5], dtype=F64)
    assert torch.equal(w, (per_class / per_class.sum())[None, :] * ind.double() / B)
    ind[:, 0] = 0                                    # a class missing everywhere: 1 / 0 = inf -> all class weights one
    w = boundary_weights64(ind, True, B, K)
    assert torch.equal(w, torch.full((K,), 0.25, dtype=F64)[None, :] * ind.double() / B)
    assert float(w[:, 0].abs().max()) == 0.0


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def test_sum_bound_on_a_sum_float32_cannot_hold():
    """column 0: 2^24 followed by eight ones: every float32 partial sum rounds back to 2^24 (ties to even), the float32 sum is 8 short
    whether torch adds in sequence or in pairs of blocks.  Column 1: all zeros (a dead channel).  Column 2: exact in float32."""
    t64 = torch.zeros(9, 3, dtype=F64)
    t64[0, 0], t64[1:, 0] = 2.0 ** 24, 1.0
    t64[:, 2] = torch.arange(9, dtype=F64)
    t32 = t64.float()
    f32 = abs(float(t32[:, 0].sum()) - (2.0 ** 24 + 8)) / (2.0 ** 24 + 8)
    assert f32 > 0
    s64, norm, live, bound = sum_bound("hand-made", t64.t(), t32.t(), (1,), rows=9)
    assert live.tolist() == [True, False, True]
    assert s64.tolist() == [2.0 ** 24 + 8, 0.0, 36.0] and norm.tolist() == [2.0 ** 24 + 8, 1.0, 36.0]
    assert bound == 16.0 * f32
    # the same figures under a row count whose cap 1 / (4 * rows) the bound does not stay under
    rows = int(1.0 / (4.0 * bound)) + 1
    with pytest.raises(AssertionError):
        sum_bound("too many rows", t64.t(), t32.t(), (1,), rows=rows)
    # sum / div as the kernel stores it
    assert sum_bound("mean", t64.t(), t32.t(), (1,), rows=9, div=9.0)[3] > 0
    # a float32 evaluation without error gives no bound: the assertion 0 < bound fires
    with pytest.raises(AssertionError):
        sum_bound("exact", t64[:, 2:].t(), t32[:, 2:].t(), (1,), rows=9)


def test_elem_bound_and_check_elems():
    ref64 = torch.tensor([1.0, -3.0, 0.1], dtype=F64)
    ref32 = ref64.float()                            # 0.1 is no float32 value: e32 = |float32(0.1) - 0.1|
    e32 = abs(float(torch.tensor(0.1, dtype=torch.float32)) - 0.1)
    bound, e = elem_bound(ref64, ref32, BF16)
    assert e == e32 > 0 and torch.equal(bound, 2.0 ** -8 * ref64.abs() + 16.0 * e32)
    bound32, _ = elem_bound(ref64, ref32, F32)
    assert torch.equal(bound32, torch.full_like(ref64, 16.0 * e32))
    assert check_elems("inside", ref64 + 0.5 * bound, ref64, ref32, BF16) <= 1.0
    with pytest.raises(AssertionError):
        check_elems("one element outside", ref64 + torch.tensor([0.0, 0.0, 1.5]) * bound, ref64, ref32, BF16)
    with pytest.raises(AssertionError):
        elem_bound(ref64[:2], ref32[:2], BF16)       # an exact float32 evaluation measures nothing
