"""CPU: the float64 specification of the op-level GPU tests (reference_ops.py) against torch.autograd, and the shared bounds
(helpers.elem_bound / sum_bound) on inputs whose float32 error is known."""
import pytest
import torch
import torch.nn.functional as F

from capstone_amd._native import BF16, F32
from helpers import check_elems, elem_bound, sum_bound
from loss_cases import (HEAD_CASES, HEAD_EMPTY_WG_CASE, HEAD_IDS, HEAD_LOSS_SCALE, HEAD_VARIANT_CASES, HEAD_VARIANT_IDS, PAD_LOGIT, SAT_BIG,
                        SAT_EQUAL_ROW, SAT_RIGHT_ROW, SAT_WRONG_ROWS, SEG_REGIME_SHAPES, SEG_REGIMES, SEG_S, SEG_SHAPES, SEG_SHIFT, head_case,
                        head_reference, partials_case, partials_reference, seg_class_weight, seg_loss_case, seg_stats_reference, top_margin)
from reference_ops import (boundary64, boundary_weights64, conv_dgrad, conv_fwd, conv_module, conv_out_shape, conv_wgrad, dice_count_table,
                           first_max_index, norm_prelu_dy, norm_prelu_terms, seg_loss_grad, seg_loss_records, seg_loss_terms)

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


# ---- label losses -------------------------------------------------------------------------------------------------------------
def _loss_inputs(C=5, B=2, S=37):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, S, C, generator=g, dtype=F64) * 2
    labels = torch.randint(0, C, (B, S), generator=g)
    cw = torch.rand(C, generator=g, dtype=F64) + 0.1
    return x, labels, cw


def test_seg_loss_terms_equal_cross_entropy_and_the_written_out_sums():
    C = 5
    x, labels, cw = _loss_inputs(C)
    flat, lab = x.reshape(-1, C), labels.reshape(-1)
    for w in (None, cw):
        t = seg_loss_terms(x, labels, C, w)
        want_sum = F.cross_entropy(flat, lab, weight=w, reduction="sum")
        want_mean = F.cross_entropy(flat, lab, weight=w)
        assert abs(float(t["ce"].sum() - want_sum)) <= 1e-12 * float(want_sum)
        assert abs(float(t["ce"].sum() / t["w"].sum() - want_mean)) <= 1e-12 * float(want_mean), "the mean divides by the weight sum"
        assert torch.equal(t["w"], torch.ones_like(t["w"]) if w is None else w[labels])
    t = seg_loss_terms(x, labels, C)
    p = torch.softmax(x, -1)
    oh = F.one_hot(labels, C).double()
    pt = p.gather(-1, labels[..., None])[..., 0]
    assert torch.equal(t["p"], p) and torch.equal(t["py"], p * oh)
    assert float((t["py"].sum(-1) - pt).abs().max()) == 0.0
    fo = (1 - pt) ** 2 * -torch.log(pt)
    assert float((t["fo"].sum(-1) - fo).abs().max()) <= 1e-14 and bool(((t["fo"] != 0) <= (oh == 1)).all()), "focal term at the label's class"
    rec = seg_loss_records(t)
    assert rec.shape[-1] == 2 + 3 * C and torch.equal(rec[..., 0], t["ce"]) and torch.equal(rec[..., 2 + C:2 + 2 * C], t["py"])
    assert float(seg_loss_records(t, ce_only=True)[..., 2:].abs().max()) == 0.0
    # a wider row: the columns from C on are not read
    wide = torch.cat([x, torch.full_like(x[..., :3], 64.0)], -1)
    assert torch.equal(seg_loss_terms(wide, labels, C)["ce"], t["ce"])


def test_prediction_is_the_first_maximal_index_and_the_counts_follow_it():
    x = torch.tensor([[[0.0, 1.0, 1.0, -1.0], [2.0, 2.0, 2.0, 0.0], [0.5, -1.0, 0.25, 0.5], [0.0, 0.0, 0.0, 3.0]]], dtype=F64)
    labels = torch.tensor([[1, 0, 3, 3]])
    t = seg_loss_terms(x, labels, 4)
    assert t["pred"].tolist() == [[1, 0, 0, 3]]
    assert torch.equal(first_max_index(x), t["pred"])
    #                         intersection   predicted      truth
    assert t["cnt"].tolist() == [[[1, 1, 0, 1], [2, 1, 0, 1], [1, 1, 0, 2]]]
    # labels outside the classes count nowhere
    got = dice_count_table(torch.tensor([[0, 255, 4, 1]]), torch.tensor([[0, 255, 1, 4]]), 4)
    assert got.tolist() == [[[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0]]]


def test_seg_loss_grad_equals_autograd_of_cross_entropy_and_the_closed_form():
    C = 5
    x, labels, cw = _loss_inputs(C)
    B = x.shape[0]
    g = torch.Generator().manual_seed(12)
    # cross-entropy alone: coefficient row (s, 0 ...)
    coef = torch.zeros(B, 1 + 3 * C, dtype=F64)
    coef[:, 0] = torch.tensor([0.25, 3.0], dtype=F64)
    got = seg_loss_grad(x, labels, C, coef, cw)
    xr = x.clone().requires_grad_(True)
    L = sum(coef[b, 0] * F.cross_entropy(xr[b], labels[b], weight=cw, reduction="sum") for b in range(B))
    want, = torch.autograd.grad(L, xr)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # the full row against the derivative written out: s w (p - 1) + p (g - <g, p>) + f (2 (1 - p_t) p_t log p_t - (1 - p_t)^2)(1 - p)
    coef[:, 1:] = torch.randn(B, 3 * C, generator=g, dtype=F64)
    got = seg_loss_grad(x, labels, C, coef, cw)
    p = torch.softmax(x, -1)
    oh = F.one_hot(labels, C).double()
    pt = (p * oh).sum(-1, keepdim=True)
    a, b_, f = coef[:, None, 1:1 + C], coef[:, None, 1 + C:1 + 2 * C], coef[:, None, 1 + 2 * C:]
    gk = a * oh + b_
    ft = (f * oh).sum(-1, keepdim=True)
    fterm = ft * (2 * (1 - pt) * pt * torch.log(pt) - (1 - pt) ** 2)
    want = coef[:, None, :1] * cw[labels][..., None] * (p - oh) + p * (gk - (gk * p).sum(-1, keepdim=True)) + fterm * (oh - p)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert got.dtype == F64 and seg_loss_grad(x.float(), labels, C, coef, cw).dtype == torch.float32, "the precision of x"


@pytest.mark.parametrize("C,ld,S", [(C, ld, S) for C, ld in SEG_SHAPES for S in SEG_S] + [(10, 12, 10)])      # S = 10: the direct call
def test_seg_loss_case_preconditions(C, ld, S):
    _seg_case_preconditions(C, ld, S, "initial")


@pytest.mark.parametrize("regime", SEG_REGIMES)
@pytest.mark.parametrize("C,ld,S", [(C, ld, S) for C, ld in SEG_REGIME_SHAPES for S in SEG_S])
def test_seg_loss_regime_preconditions(C, ld, S, regime):
    """the promises of the initial draw hold in every regime, and each regime is in the state its name says"""
    _seg_case_preconditions(C, ld, S, regime)
    base, case = seg_loss_case(C, ld, S), seg_loss_case(C, ld, S, regime=regime)
    for k in ("labels", "coef", "cw"):
        assert torch.equal(case[k], base[k]), k
    assert case["tie_rows"] == base["tie_rows"]
    x, labels = case["x"][..., :C], case["labels"].long()
    assert bool((case["x"][..., C:] == PAD_LOGIT).all())
    if regime in SEG_SHIFT:
        # x is float32: the shifted logit IS a float32 number; that the addition did not round is what is asserted
        assert torch.equal(x.double(), base["x"][..., :C].double() + SEG_SHIFT[regime]), "the offset is exact"
        return
    lead_ok = case["label_leads"]
    tie = torch.zeros(S, dtype=torch.bool)
    tie[[r for r, _ in case["tie_rows"]]] = True
    special = tie.clone()
    if regime == "saturated":
        special[4:9] = True
    body = ~special[None, :].expand_as(lead_ok)
    share = float(lead_ok[body].float().mean())
    assert (0.95 if S > 1000 else 0.80) <= share <= 0.98, share
    top = x.double().topk(2, dim=-1).values
    lead = top[..., 0] - top[..., 1]
    t64 = seg_loss_terms(x.double(), labels, C)
    t32 = seg_loss_terms(x, labels, C)
    right, wrong = body & lead_ok, body & ~lead_ok
    assert torch.equal(t64["pred"][right], labels[right]) and bool((t64["pred"][wrong] != labels[wrong]).all())
    hist_wrong = F.one_hot(labels, C) * wrong[..., None]
    assert bool(((hist_wrong.sum(1) > 0) | (F.one_hot(labels, C).sum(1) == 0)).all()), "a wrong voxel for every class of a sample's labels"
    pt32 = t32["py"].sum(-1)
    rows_wrong = list(SAT_WRONG_ROWS)
    if regime == "confident":
        assert 6.0 <= float(lead[body].min()) and float(lead[body].max()) <= 10.0
        assert float(t64["ce"][right].median()) < 2e-3 and float(t64["ce"][right].max()) < 9 * 2.5e-3
        # the lead over the largest other logit, plus what the label's logit lies below that one
        assert 6.0 < float(t64["ce"][wrong].min()) and float(t64["ce"][wrong].median()) < 13.0 and float(t64["ce"][wrong].max()) < 30.0
        assert bool((pt32[right] < 1.0).all())
    else:
        assert 30.0 <= float(lead[body].min()) and float(lead[body].max()) <= 124.0
        e32 = torch.exp(-lead[body].float())
        tiny = float(torch.finfo(torch.float32).tiny)
        assert bool(((e32 > 1e-20) & (e32 < 2.0 ** -23)).any()) and bool(((e32 > tiny) & (e32 < 1e-20)).any())
        assert bool(((e32 > 0) & (e32 < tiny)).any()) and bool((e32 == 0).any()), "below epsilon, a subnormal, 0"
        assert bool((pt32[lead_ok] == 1.0).all()), "the label's probability is exactly 1.0 in float32"
        assert bool(lead_ok[:, SAT_RIGHT_ROW].all()) and not bool(lead_ok[:, [4] + rows_wrong].any())
        rows = rows_wrong
        assert bool((x[:, rows].max(-1).values == SAT_BIG).all()) and bool((t64["pred"][:, rows] != labels[:, rows]).all())
        assert bool((t64["ce"][:, rows] > SAT_BIG - 16).all()) and bool((t64["p"][:, rows].sort(-1).values[..., :-1] == 0).all())
        r = SAT_RIGHT_ROW
        assert bool((t64["ce"][:, r] == 0).all()) and bool((t64["py"][:, r].sum(-1) == 1).all())
        b, r = SAT_EQUAL_ROW
        assert bool((x[b, r] == -SAT_BIG).all()) and int(t64["pred"][b, r]) == 0
        assert abs(float(t64["ce"][b, r]) - float(torch.log(torch.tensor(float(C), dtype=F64)))) < 1e-15
        for t in (t64, t32):
            for k in ("ce", "p", "py", "fo"):
                assert bool(torch.isfinite(t[k]).all()), k


def _seg_case_preconditions(C, ld, S, regime):
    case = seg_loss_case(C, ld, S, regime=regime)
    x, labels = case["x"], case["labels"].long()
    assert x.shape == (3, S, ld) and x.dtype == torch.float32
    assert torch.equal(torch.round(x * 1024.0), x * 1024.0), "multiples of 2^-10"
    m = top_margin(x[..., :C].double())
    assert bool(((m == 0) | (m >= 2.0 ** -10)).all())
    ties = x[..., :C] == x[..., :C].max(-1, keepdim=True).values
    assert int((ties.sum(-1) == 2).sum()) >= 3 and (C < 3 or int((ties.sum(-1) == 3).sum()) >= 3), "exact ties of two and of three"
    for r, cls in case["tie_rows"]:
        assert first_max_index(x[:, r, :C]).tolist() == [cls[0]] * 3
    assert int(labels.max()) == C - 1
    hist = F.one_hot(labels, C).sum(1)
    assert bool((hist[1:] > 0).all()) and int(hist[0, C - 1]) == 0 and bool((hist[0, :C - 1] > 0).all() or S < 100)
    for weighted in (False, True):
        for ce_only in (False, True):
            ref = seg_stats_reference(C, ld, S, weighted, ce_only, regime=regime)          # asserts 0 < bound < 1 / (4 S)
            assert 0.0 < ref["bound"] < 1.0 / (4 * S)
            assert torch.equal(ref["pred"], ref["pred32"]), "float32 and float64 softmax order the classes alike"
            assert torch.equal(ref["pred"], first_max_index(x[..., :C])), "softmax keeps the order and the ties of the logits"
            assert ref["sums"].shape == (3, 2 + 3 * C)


HEAD_ALL = HEAD_CASES + [HEAD_EMPTY_WG_CASE]


@pytest.mark.parametrize("C,cin,residual,g_ld,dtn,weighted,shape", HEAD_ALL, ids=HEAD_IDS + ["empty-workgroups"])
def test_head_case_preconditions(C, cin, residual, g_ld, dtn, weighted, shape):
    _head_case_preconditions(C, cin, residual, g_ld, dtn, weighted, shape, "base")


@pytest.mark.parametrize("C,cin,residual,g_ld,dtn,weighted,shape,variant", HEAD_VARIANT_CASES, ids=HEAD_VARIANT_IDS)
def test_head_variant_preconditions(C, cin, residual, g_ld, dtn, weighted, shape, variant):
    """regions (a) to (d) keep their meaning; shifted: the biases of the base case + 64, the logits still exact and below 2^24 units;
    confident: the second block's core predicts class 0 with a lead of about 6, label 0 but for two voxels per sample"""
    r = _head_case_preconditions(C, cin, residual, g_ld, dtn, weighted, shape, variant)
    hc, base = head_case(C, cin, shape, residual, variant), head_case(C, cin, shape, residual)
    assert torch.equal(hc.w, base.w)
    if variant == "shifted":
        assert torch.equal(hc.b, base.b + 64.0) and torch.equal(hc.x, base.x) and torch.equal(hc.labels, base.labels)
        assert torch.equal(hc.logits(F64), base.logits(F64) + 64.0)
        assert float(hc.logits(F64).abs().max()) / 2.0 ** -11 < 2.0 ** 20 < 2.0 ** 24
        assert r["confident"] == r["confident_wrong"] == 0
    else:
        assert torch.equal(hc.b, base.b)
        n_core = shape[0] * shape[1] * 4 * 3
        assert r["confident"] == n_core - 2 * shape[0] and r["confident_wrong"] == 2 * shape[0], "the confident block is not empty"
        assert 5.0 < r["confident_lead"] < 8.0
        assert r["tile0"] == r["background"], "the block lies outside the first tile"


def _head_case_preconditions(C, cin, residual, g_ld, dtn, weighted, shape, variant):
    hc = head_case(C, cin, shape, residual, variant)
    st = torch.bfloat16 if dtn == "bf16" else torch.float16
    unit = 2.0 ** -11
    assert torch.equal(hc.x, torch.round(hc.x)) and torch.equal(hc.x.to(st).float(), hc.x), "activations: integers of the storage type"
    wu, bu = hc.w / unit, hc.b / unit
    assert torch.equal(wu, torch.round(wu)) and float(wu.abs().max()) <= 127 and torch.equal(hc.w.to(st).float(), hc.w)
    assert bool((wu[:, 1:].abs().flatten(2).sum(1) > 0).all()), "all 27 taps carry weights"
    assert torch.equal(bu, torch.round(bu))
    y64, y32 = hc.logits(torch.float64), hc.logits(torch.float32)
    assert torch.equal(y32.double(), y64), "the float32 convolution is exact"
    assert float(y64.abs().max()) / unit < 2.0 ** 20
    r = hc.regions()
    print(r)
    assert r["min_margin"] >= 2.0 ** -12
    assert r["tie2"] > 0 and (C < 3 or r["tie3"] > 0), "(a) exact ties of the top two and the top three"
    assert r["near_first"] + r["near_later"] > 0, "(b) margins in (0, 1e-3)"
    assert r["background"] == r["tile0"] == shape[0] * 256, "(c) the first tile of every sample: background in truth and prediction"
    assert r["ordinary"] > r["tile0"] // 2, "(d)"
    spread = y64.max(-1).values - y64.min(-1).values
    assert 0.25 < float(spread.median()) < 8.0, "logits spread of order 1: no saturated softmax"
    ref = head_reference(C, cin, residual, weighted, shape, HEAD_LOSS_SCALE[dtn], variant)
    S = shape[1] * shape[2] * shape[3]
    if dtn == "fp16":
        mag = ref["g64"].abs()
        assert float(mag[mag > 0].min()) >= 2.0 ** -14 and float(mag.max()) < 65504.0, "no fp16 subnormal or overflow in the gradient"
    assert 0.0 < ref["bound"] < 1.0 / (4 * S)
    assert torch.equal(ref["pred"], ref["pred_softmax"]), "softmax then argmax = first maximal logit"
    hist = F.one_hot(hc.labels.long().reshape(shape[0], -1), C).sum(1)
    assert bool((hist > 0).all()), "labels cover every class in every sample"
    assert float((ref["g32"].double() - ref["g64"]).abs().max()) > 0
    return r


def test_head_cases_take_both_directions_of_a_near_tie():
    tot = {"near_first": 0, "near_later": 0}
    for C, cin, residual, _, _, _, shape in HEAD_CASES:
        r = head_case(C, cin, shape, residual).regions()
        tot = {k: tot[k] + r[k] for k in tot}
    assert tot["near_first"] > 0 and tot["near_later"] > 0, tot


@pytest.mark.parametrize("R", [1, 32, 64])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 2048])
def test_partials_case_bound(P, R):
    part = partials_case(P, R)
    exact, mag, bound = partials_reference(part)
    assert part.shape == (2, P, R) and bool((part > 0).any()) and bool((part < 0).any()) or P * R == 1
    assert float(part.abs().max() / part.abs().min()) > 2.0 ** 20 or P * R == 1, "mixed magnitude"
    if P == 1:
        assert bound == 0.0 and torch.equal(exact, part[:, 0]), "one slot: the sum is the entry"
    else:
        assert 0.0 < bound < 1e-13, "numpy's pairwise sum errs, by a few ulp"
    assert bool((mag >= exact.abs()).all())


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
