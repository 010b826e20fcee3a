"""GPU: every entry point of the InstanceNorm + PReLU passes (norm_act.hip), the BatchNorm + PReLU passes (batch_norm_act.hip) and
their shared skeleton (norm_common.h), element by element against float64.

The older op tests (_in_op, _bn_op) bound max |error| / max |reference| of a whole tensor by 2.5e-2 (bf16) and allow the fp32 scalars the
same; here every stored element and every sum is held to float64.  The kernels are functions of (g, y, float32 tables, alpha): the
reference (norm_prelu_terms / norm_prelu_dy of reference_ops.py) reads the same float32 table values as float64, so it is exact up
to fp32 arithmetic.  Operands are drawn with a seeded
generator and rounded to the storage type; gamma in [0.5, 1.5] with channel 1 = 2^-6 and the last channel = -0.75, beta = 0.3 randn,
alpha = 0.2.  No pre-activation (xhat; gamma * xhat + beta; y * scale + shift) lies within 1e-3 of the PReLU kink: elements that did
were moved by +0.25 and rounded again (one round sufficed in every case), then the condition is ASSERTED; no element is left out.

Bounds (helpers.elem_bound / check_elems / sum_bound).  Per element (out, dy): |got - ref64| <= u * |ref64| + 16 * e32, e32 = largest |float32 - float64| evaluation of the case
(asserted > 0), u = 2^-8 bf16, 2^-10 fp16, 0 fp32; g_copy bit-equal to g.  Sums (reduce partials, sums table, d gamma, d beta,
da_part, colsum_out, ctseg_colsum): error normalised by the sum of |terms|, at most 16 x the normalised error of the plain float32
evaluation, and 0 < bound < 1 / (4 * rows summed) is asserted, so one dropped or doubled row fails.  d alpha is one scalar: see
_check_slope.  Finalize entries run on integer-valued partials (exact float64 column sums in any order) and must lie within one
fp32 ulp of the numpy float64 evaluation of the kernel's own expressions.  Outputs are pre-filled with a sentinel and one 16-byte
chunk wider than needed: columns [0, C) in bound, pad columns [C, Cv * EPC) zero, the rest and every guard entry untouched.

Measured on an MI355X, worst error / bound (float32 figures computed on the CPU in brackets):
  forward apply    instnorm bf16 0.995, fp16 0.496, fp32 0.062; scale/shift bf16 0.995, fp16 0.497, fp32 0.062  (e32 5.6e-08 .. 5.8e-07;
                   16-bit: the ulp term dominates, a correctly rounded store alone reaches 1.0 just above a power of two)
  dy               instnorm bf16 0.995, fp32 0.075; batchnorm bf16 0.994, fp32 0.062; 16-wide dy of 12-wide rows 0.982 / 0.983
                   (e32 1.8e-07 .. 7.4e-07)
  reduce partials  instnorm bf16 0.579, fp32 0.174; batchnorm bf16 0.495, fp32 0.167   (float32 figure 3.3e-09 .. 3.2e-07, and
                   1.1e-05 on one 6-row range of the 2^-6 channel; caps 7.4e-06 .. 2.5e-01)
  sums table       instnorm 0.401 / 0.192; batchnorm 0.491 / 0.197;  d gamma 0.495 / 0.225, d beta 0.451 / 0.146   (bf16 / fp32)
  da_part          instnorm 0.579 / 0.137, batchnorm 0.174 / 0.185;  d alpha at most 0.038 of its bound (_check_slope)
  colsum_out       0.025 .. 0.084;  ctseg_colsum bf16 0.069, fp32 0.243   (float32 figure 2.1e-08 .. 8.0e-08)
  plan node        out 0.992 / 0.078, dy 0.983 / 0.062, eval out 0.989 / 0.062, d gamma 0.116, d beta 0.386; mean, rstd and the running
                   statistics at most 0.055 of their propagated tolerance; batch against per-sample sums: 19867 (bf16) and 46782
                   (fp32) bounds apart
The largest case's 4200-term fp32 chains (P = 1 at S = 33600) stay within the plain bound: no sum needed a kernel-order reference.

Branches of norm_common.h (the expected Cv and grids are asserted in test_sweep_branches):
  chunk_sweep_fwd / _bwd: the kept-chunk branch everywhere but (2, 10, 125) fp32 (Cv = 3, 2 blocks: per-element division); one
  iteration per thread up to (1, 256, 33600) bf16 (4096-block cap, 832 rows swept twice); P_cap = N in the colsum apply: one block
  per sample, three iterations.  bwd_reduce_rows: wave butterflies at Cv = 2, 4, 32, 64; slot per thread at Cv = 3, 5, 10 and 96
  (nrow_thr = 2).  store_dy_chunk: the widened 16-byte store and the plain 8-byte one (test_backward_12_wide_rows).  col16_stats<16>
  up to 1024 rows, <64> up to 8192 (InstanceNorm) and beyond 1024 (BatchNorm), the two-level InstanceNorm kernel above, its counter
  reset, the variance clamp, count == 1, momentum 0 / 0.1 / 0.25 / 1.  block_sum3 and slope_grad_sum with more rows than threads.

Fixed here:
  * ctseg_colsum, bf16, 1024 < C <= 2048: colsum_final_kernel has one thread per partial column and 1024 threads; the launcher let
    up to 2048 columns through, the kernel then formed no sub-sum and wrote 0 to columns 0 .. 1023 (seen on the device: every
    output 0).  The launcher refuses more than 1024 partial columns (test_colsum_width_limit).

Not covered: fp16 in the backward (the library has no such kernels: the refusal is asserted); CTSEG_MAX_WG caps (they size conv
grids, not these passes); the InstanceNorm fusions into the conv passes (operand normalisation, backward statistics in the
epilogue: test_gpu_conv_extras.py); C > 256 * EPC in the reduce pass (refused by the launcher; no layer comes near).
"""
import functools
import inspect
import re
import sys
import types
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd._native import BF16, F16, F32  # noqa: E402
from capstone_amd.engine import BufferStore, GemmLayer, rup  # noqa: E402
from capstone_amd.plan import Plan, _BatchNormAct, _bwd_row_ranges, _NormAct  # noqa: E402
from helpers import ACT_SENTINEL, GRAD_SENTINEL, TDT, MiniPlan, check_elems, elem_bound, from_cl, sum_bound, to_cl  # noqa: E402
from reference_ops import norm_prelu_dy, norm_prelu_terms, rounded  # noqa: E402

DEV = "cuda:0"
DT_ID = {F32: "fp32", BF16: "bf16", F16: "fp16"}
ALPHA = 0.2
EPS = 1e-5
KINK = 1e-3
POISON = 24576.0             # 3 * 2^13: exact in bf16, fp16 and fp32; what the columns a pass must not use hold
BIG = 1e30                   # the same for fp32 partial rows
F64, F32T = torch.float64, torch.float32


def _call(name, *args):
    nat.call(name, *args)


def _sync():
    torch.cuda.synchronize()


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def _guarded(n, fill=GRAD_SENTINEL, dtype=torch.float32, tail=8):
    """n entries followed by ``tail`` guard entries, all holding ``fill``"""
    return torch.full((n + tail,), fill, dtype=dtype, device=DEV)


# ---- the launchers' geometry, as norm_common.h writes it ------------------------------------------------------------------------
def _chunks(dt, C, *lds, half_chunks=True):
    """CHECK_CL: (elements per chunk, chunks per row)"""
    epc = 4 if dt == F32 else 8
    if half_chunks and dt != F32 and any(ld % 8 for ld in lds):
        epc = 4
    return epc, -(-C // epc)


def _ew_blocks_for(total, Cv, exact=False, cap=4096):
    b = min(4096, max(1, -(-total // 256)))
    b, step = min(b, cap), Cv
    while step % 2 == 0:
        step //= 2
    if exact or b >= step:
        b = b // step * step
    return b


def _sweep(S, Cv):
    """(blocks, branch of chunk_sweep_*, iterations of the busiest thread)"""
    b = _ew_blocks_for(S * Cv, Cv)
    stride = b * 256
    return b, ("keep" if stride % Cv == 0 else "divide"), -(-S * Cv // stride)


def _wide(dt):
    """one 16-byte chunk, in elements"""
    return 4 if dt == F32 else 8


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _rows(x, dt, ld, fill=POISON):
    """(N, C, S) cpu tensor -> device storage [N][S][ld]; columns [C, ld) hold ``fill``"""
    N, C, S = x.shape
    t = torch.full((N, S, ld), fill, dtype=TDT[dt])
    t[..., :C] = x.permute(0, 2, 1).to(TDT[dt])
    return t.to(DEV)


def _out_rows(N, S, ld, dt, tail=64):
    """a sentinel-filled output of N * S rows ``ld`` wide, with ``tail`` guard elements behind the last row"""
    return torch.full((N * S * ld + tail,), ACT_SENTINEL, dtype=TDT[dt], device=DEV)


@functools.lru_cache(maxsize=4)
def _data(kind, N, C, S, dt, moved=False):
    """Operands (rounded to the storage type) and float32 tables of one case.  kind: "in" (per-sample mean / rstd; pre-activation
    xhat), "bn" (batch mean / rstd, gamma, beta; pre-activation gamma * xhat + beta), "ss" (scale / shift table; pre-activation
    y * scale + shift).  moved: the mean table moved by 0.625 standard deviations.  No element's pre-activation, evaluated in
    float64 on the float32 tables, lies within KINK of the PReLU kink (asserted)."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((kind, N, C, S, dt, moved)).encode()))
    y = rounded(torch.randn(N, C, S, generator=g) * 1.3 + 0.4, TDT[dt])
    gy = rounded(torch.randn(N, C, S, generator=g), TDT[dt])
    res = rounded(torch.randn(N, C, S, generator=g), TDT[dt])
    dims = (2,) if kind == "in" else (0, 2)
    m64 = y.double().mean(dims, keepdim=True)
    v64 = y.double().var(dims, unbiased=False, keepdim=True)
    if moved:
        m64 = m64 + 0.625 * v64.sqrt()
    d = types.SimpleNamespace(kind=kind, N=N, C=C, S=S, dt=dt, g=gy, res=res)
    d.m, d.r = m64.float(), (v64 + EPS).rsqrt().float()
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[1], gamma[C - 1] = 2.0 ** -6, -0.75
    d.gamma, d.beta = gamma.reshape(1, C, 1), (0.3 * torch.randn(C, generator=g)).reshape(1, C, 1)
    d.sc = (d.gamma.double() * d.r.double()).float()
    d.sh = (d.beta.double() - d.m.double() * d.sc.double()).float()

    def pre(yy):
        if kind == "ss":
            return yy.double() * d.sc.double() + d.sh.double()
        xh = (yy.double() - d.m.double()) * d.r.double()
        return xh if kind == "in" else d.gamma.double() * xh + d.beta.double()
    for rounds in range(9):
        near = pre(y).abs() < KINK
        if not bool(near.any()):
            break
        assert rounds < 8
        y = rounded(torch.where(near, y + 0.25, y), TDT[dt])
    assert float(pre(y).abs().min()) >= KINK
    d.y, d.kink_rounds = y, rounds
    return d


def _al(T):
    return torch.tensor(ALPHA, dtype=torch.float32).to(T)


def _fwd_ref(d, T, residual):
    y = d.y.to(T)
    pre = (y - d.m.to(T)) * d.r.to(T) if d.kind == "in" else y * d.sc.to(T) + d.sh.to(T)
    o = torch.where(pre > 0, pre, _al(T) * pre)
    return o + d.res.to(T) if residual else o


def _bwd_args(d, T):
    """(g, y, mean, rstd, alpha, gamma, beta) of a case in precision T; gamma and beta None for InstanceNorm"""
    gb = (None, None) if d.kind == "in" else (d.gamma.to(T), d.beta.to(T))
    return (d.g.to(T), d.y.to(T), d.m.to(T), d.r.to(T), _al(T)) + gb


def _bwd_terms(d, T):
    """xhat, dz (the gradient behind the PReLU) and the three summed terms, in precision T"""
    return norm_prelu_terms(*_bwd_args(d, T))


def _bwd_dy(d, T, per_sample=False):
    return norm_prelu_dy(*_bwd_args(d, T), dims=(2,) if (d.kind == "in" or per_sample) else (0, 2))


# ---- the checks (the bounds per element and per sum: helpers) -------------------------------------------------------------------
def _check_rows(tag, flat, N, S, ld, C, store, ref64, ref32, dt):
    """an output the test pre-filled with the sentinel: columns [0, C) within the bound, [C, store) zero, the rest untouched"""
    got = flat.float().cpu()
    body, tail = got[:N * S * ld].view(N, S, ld), got[N * S * ld:]
    assert bool((tail == ACT_SENTINEL).all()), f"{tag}: written behind the last row"
    assert bool((body[..., store:] == ACT_SENTINEL).all()), f"{tag}: columns [{store}, {ld}) were written"
    assert bool((body[..., C:store] == 0).all()), f"{tag}: pad columns [{C}, {store}) are not zero"
    return check_elems(tag, body[..., :C].permute(0, 2, 1), ref64, ref32, dt)


def _check_sums(tag, got, t64, t32, dims, rows, div=1.0):
    """``got`` (= sums / div) against the float64 sums, error normalised by the sum of |terms| (helpers.sum_bound).  A sum none of whose
    terms is nonzero must be exactly 0."""
    s64, norm, live, bound = sum_bound(tag, t64, t32, dims, rows, div)
    got = got.double().cpu() * div
    assert got.shape == s64.shape, (got.shape, s64.shape)
    assert bool((got[~live] == 0).all()), f"{tag}: a sum without terms is not 0"
    err = float(((got - s64).abs() / norm)[live].max())
    print(f"{tag}: worst error / bound {err / bound:.3f} (float32 figure {bound / 16:.2e}, cap {1 / (4 * rows):.2e})")
    assert err <= bound, (tag, err, bound)
    return err / bound


def _check_slope(tag, got, t64, t32, dims, rows):
    """d alpha, one scalar: the float32 cast of the float64 sum of the per-channel slope terms (da_part), which the reduce pass
    accumulated in fp32.  The plain float32 sum of all terms is ONE sample of a rounding error (5e-10 of the sum of |terms| at
    (2, 10, 125) fp32, where the kernel's 6.7e-10 was 1.26 x 16 times it), not a bound.  The kernel's order of operations gives
    one: every da_part lies within the per-channel bound of its own sum of |terms| (sum_bound over ``dims``), so their float64
    sum lies within that bound of the total, and the cast adds at most 2^-24 of it."""
    _, _, _, bound = sum_bound(tag, t64, t32, dims, rows)
    bound += 2.0 ** -24
    assert bound < 1.0 / (4.0 * rows)
    s64, a64 = t64.sum(), t64.abs().sum()
    err = float((got.double().cpu().reshape(()) - s64).abs() / a64)
    print(f"{tag}: worst error / bound {err / bound:.3f} (bound {bound:.2e}, cap {1 / (4 * rows):.2e})")
    assert err <= bound, (tag, err, bound)
    return err / bound


def _ranges(t, P):
    """(N, C, S) -> (N, C, P, rows_per): the row ranges of bwd_reduce_rows, zero-padded"""
    N, C, S = t.shape
    rp = -(-S // P)
    return torch.nn.functional.pad(t, (0, P * rp - S)).reshape(N, C, P, rp)


def _ulp_close(got, exp64):
    """within one float32 unit in the last place of the float64 expectation rounded to float32"""
    e32 = np.asarray(exp64, dtype=np.float64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - e32.astype(np.float64)) <= np.spacing(np.abs(e32)).astype(np.float64)))


# =================================================================================================================================
# 1. finalize entries on synthetic partials
# =================================================================================================================================
def _int_partials(rng, R, ld, col0, C, K=2, clamp=None):
    """R rows of [K][ld] integer-valued fp32 partials whose column totals are s in [-64, 64] and (second row) s^2 + a positive
    integer (third row, K = 3: any integer); column ``clamp`` gets a total of squares of 0 beside a nonzero sum (var < 0).  Columns
    outside [col0, col0 + C) hold BIG.  -> (partials, totals [K][C] as float64)"""
    part = np.full((R, K, ld), BIG, np.float32)
    tot = np.empty((K, C), np.int64)
    tot[0] = rng.integers(-64, 65, C)
    tot[1] = tot[0] ** 2 + rng.integers(1, 50, C)
    if K == 3:
        tot[2] = rng.integers(-500, 500, C)
    if clamp is not None:
        tot[0, clamp], tot[1, clamp] = 37, 0
    v = rng.integers(-3, 4, (R, K, C))
    v[0] += tot - v.sum(0)
    assert np.abs(v).max() < 2 ** 22
    part[:, :, col0:col0 + C] = v
    return part, tot.astype(np.float64)


def _stats(tot, count, eps):
    mean = tot[0] / count
    var = np.maximum(tot[1] / count - mean * mean, 0.0)
    return mean, var, 1.0 / np.sqrt(var + eps)


# P: 1 / 7 / 1024 rows col16_stats<16>; 1025 / 8192 col16_stats<64>; 8193 / 8200 the two-level kernel with 64 groups and the counter
FIN_CASES = [(P, 16, c0, C) for P in (1, 7, 1024, 1025, 8192, 8193, 8200) for c0, C in ((0, 10), (8, 8))] + [(1025, 256, 24, 200)]


@pytest.mark.parametrize("P,ld,col0,C", FIN_CASES, ids=[f"P={c[0]} ld={c[1]} col0={c[2]} C={c[3]}" for c in FIN_CASES])
def test_instnorm_finalize(P, ld, col0, C):
    N, count, clamp = 2, 1000.0, 3
    rng = np.random.default_rng(P * 1000 + ld + col0)
    parts, tots = zip(*[_int_partials(rng, P, ld, col0, C, clamp=clamp) for _ in range(N)])
    part = _dev32(np.stack(parts))
    scratch = torch.zeros(N * 64 * 2 * ld + N, dtype=torch.float64, device=DEV)
    runs = []
    for _ in range(2 if P > 8192 else 1):           # the two-level kernel resets its counters: a second call on the same scratch
        mr = _guarded(N * C * 2)
        _call("ctseg_instnorm_finalize", part.data_ptr(), N, P, ld, col0, C, count, EPS, scratch.data_ptr(), mr.data_ptr())
        _sync()
        runs.append(mr.cpu())
    mr = runs[0]
    assert bool((mr[N * C * 2:] == GRAD_SENTINEL).all())
    got = mr[:N * C * 2].view(N, C, 2).numpy()
    for n in range(N):
        mean, var, rstd = _stats(tots[n], count, EPS)
        assert var[clamp] == 0.0 and (np.delete(var, clamp) > 0).all()
        assert _ulp_close(got[n, :, 0], mean), "mean"
        assert _ulp_close(got[n, :, 1], rstd), "rstd"
        assert got[n, clamp, 1] == np.float32(1.0 / np.sqrt(EPS)), "variance clamp"
    if len(runs) == 2:
        assert torch.equal(runs[0], runs[1]), "second call on the same scratch"
        assert bool((scratch[N * 64 * 2 * ld:].view(torch.int64) == 0).all()), "counters reset"


# N * P = 1 / 1024: col16_stats<16>; 1025 / 2050: col16_stats<64>
@pytest.mark.parametrize("C,col0", [(10, 0), (13, 3)])
@pytest.mark.parametrize("N,P", [(1, 1), (2, 512), (1, 1025), (2, 1025)])
def test_batchnorm_finalize(N, P, C, col0):
    ld, S = 16, 1000
    rng = np.random.default_rng(N * 10000 + P + C)
    part_np, tot = _int_partials(rng, N * P, ld, col0, C)
    part = _dev32(part_np)
    gamma = (0.5 + rng.random(C)).astype(np.float32)
    gamma[1], gamma[C - 1] = 2.0 ** -6, -0.75
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    rm0, rv0 = (0.1 * rng.standard_normal(C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    G = 4
    for momentum in (0.0, 0.1, 1.0):
        for eps in (1e-5, 1e-3):
            for count in (1.0, float(N * S)):
                # [guard | gamma | guard | beta | guard | running_mean | guard | running_var | guard]
                flat = np.full(4 * C + 5 * G, GRAD_SENTINEL, np.float32)
                offs = [G + i * (C + G) for i in range(4)]
                for o, v in zip(offs, (gamma, beta, rm0, rv0)):
                    flat[o:o + C] = v
                fl = _dev32(flat)
                p = [fl.data_ptr() + 4 * o for o in offs]
                nbt = torch.tensor([-7, 0, -7], dtype=torch.int64, device=DEV)
                mean, var, rstd = _stats(tot, count, eps)
                sc = gamma.astype(np.float64) * rstd
                unb = var * count / (count - 1.0) if count > 1.0 else var
                rm, rv = rm0, rv0
                for calls in (1, 2):
                    mr, ss = _guarded(2 * C), _guarded(2 * C)
                    _call("ctseg_batchnorm_finalize", part.data_ptr(), N, P, ld, col0, C, count, eps, momentum, p[0], p[1], p[2], p[3],
                          nbt.data_ptr() + 8, mr.data_ptr(), ss.data_ptr())
                    _sync()
                    tag = f"momentum {momentum} eps {eps} count {count} call {calls}"
                    mr, ss, f = mr.cpu().numpy(), ss.cpu().numpy(), fl.cpu().numpy()
                    assert (mr[2 * C:] == GRAD_SENTINEL).all() and (ss[2 * C:] == GRAD_SENTINEL).all(), tag
                    assert _ulp_close(mr[:2 * C:2], mean) and _ulp_close(mr[1:2 * C:2], rstd), tag
                    assert _ulp_close(ss[:2 * C:2], sc) and _ulp_close(ss[1:2 * C:2], beta.astype(np.float64) - mean * sc), tag
                    keep = np.ones(f.size, bool)
                    for o in offs[2:]:
                        keep[o:o + C] = False
                    assert (f[keep] == flat[keep]).all(), f"{tag}: gamma, beta or a guard changed"
                    want_m = (1.0 - momentum) * rm.astype(np.float64) + momentum * mean
                    want_v = (1.0 - momentum) * rv.astype(np.float64) + momentum * unb
                    rm, rv = f[offs[2]:offs[2] + C].copy(), f[offs[3]:offs[3] + C].copy()
                    assert _ulp_close(rm, want_m), f"{tag}: running_mean"
                    assert _ulp_close(rv, want_v), f"{tag}: running_var"
                    if momentum == 0.0:
                        assert (rm == rm0).all() and (rv == rv0).all(), tag
                    assert nbt.cpu().tolist() == [-7, calls, -7], tag
                if count == 1.0:
                    assert (unb == var).all()


@pytest.mark.parametrize("C", [10, 300])            # 300: the loop of the 256 threads runs a second time
def test_batchnorm_eval_table(C):
    rng = np.random.default_rng(C)
    rm, rv = (0.4 * rng.standard_normal(C)).astype(np.float32), (0.2 + rng.random(C)).astype(np.float32)
    gamma = (0.5 + rng.random(C)).astype(np.float32)
    gamma[1], gamma[C - 1] = 2.0 ** -6, -0.75
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    ss = _guarded(2 * C)
    t = [_dev32(a) for a in (rm, rv, gamma, beta)]
    _call("ctseg_batchnorm_eval_table", t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), C, EPS, ss.data_ptr())
    _sync()
    ss = ss.cpu().numpy()
    sc = gamma.astype(np.float64) / np.sqrt(rv.astype(np.float64) + EPS)
    assert (ss[2 * C:] == GRAD_SENTINEL).all()
    assert _ulp_close(ss[:2 * C:2], sc), "scale"
    assert _ulp_close(ss[1:2 * C:2], beta.astype(np.float64) - rm.astype(np.float64) * sc), "shift"


@pytest.mark.parametrize("P", [1, 300])             # 300: block_sum3's 256 threads take a second row
def test_instnorm_prelu_bwd_finalize(P):
    N, C, ld, S = 2, 10, 12, 315.0
    rng = np.random.default_rng(P)
    parts, tots = zip(*[_int_partials(rng, P, ld, 0, C, K=3) for _ in range(N)])
    part = _dev32(np.stack(parts))
    tot = np.stack(tots)                             # [N][3][C]
    for with_dalpha in (False, True):                # True: the slope sum by the block that finishes last, which resets its counter
        sums = _guarded(N * C * 2)
        da = torch.full((N * C + 1 + 4,), -3.0, dtype=torch.float64, device=DEV)
        da[N * C] = 0.0                              # the counter slot behind the N * C terms
        dal = _guarded(1)
        _call("ctseg_instnorm_prelu_bwd_finalize", part.data_ptr(), N, P, ld, C, S, da.data_ptr(), sums.data_ptr(),
              dal.data_ptr() if with_dalpha else None)
        _sync()
        sums, da, dal = sums.cpu().numpy(), da.cpu().numpy(), dal.cpu().numpy()
        assert (sums[N * C * 2:] == GRAD_SENTINEL).all() and (da[N * C + 1:] == -3.0).all() and da[N * C] == 0.0
        got = sums[:N * C * 2].reshape(N, C, 2)
        assert _ulp_close(got[..., 0], tot[:, 0] / S) and _ulp_close(got[..., 1], tot[:, 1] / S)
        assert (da[:N * C].reshape(N, C) == tot[:, 2]).all(), "da_part"
        assert (dal[1:] == GRAD_SENTINEL).all()
        assert dal[0] == (np.float32(tot[:, 2].sum()) if with_dalpha else GRAD_SENTINEL), "d alpha"


@pytest.mark.parametrize("P", [1, 300])
def test_batchnorm_prelu_bwd_finalize(P):
    N, C, ld, M = 2, 10, 12, 630.0
    rng = np.random.default_rng(P + 5)
    part_np, tot = _int_partials(rng, N * P, ld, 0, C, K=3)
    part = _dev32(part_np)
    sums, grads = _guarded(2 * C), _guarded(2 * C + 4)          # [d gamma | guard | d beta | guard]
    da = torch.full((C + 4,), -3.0, dtype=torch.float64, device=DEV)
    _call("ctseg_batchnorm_prelu_bwd_finalize", part.data_ptr(), N, P, ld, C, M, sums.data_ptr(), grads.data_ptr(),
          grads.data_ptr() + 4 * (C + 4), da.data_ptr())
    _sync()
    sums, grads, da = sums.cpu().numpy(), grads.cpu().numpy(), da.cpu().numpy()
    assert (sums[2 * C:] == GRAD_SENTINEL).all() and (da[C:] == -3.0).all()
    assert (grads[C:C + 4] == GRAD_SENTINEL).all() and (grads[2 * C + 4:] == GRAD_SENTINEL).all()
    assert _ulp_close(sums[:2 * C:2], tot[0] / M) and _ulp_close(sums[1:2 * C:2], tot[1] / M)
    assert (grads[C + 4:2 * C + 4] == tot[0]).all(), "d beta"
    assert (grads[:C] == tot[1]).all(), "d gamma"
    assert (da[:C] == tot[2]).all(), "da_part"


# n_da: less than a wave, one short of / one past the block, a third sweep of the block
@pytest.mark.parametrize("n_da", [1, 255, 257, 2 * 256 + 1])
def test_slope_gradient_sums(n_da):
    rng = np.random.default_rng(n_da)
    terms = rng.integers(-4096, 4096, n_da + 4) / 64.0           # multiples of 2^-6: every order of summation is exact
    want = np.float32(terms[:n_da].sum())
    da = torch.as_tensor(terms, dtype=torch.float64).to(DEV)
    out = _guarded(1)
    _call("ctseg_instnorm_prelu_dalpha", da.data_ptr(), n_da, out.data_ptr())
    _sync()
    assert out.cpu().tolist() == [float(want)] + [GRAD_SENTINEL] * 8
    # the same sum by block (0, 0) of the two apply passes (slope_grad_sum)
    for kind in ("in", "bn"):
        b = _Bwd(kind, 2, 8, 3, F32)
        out = _guarded(1)
        b.apply(b.exact_sums(), da_part=da, n_da=n_da, dalpha=out)
        assert out.cpu().tolist() == [float(want)] + [GRAD_SENTINEL] * 8, kind


# =================================================================================================================================
# 2. forward apply
# =================================================================================================================================
# (N, C, S, storage types, 12-wide rows).  chunk_sweep_fwd, from ew_blocks_for (asserted in test_sweep_branches):
#   (2, 10, 315) fp32 Cv = 3: 4 -> 3 blocks, stride 768 a multiple of 3: a thread keeps its chunk; 16-bit Cv = 2
#   (2, 10, 315) 12-wide, 16-bit: 8-byte chunks (EPC = 4), Cv = 3, as fp32
#   (2, 40, 315) Cv = 10 / 5: 13 -> 10 blocks / 7 -> 5 blocks, kept      (3, 256, 315) Cv = 64 / 32, kept
#   (2, 8, 3) one block, six (fp32) / three work items: one thread's worth
#   (2, 10, 125) fp32 Cv = 3: 2 blocks, fewer than Cv's odd part, stride 512: the per-element division branch
#   (1, 256, 33600) bf16 Cv = 32: 4200 -> 4096 blocks, 32768 rows per sweep: rows 0 .. 831 in a second iteration
ALL3, TRAIN2 = (F32, BF16, F16), (F32, BF16)
FWD_CASES = [(2, 10, 315, ALL3, False), (2, 10, 315, (BF16, F16), True), (1, 16, 315, ALL3, False), (2, 40, 315, ALL3, False),
             (3, 256, 315, ALL3, False), (2, 8, 3, ALL3, False), (2, 10, 125, (F32,), False), (1, 256, 33600, (BF16,), False)]
BWD_CASES = [(N, C, S, tuple(d for d in dts if d != F16), nar) for N, C, S, dts, nar in FWD_CASES] + [(2, 384, 105, (F32,), False)]


def _expand(cases):
    out = [(N, C, S, dt, nar) for N, C, S, dts, nar in cases for dt in dts]
    return out, [f"{N}x{C}x{S} {DT_ID[dt]}{' 12-wide' if nar else ''}" for N, C, S, dt, nar in out]


def test_sweep_branches():
    assert _sweep(315, 3) == (3, "keep", 2) and _sweep(315, 2) == (3, "keep", 1)
    assert _sweep(315, 10) == (10, "keep", 2) and _sweep(315, 5) == (5, "keep", 2)
    assert _sweep(3, 2) == (1, "keep", 1)
    assert _sweep(125, 3) == (2, "divide", 1)
    assert _sweep(33600, 32) == (4096, "keep", 2) and 33600 - 4096 * 256 // 32 == 832
    assert _chunks(BF16, 10, 12, 20) == (4, 3) and _chunks(BF16, 10, 16, 24) == (8, 2) and _chunks(F32, 384, 384) == (4, 96)


FWD, FWD_IDS = _expand(FWD_CASES)


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kind", ["in", "ss"], ids=["instnorm", "scale_shift"])
@pytest.mark.parametrize("N,C,S,dt,narrow", FWD, ids=FWD_IDS)
def test_forward_apply(N, C, S, dt, narrow, kind, residual):
    d = _data(kind, N, C, S, dt)
    w = _wide(dt)
    y_ld = 12 if narrow else rup(C, w)
    res_ld, out_ld = y_ld + w, y_ld + w              # the residual's rows are one chunk wider than y's, the output's too
    epc, Cv = _chunks(dt, C, y_ld, out_ld, res_ld if residual else y_ld)
    assert epc == (4 if narrow or dt == F32 else 8)
    y = _rows(d.y, dt, y_ld)
    res = _rows(d.res, dt, res_ld) if residual else None
    out = _out_rows(N, S, out_ld, dt)
    al = _dev32([ALPHA])
    if kind == "in":
        tab = torch.stack([d.m, d.r], -1).reshape(N, C, 2).contiguous().to(DEV)
        _call("ctseg_instnorm_prelu_fwd", dt, y.data_ptr(), y_ld, tab.data_ptr(), al.data_ptr(), nat.ptr(res), res_ld if residual else 0,
              out.data_ptr(), out_ld, N, S, C)
    else:
        tab = torch.stack([d.sc, d.sh], -1).reshape(C, 2).contiguous().to(DEV)
        _call("ctseg_scale_shift_prelu_fwd", dt, y.data_ptr(), y_ld, tab.data_ptr(), al.data_ptr(), nat.ptr(res), res_ld if residual else 0,
              out.data_ptr(), out_ld, N, S, C)
    _sync()
    _check_rows(f"forward {kind} {N}x{C}x{S} {DT_ID[dt]}", out, N, S, out_ld, C, Cv * epc, _fwd_ref(d, F64, residual),
                _fwd_ref(d, F32T, residual), dt)


def test_instnorm_prelu_fwd_without_a_norm_adds_the_residual():
    """mean_rstd == NULL: out = y + res (the residual hand-off of a ResidualUnit): exact in fp32, one rounding in bf16"""
    d = _data("in", 2, 10, 315, BF16)
    y, res, out = _rows(d.y, BF16, 16), _rows(d.res, BF16, 24), _out_rows(2, 315, 24, BF16)
    _call("ctseg_instnorm_prelu_fwd", BF16, y.data_ptr(), 16, None, None, res.data_ptr(), 24, out.data_ptr(), 24, 2, 315, 10)
    _sync()
    body = out.float().cpu()[:2 * 315 * 24].view(2, 315, 24)
    assert torch.equal(body[..., :10].permute(0, 2, 1), rounded(d.y + d.res, TDT[BF16]))
    assert bool((body[..., 10:16] == 0).all()) and bool((body[..., 16:] == ACT_SENTINEL).all())


# =================================================================================================================================
# 3. backward: reduce -> finalize -> apply
# =================================================================================================================================
class _Bwd:
    """the device buffers of one backward case and its three passes, called directly"""

    def __init__(self, kind, N, C, S, dt, narrow=False, moved=False):
        self.d = d = _data(kind, N, C, S, dt, moved)
        self.kind, self.N, self.C, self.S, self.dt = kind, N, C, S, dt
        w = _wide(dt)
        self.g_ld = 12 if narrow else rup(C, w) + w       # g's rows one chunk wider than y's
        self.y_ld = 12 if narrow else rup(C, w)
        self.g, self.y = _rows(d.g, dt, self.g_ld), _rows(d.y, dt, self.y_ld)
        self.pld = rup(C, 4) + 4
        self.al = _dev32([ALPHA])
        if kind == "in":
            self.mr = torch.stack([d.m, d.r], -1).reshape(N, C, 2).contiguous().to(DEV)
        else:
            self.mr = torch.stack([d.m, d.r], -1).reshape(C, 2).contiguous().to(DEV)
            self.gamma, self.beta = d.gamma.reshape(C).contiguous().to(DEV), d.beta.reshape(C).contiguous().to(DEV)
        self.t64, self.t32 = _bwd_terms(d, F64)[2], _bwd_terms(d, F32T)[2]
        self.rows = S if kind == "in" else N * S          # rows in one of the finalised sums
        self.tag = f"{kind} {N}x{C}x{S} {DT_ID[dt]}{' 12-wide' if narrow else ''}"
        self._dy = None

    def dy_refs(self):
        """(float64, float32) evaluations of dy, computed once"""
        if self._dy is None:
            self._dy = (_bwd_dy(self.d, F64), _bwd_dy(self.d, F32T))
        return self._dy

    def reduce(self, P, dt=None):
        N, C, S = self.N, self.C, self.S
        part = torch.full((N, P, 3, self.pld), GRAD_SENTINEL, dtype=torch.float32, device=DEV)
        head = (self.dt if dt is None else dt, self.g.data_ptr(), self.g_ld, self.y.data_ptr(), self.y_ld, self.mr.data_ptr())
        if self.kind == "in":
            _call("ctseg_instnorm_prelu_bwd_reduce", *head, self.al.data_ptr(), part.data_ptr(), P, self.pld, N, S, C)
        else:
            _call("ctseg_batchnorm_prelu_bwd_reduce", *head, self.gamma.data_ptr(), self.beta.data_ptr(), self.al.data_ptr(),
                  part.data_ptr(), P, self.pld, N, S, C)
        _sync()
        return part

    def check_partials(self, part, P):
        got = part.cpu()
        assert bool((got[..., self.C:] == GRAD_SENTINEL).all()), "partial columns beyond C"
        rows_per = -(-self.S // P)
        return max(_check_sums(f"{self.tag} P={P} partial {k + 1}", got[:, :, k, :self.C].permute(0, 2, 1), _ranges(self.t64[k], P),
                               _ranges(self.t32[k], P), (3,), rows_per) for k in range(3))

    def finalize(self, part, P):
        """-> (sums table, da_part, d gamma | d beta or None), all on the device and checked"""
        N, C, S = self.N, self.C, self.S
        if self.kind == "in":
            sums = _guarded(N * C * 2)
            da = torch.full((N * C + 1 + 4,), -3.0, dtype=torch.float64, device=DEV)
            _call("ctseg_instnorm_prelu_bwd_finalize", part.data_ptr(), N, P, self.pld, C, float(S), da.data_ptr(), sums.data_ptr(), None)
            _sync()
            assert bool((sums[N * C * 2:] == GRAD_SENTINEL).all()) and bool((da[N * C:] == -3.0).all())
            tab = sums[:N * C * 2].view(N, C, 2).cpu()
            r = [_check_sums(f"{self.tag} P={P} sums {k + 1}", tab[..., k], self.t64[k], self.t32[k], (2,), S, div=float(S)) for k in (0, 1)]
            r.append(_check_sums(f"{self.tag} P={P} da_part", da[:N * C].view(N, C), self.t64[2], self.t32[2], (2,), S))
            return sums, da, None, max(r)
        sums, grads = _guarded(2 * C), _guarded(2 * C + 4)
        da = torch.full((C + 4,), -3.0, dtype=torch.float64, device=DEV)
        _call("ctseg_batchnorm_prelu_bwd_finalize", part.data_ptr(), N, P, self.pld, C, float(N * S), sums.data_ptr(), grads.data_ptr(),
              grads.data_ptr() + 4 * (C + 4), da.data_ptr())
        _sync()
        assert bool((sums[2 * C:] == GRAD_SENTINEL).all()) and bool((da[C:] == -3.0).all())
        assert bool((grads[C:C + 4] == GRAD_SENTINEL).all()) and bool((grads[2 * C + 4:] == GRAD_SENTINEL).all())
        tab, M = sums[:2 * C].view(C, 2).cpu(), N * S
        r = [_check_sums(f"{self.tag} P={P} sums {k + 1}", tab[:, k], self.t64[k], self.t32[k], (0, 2), M, div=float(M)) for k in (0, 1)]
        r.append(_check_sums(f"{self.tag} P={P} d beta", grads[C + 4:2 * C + 4], self.t64[0], self.t32[0], (0, 2), M))
        r.append(_check_sums(f"{self.tag} P={P} d gamma", grads[:C], self.t64[1], self.t32[1], (0, 2), M))
        r.append(_check_sums(f"{self.tag} P={P} da_part", da[:C], self.t64[2], self.t32[2], (0, 2), M))
        return sums, da, grads, max(r)

    def exact_sums(self):
        """the sums table from float64 (for runs that are not about the sums)"""
        dims = (2,) if self.kind == "in" else (0, 2)
        return torch.stack([self.t64[0].mean(dims), self.t64[1].mean(dims)], -1).float().contiguous().to(DEV)

    def apply(self, sums, dy=None, dy_ld=None, g_copy=None, gc_ld=0, da_part=None, n_da=0, dalpha=None, colsum=None, dt=None):
        N, C, S = self.N, self.C, self.S
        if dy is None:
            dy_ld = self.y_ld + _wide(self.dt)
            dy = _out_rows(N, S, dy_ld, self.dt)
        head = (self.dt if dt is None else dt, self.g.data_ptr(), self.g_ld, self.y.data_ptr(), self.y_ld, self.mr.data_ptr())
        tail = (sums.data_ptr(), dy.data_ptr(), dy_ld, nat.ptr(g_copy), gc_ld, N, S, C)
        slope = (nat.ptr(da_part), n_da, nat.ptr(dalpha))
        if self.kind == "bn":
            _call("ctseg_batchnorm_prelu_bwd_apply", *head, self.gamma.data_ptr(), self.beta.data_ptr(), self.al.data_ptr(), *tail, *slope)
        elif colsum is None:
            _call("ctseg_instnorm_prelu_bwd_apply", *head, self.al.data_ptr(), *tail, *slope)
        else:
            cs_part, p_cap, cs_out = colsum
            _call("ctseg_instnorm_prelu_bwd_apply_colsum", *head, self.al.data_ptr(), *tail, cs_part.data_ptr(), p_cap, cs_out.data_ptr(),
                  *slope)
        _sync()
        return dy, dy_ld

    def check_dy(self, dy, dy_ld, store, what="dy"):
        return _check_rows(f"{self.tag} {what}", dy, self.N, self.S, dy_ld, self.C, store, *self.dy_refs(), self.dt)

    def check_dalpha(self, dalpha, what="d alpha"):
        assert bool((dalpha[1:] == GRAD_SENTINEL).all())
        return _check_slope(f"{self.tag} {what}", dalpha[:1], self.t64[2], self.t32[2], (2,) if self.kind == "in" else (0, 2),
                            self.N * self.S)

    def chain(self, P):
        """the three passes at P row ranges per sample -> (dy, dy_ld, g_copy, sums, da_part, grads, dalpha), every output checked"""
        N, C, S, dt = self.N, self.C, self.S, self.dt
        part = self.reduce(P)
        self.check_partials(part, P)
        sums, da, grads, _ = self.finalize(part, P)
        gc_ld = self.y_ld + _wide(dt)
        gc, dal = _out_rows(N, S, gc_ld, dt), _guarded(1)
        n_da = N * C if self.kind == "in" else C
        dy, dy_ld = self.apply(sums, g_copy=gc, gc_ld=gc_ld, da_part=da, n_da=n_da, dalpha=dal)
        epc, Cv = _chunks(dt, C, self.g_ld, self.y_ld, dy_ld, gc_ld)
        self.check_dy(dy, dy_ld, Cv * epc)
        self.check_dalpha(dal)
        body = gc.float().cpu()
        assert bool((body[N * S * gc_ld:] == ACT_SENTINEL).all())
        body = body[:N * S * gc_ld].view(N, S, gc_ld)
        assert torch.equal(body[..., :C].permute(0, 2, 1), self.d.g), "g_copy is not bit-equal to g"
        assert bool((body[..., Cv * epc:] == ACT_SENTINEL).all()), "g_copy beyond its chunks"
        return dy, dy_ld, gc, sums, da, grads, dal


BWD, BWD_IDS = _expand(BWD_CASES)


# bwd_reduce_rows: Cv = 2 / 4 / 32 / 64 (and 2 at C = 8) the wave-butterfly branch; Cv = 3 (nrow_thr 85), 5 (51), 10 (25) and
# 96 (C = 384 fp32: nrow_thr = 2, threads 192 .. 255 idle) the slot-per-thread branch.  chunk_sweep_bwd: as the forward table.
@pytest.mark.parametrize("kind", ["in", "bn"], ids=["instnorm", "batchnorm"])
@pytest.mark.parametrize("N,C,S,dt,narrow", BWD, ids=BWD_IDS)
def test_backward_reduce_finalize_apply(N, C, S, dt, narrow, kind):
    b = _Bwd(kind, N, C, S, dt, narrow)
    for P in sorted({1, 3, _bwd_row_ranges(S, N, dt)}):
        b.chain(P)


@pytest.mark.parametrize("kind", ["in", "bn"], ids=["instnorm", "batchnorm"])
def test_backward_refuses_fp16(kind):
    b = _Bwd(kind, 2, 8, 3, BF16)
    for run in (lambda: b.reduce(1, dt=F16), lambda: b.apply(b.exact_sums(), dt=F16)):
        with pytest.raises(nat.NativeError, match="CTSEG_F16 is accepted by the forward pass only"):
            run()


def test_batchnorm_statistics_span_the_batch():
    """(3, 256, 315): the float64 dy with the sums taken over the batch against the one with per-sample sums (three N = 1 runs):
    somewhere they lie more than 100 bounds apart, so a kernel that reduced per sample could not pass"""
    for dt in TRAIN2:
        d = _data("bn", 3, 256, 315, dt)
        ref = _bwd_dy(d, F64)
        bound, _ = elem_bound(ref, _bwd_dy(d, F32T), dt)
        apart = float(((ref - _bwd_dy(d, F64, per_sample=True)).abs() / bound).max())
        print(f"batch against per-sample sums, {DT_ID[dt]}: up to {apart:.0f} bounds apart")
        assert apart > 100.0


@pytest.mark.parametrize("kind", ["in", "bn"], ids=["instnorm", "batchnorm"])
@pytest.mark.parametrize("dy_ld", [16, 12])
def test_backward_12_wide_rows(kind, dy_ld):
    """12-wide g and y (8-byte chunks, Cv = 3).  dy 16 wide: the last chunk and the pad columns go out as one 16-byte store
    (store_dy_chunk), columns 10 .. 15 zero; dy 12 wide: nothing beyond column 11 of any row."""
    b = _Bwd(kind, 2, 10, 315, BF16, narrow=True)
    dy = _out_rows(2, 315, dy_ld, BF16)
    b.apply(b.exact_sums(), dy=dy, dy_ld=dy_ld)
    b.check_dy(dy, dy_ld, dy_ld, what=f"{dy_ld}-wide dy")


# P_cap = N: one block per sample (grid cap 1), up to 3 sweep iterations per thread; N * 512: the uncapped grid.  The column sums by
# the butterfly branch (Cv = 2, 4) and the slot-per-thread branch (Cv = 3, 5, 10).  A cap below Cv's odd part is refused.
@pytest.mark.parametrize("cap_per_sample", [1, 512])
@pytest.mark.parametrize("N,C,dt", [(2, 10, BF16), (2, 10, F32), (1, 16, F32), (2, 40, BF16), (2, 40, F32)],
                         ids=["10 bf16", "10 fp32", "16 fp32", "40 bf16", "40 fp32"])
def test_instnorm_bwd_apply_colsum(N, C, dt, cap_per_sample):
    S = 315
    b = _Bwd("in", N, C, S, dt, moved=True)
    epc, Cv = _chunks(dt, C, b.g_ld, b.y_ld)
    p_cap = N * cap_per_sample
    cs_part = torch.full((p_cap + 1, Cv * epc), GRAD_SENTINEL, dtype=torch.float32, device=DEV)
    cs_out = _guarded(rup(C, 4))
    sums = b.exact_sums()
    if _ew_blocks_for(S * Cv, Cv, True, cap_per_sample) == 0:
        with pytest.raises(nat.NativeError, match="partial buffer too small"):
            b.apply(sums, colsum=(cs_part, p_cap, cs_out))
        return
    dy, dy_ld = b.apply(sums, colsum=(cs_part, p_cap, cs_out))
    b.check_dy(dy, dy_ld, Cv * epc)
    dy64, dy32 = b.dy_refs()
    got = cs_out.cpu()
    assert bool((got[C:] == GRAD_SENTINEL).all()), "column sums beyond C"
    assert bool((cs_part[p_cap:] == GRAD_SENTINEL).all()), "partial rows beyond P_cap"
    _check_sums(f"{b.tag} colsum_out P_cap={p_cap}", got[:C], dy64, dy32, (0, 2), N * S)
    s64, a64, _, bound = sum_bound(b.tag, dy64, dy32, (0, 2), N * S)
    assert float((s64.abs() / a64).min()) > 100 * bound, "the moved mean leaves column sums far above the bound"


# ---- the plan's mirror of the same calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["in", "bn"], ids=["_NormAct", "_BatchNormAct"])
def test_emit_bwd_passes_the_same_arguments(kind):
    """_NormAct / _BatchNormAct.emit_bwd on the operands of the direct run: the same three entries, bit-equal results"""
    N, C, S, dt, dims = 2, 10, 315, BF16, (7, 9, 5)
    b = _Bwd(kind, N, C, S, dt)
    dy, dy_ld, _, _, _, grads, dal = b.chain(_bwd_row_ranges(S, N, dt))
    d = b.d
    guards = [torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(8))]
    alpha = torch.nn.Parameter(torch.tensor([ALPHA]))
    if kind == "in":
        plan = MiniPlan([guards[0], alpha, guards[1]], DEV, dt, 3)
        na = _NormAct(plan, alpha)
        want = ["ctseg_instnorm_prelu_bwd_reduce", "ctseg_instnorm_prelu_bwd_finalize", "ctseg_instnorm_prelu_bwd_apply"]
    else:
        bn = torch.nn.BatchNorm3d(C)
        with torch.no_grad():
            bn.weight.copy_(d.gamma.reshape(C))
            bn.bias.copy_(d.beta.reshape(C))
        plan = MiniPlan([guards[0], bn.weight, bn.bias, alpha, guards[1]], DEV, dt, 3)
        plan.bn_train = True
        na = _BatchNormAct(plan, bn, alpha)
        want = ["ctseg_batchnorm_prelu_bwd_reduce", "ctseg_batchnorm_prelu_bwd_finalize", "ctseg_batchnorm_prelu_bwd_apply"]
    na.y, na.mr = to_cl(d.y.reshape(N, C, *dims), dt, DEV), b.mr
    ga, gc = to_cl(d.g.reshape(N, C, *dims), dt, DEV), to_cl(torch.ones(N, C, *dims), dt, DEV)
    plan.store.flat_g.fill_(GRAD_SENTINEL)
    out = na.emit_bwd(ga, g_copy=gc)
    assert [p[0] for p in plan.prog] == want
    Plan.run(plan.prog, nat.stream_ptr())            # (no packed conv operands in this plan: nothing for MiniPlan.run to refresh)
    _sync()
    direct = dy.float().cpu()[:N * S * dy_ld].view(N, S, dy_ld)[..., :C]
    assert torch.equal(out.t.float().cpu().reshape(N, S, -1)[..., :C], direct), "dy"
    assert bool((out.t[..., C:] == 0).all())
    assert torch.equal(from_cl(gc).reshape(N, C, S), d.g), "g_copy"
    st = plan.store
    assert torch.equal(st.grad_view(alpha).cpu(), dal[:1].cpu()), "d alpha"
    written = [alpha]
    if kind == "bn":
        assert torch.equal(st.grad_view(bn.weight).cpu(), grads[:C].cpu()), "d gamma"
        assert torch.equal(st.grad_view(bn.bias).cpu(), grads[C + 4:2 * C + 4].cpu()), "d beta"
        written += [bn.weight, bn.bias]
    keep = torch.ones(st.flat_g.numel(), dtype=torch.bool)
    for p in written:
        keep[st.off(p):st.off(p) + p.numel()] = False
    assert bool((st.flat_g.cpu()[keep] == GRAD_SENTINEL).all()), "the flat gradient outside the node's parameters"


# =================================================================================================================================
# 4. BatchNorm through the plan node, statistics from a conv epilogue
# =================================================================================================================================
@pytest.mark.parametrize("dt", TRAIN2, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [10, 32])
def test_batchnorm_plan_node(C, dt):
    N, dims, S = 2, (7, 9, 5), 315
    M = N * S
    g = torch.Generator().manual_seed(C + 100 * dt)
    x = rounded(torch.randn(N, C, *dims, generator=g) * 1.5 + 0.3, TDT[dt])
    gy = rounded(torch.randn(N, C, *dims, generator=g), TDT[dt])
    res = rounded(torch.randn(N, C, *dims, generator=g), TDT[dt])
    conv, bn, act = torch.nn.Conv3d(C, C, 1), torch.nn.BatchNorm3d(C, momentum=0.25), torch.nn.PReLU()
    with torch.no_grad():
        conv.weight.copy_(torch.eye(C).reshape(C, C, 1, 1, 1))     # identity: the statistics come out of a conv epilogue
        conv.bias.zero_()
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.weight[1], bn.weight[C - 1] = 2.0 ** -6, -0.75
        bn.bias.copy_(0.3 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
        act.weight.fill_(ALPHA)
    gam, bet = bn.weight.detach().clone().reshape(1, C, 1), bn.bias.detach().clone().reshape(1, C, 1)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    # the kink condition needs the table the device will compute: the float64 statistics stand in for it while elements are moved
    # (a 1.5 x margin), and the condition itself is asserted below on the table the kernels wrote
    for rounds in range(9):
        xd = x.double()
        m, r = xd.mean((0, 2, 3, 4), keepdim=True), (xd.var((0, 2, 3, 4), unbiased=False, keepdim=True) + EPS).rsqrt()
        near = (gam.reshape(1, C, 1, 1, 1).double() * (xd - m) * r + bet.reshape(1, C, 1, 1, 1).double()).abs() < 1.5 * KINK
        if not bool(near.any()):
            break
        assert rounds < 8
        x = rounded(torch.where(near, x + 0.25, x), TDT[dt])
    plan = MiniPlan([conv.weight, conv.bias, bn.weight, bn.bias, act.weight], DEV, dt, 3)
    plan.bn_train = True
    plan.engine = types.SimpleNamespace(bufs=BufferStore([bn], plan.device))
    layer = GemmLayer(plan, "id", False, 1, 1, C, [(conv.weight, conv.bias, C)], C)
    plan.packer.finalize()
    y, stats = layer.emit_fwd(to_cl(x, dt, DEV), want_stats=True)
    ra = to_cl(res, dt, DEV)
    na = _BatchNormAct(plan, bn, act.weight)
    out = na.emit_fwd(y, stats, 0, ra, None)
    prog = list(plan.prog)
    plan.run()
    _sync()
    assert int(bn.num_batches_tracked) == 1
    yv = from_cl(y).reshape(N, C, S)                 # what the passes normalise: the identity conv's stored output
    # statistics: float64 on the stored y, the partial-sum bounds of test_gpu_conv_extras.py carried through
    yb = yv.permute(1, 0, 2).reshape(1, C, M)
    s64, a64, live, bs = sum_bound("sum", yb.double(), yb, (2,), M)
    q64, _, liveq, bq = sum_bound("sumsq", yb.double() * yb.double(), yb * yb, (2,), M)
    assert bool(live.all()) and bool(liveq.all()), "a channel of zeros"
    mean64, ey2, eabs = s64[0] / M, q64[0] / M, a64[0] / M
    var64 = ey2 - mean64 * mean64
    rstd64 = (var64 + EPS).rsqrt()
    f32 = 2.0 ** -23
    tol_mean = bs * eabs + f32 * mean64.abs()
    tol_var = bq * ey2 + 2.0 * mean64.abs() * bs * eabs + (bs * eabs) ** 2
    tol_rstd = rstd64 * (0.5 * tol_var / (var64 + EPS) + 4 * f32)
    mr = na.mr.cpu()
    em, er = (mr[:, 0].double() - mean64).abs(), (mr[:, 1].double() - rstd64).abs()
    print(f"mean err / tol {float((em / tol_mean).max()):.3f}, rstd err / tol {float((er / tol_rstd).max()):.3f}")
    assert bool((em <= tol_mean).all()) and bool((er <= tol_rstd).all())
    mom, rel = 0.25, 4 * 2.0 ** -24
    unb64 = var64 * M / (M - 1)
    want_m, want_v = (1 - mom) * rm0 + mom * mean64, (1 - mom) * rv0 + mom * unb64
    erm, erv = (bn.running_mean.cpu().double() - want_m).abs(), (bn.running_var.cpu().double() - want_v).abs()
    tm, tv = mom * tol_mean + rel * want_m.abs(), mom * tol_var * M / (M - 1) + rel * want_v.abs()
    print(f"running_mean err / tol {float((erm / tm).max()):.3f}, running_var err / tol {float((erv / tv).max()):.3f}")
    assert bool((erm <= tm).all()) and bool((erv <= tv).all())
    # the passes as functions of the float32 tables the finalize wrote
    d = types.SimpleNamespace(kind="bn", N=N, C=C, S=S, dt=dt, y=yv, g=gy.reshape(N, C, S), res=res.reshape(N, C, S),
                              m=mr[:, 0].reshape(1, C, 1), r=mr[:, 1].reshape(1, C, 1), gamma=gam, beta=bet)
    xh64 = (d.y.double() - d.m.double()) * d.r.double()
    assert float((gam.double() * xh64 + bet.double()).abs().min()) >= KINK

    def fwd(T, sc, sh):
        z = d.y.to(T) * sc.to(T) + sh.to(T)
        return torch.where(z > 0, z, _al(T) * z) + d.res.to(T)
    sc64 = gam.double() * d.r.double()
    sh64 = bet.double() - d.m.double() * sc64
    tag = f"plan node C={C} {DT_ID[dt]}"
    check_elems(f"{tag} out", from_cl(out).reshape(N, C, S), fwd(F64, sc64, sh64), fwd(F32T, sc64.float(), sh64.float()), dt)
    assert bool((out.t[..., C:] == 0).all())
    ga, gc = to_cl(gy, dt, DEV), to_cl(torch.ones_like(gy), dt, DEV)
    dy = na.emit_bwd(ga, g_copy=gc)
    plan.run()
    _sync()
    check_elems(f"{tag} dy", from_cl(dy).reshape(N, C, S), _bwd_dy(d, F64), _bwd_dy(d, F32T), dt)
    assert bool((dy.t[..., C:] == 0).all())
    assert torch.equal(from_cl(gc), gy), "g_copy"
    t64, t32, st = _bwd_terms(d, F64)[2], _bwd_terms(d, F32T)[2], plan.store
    _check_sums(f"{tag} d beta", st.grad_view(bn.bias), t64[0], t32[0], (0, 2), M)
    _check_sums(f"{tag} d gamma", st.grad_view(bn.weight), t64[1], t32[1], (0, 2), M)
    _check_slope(f"{tag} d alpha", st.grad_view(act.weight), t64[2], t32[2], (0, 2), M)
    # a second forward: the running statistics move again, the count goes to 2
    rm1, rv1 = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    Plan.run(prog, nat.stream_ptr())
    _sync()
    assert int(bn.num_batches_tracked) == 2
    want_m, want_v = (1 - mom) * rm1 + mom * mean64, (1 - mom) * rv1 + mom * unb64
    erm, erv = (bn.running_mean.cpu().double() - want_m).abs(), (bn.running_var.cpu().double() - want_v).abs()
    assert bool((erm <= mom * tol_mean + rel * want_m.abs()).all()) and bool((erv <= mom * tol_var * M / (M - 1) + rel * want_v.abs()).all())
    # eval mode: the table comes from the running statistics, which stay as they are
    rm2, rv2 = bn.running_mean.cpu().clone(), bn.running_var.cpu().clone()
    sc64 = gam.double() / (rv2.double().reshape(1, C, 1) + EPS).sqrt()
    sh64 = bet.double() - rm2.double().reshape(1, C, 1) * sc64
    xe = rounded(torch.randn(N, C, S, generator=g) * 1.5 + 0.3, TDT[dt])
    for rounds in range(9):
        near = (xe.double() * sc64 + sh64).abs() < KINK
        if not bool(near.any()):
            break
        assert rounds < 8
        xe = rounded(torch.where(near, xe + 0.25, xe), TDT[dt])
    assert float((xe.double() * sc64 + sh64).abs().min()) >= KINK
    d.y = xe
    plan.bn_train = False
    ne = _BatchNormAct(plan, bn, act.weight)
    oe = ne.emit_fwd(to_cl(xe.reshape(N, C, *dims), dt, DEV), None, 0, ra, None)
    assert [p[0] for p in plan.prog] == ["ctseg_batchnorm_eval_table", "ctseg_scale_shift_prelu_fwd"]
    plan.run()
    _sync()
    check_elems(f"{tag} eval out", from_cl(oe).reshape(N, C, S), fwd(F64, sc64, sh64), fwd(F32T, sc64.float(), sh64.float()), dt)
    assert torch.equal(bn.running_mean.cpu(), rm2) and torch.equal(bn.running_var.cpu(), rv2) and int(bn.num_batches_tracked) == 2


# =================================================================================================================================
# 5. ctseg_colsum
# =================================================================================================================================
def _colsum(rows, C, dt, P, seed=0):
    g = torch.Generator().manual_seed(rows * 7 + C + seed)
    x = rounded(torch.randn(rows, C, generator=g) * 1.3 + 0.4, TDT[dt])
    epc, Cv = _chunks(dt, C, half_chunks=False)
    ld = Cv * epc + _wide(dt)
    xd = torch.full((rows, ld), POISON, dtype=TDT[dt])
    xd[:, :C] = x.to(TDT[dt])
    xd = xd.to(DEV)
    part = torch.full((P + 1, Cv * epc), GRAD_SENTINEL, dtype=torch.float32, device=DEV)
    out = _guarded(C)
    _call("ctseg_colsum", dt, xd.data_ptr(), ld, rows, C, part.data_ptr(), P, out.data_ptr())
    _sync()
    assert bool((part[P:] == GRAD_SENTINEL).all()) and bool((out[C:] == GRAD_SENTINEL).all())
    return x, out[:C].cpu()


# colsum_partial_kernel: Cv = 2 .. 64 chunks, 128 .. 4 row threads; P = 64 leaves ranges without a row at 1 and 315 rows.
# colsum_final_kernel: 64 (pld 16) .. 4 (pld 256) sub-sums per column.
@pytest.mark.parametrize("P", [1, 3, 64])
@pytest.mark.parametrize("dt", TRAIN2, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,C", [(315, 10), (315, 40), (1, 8), (4099, 256)])
def test_colsum(rows, C, dt, P):
    x, got = _colsum(rows, C, dt, P)
    if rows == 1:      # a sum of one stored value: the float32 evaluation is exact, the bound is 0 and the result must be the value
        assert torch.equal(got, x[0]), "one row"
        return
    _check_sums(f"colsum {rows}x{C} {DT_ID[dt]} P={P}", got, x.double(), x, (0,), rows)


def test_colsum_width_limit():
    """colsum_final_kernel gives every partial column one of its 1024 threads.  bf16 with 1024 < C <= 2048 passed the launcher's
    Cv <= 256 check with more partial columns than that: the kernel then formed no sub-sum at all and wrote 0 to columns 0 .. 1023.
    The launcher refuses it now; C = 1024 (one sub-sum per column) still sums."""
    with pytest.raises(nat.NativeError, match="the final sum takes at most 1024"):
        _colsum(37, 1032, BF16, 3)
    x, got = _colsum(37, 1024, BF16, 3)
    _check_sums("colsum 37x1024 bf16", got, x.double(), x, (0,), 37)


# =================================================================================================================================
def test_every_norm_export_is_called_here():
    """the norm entries of _native.py, each named by a direct call of this file (the plan-node tests assert the names they record)"""
    src = inspect.getsource(sys.modules[__name__])
    called = set(re.findall(r'_call\(\s*"(ctseg_\w+)"', src))
    norm = {n for n in nat.EXPORTS if n.startswith(("ctseg_instnorm_", "ctseg_batchnorm_")) or n in ("ctseg_scale_shift_prelu_fwd", "ctseg_colsum")}
    assert norm <= called, sorted(norm - called)
