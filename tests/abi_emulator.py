"""CPU emulator of the C ABI in include/ctseg_hip.h — TEST INFRASTRUCTURE.

Interprets the programs recorded by capstone_amd.plan.Plan (and direct engine calls) on host memory
with numpy, so that the host-side logic of the product (tap tables, packed-weight indices, channel
strides and slices, the forward/backward graph, gradient placement) can be checked against the
oracle WITHOUT a GPU.  fp32 storage only.  It is also the per-kernel specification the GPU tests
compare the HIP kernels with.  Never imported by the product.
"""
import contextlib
import ctypes
import os

import numpy as np

F32 = 0


def mem(ptr, count, dtype=np.float32):
    if not ptr or count <= 0:
        return None
    nbytes = int(count) * np.dtype(dtype).itemsize
    return np.frombuffer((ctypes.c_char * nbytes).from_address(ptr), dtype=dtype)


def cl_view(ptr, N, X, Y, Z, C, ld, dtype=np.float32):
    """channels-last strided view (N,X,Y,Z,C) of memory starting at ptr with voxel stride ld"""
    nvox = N * X * Y * Z
    flat = mem(ptr, (nvox - 1) * ld + C, dtype)
    it = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat, (N, X, Y, Z, C), (X * Y * Z * ld * it, Y * Z * ld * it, Z * ld * it, ld * it, it))


def _i8(v):
    v &= 255
    return v - 256 if v > 127 else v


def _gather(inp, rowgrid, sin, off):
    """inp (N,Xi,Yi,Zi,C) -> (N,Xr,Yr,Zr,C) with zero fill outside"""
    N, Xi, Yi, Zi, C = inp.shape
    idx, ok = [], []
    for r, s, d in zip(rowgrid, (Xi, Yi, Zi), off):
        i = np.arange(r) * sin + d
        ok.append((i >= 0) & (i < s))
        idx.append(np.clip(i, 0, s - 1))
    g = inp[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]
    m = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    return g * m[None, :, :, :, None]


class Emulator:
    def __init__(self):
        self.conv_tile_rows = lambda cn: 256 if cn <= 32 else 128

    def run(self, prog):
        for name, _, args in prog:
            getattr(self, name[len("ctseg_"):])(*args)

    # ---------------------------------------------------------------------------------------------
    def conv_split_ok(self, d):
        return int(d.nclass == 1 and not d.add and d.out2_col0 % 4 == 0)

    def conv_igemm(self, d):
        assert d.dtype == F32
        N, Cg, Cn, cs = d.N, d.Cg, d.Cn, d.Cn_store
        inp = cl_view(d.in_, N, d.Xi, d.Yi, d.Zi, Cg, d.g_ld)
        out = cl_view(d.out, N, d.Xo, d.Yo, d.Zo, cs, d.o_ld) if not d.out2 else None
        add = cl_view(d.add, N, d.Xo, d.Yo, d.Zo, cs, d.add_ld) if d.add else None
        bias = mem(d.bias, Cn) if d.bias else np.zeros(Cn, np.float32)
        rg = (d.Xr, d.Yr, d.Zr)
        stats = None
        if d.stats:
            stats = mem(d.stats, N * d.stats_tiles * 2 * d.stats_ld).reshape(N, d.stats_tiles, 2, d.stats_ld)
            stats[:] = 0
        for ci in range(d.nclass):
            k = d.cls[ci]
            W = mem(d.w + 4 * k.w_off, Cn * k.kpad).reshape(Cn, k.kpad)
            acc = np.zeros((N,) + rg + (Cn,), np.float32)
            for j in range(k.ntaps):
                tp = k.taps[j]
                off = (_i8(tp), _i8(tp >> 8), _i8(tp >> 16))
                acc += _gather(inp, rg, d.sin, off) @ W[:, j * Cg:(j + 1) * Cg].T
            val = acc + bias
            if stats is not None:
                stats[:, d.stats_tile0, 0, :Cn] += val.sum(axis=(1, 2, 3))
                stats[:, d.stats_tile0, 1, :Cn] += (val * val).sum(axis=(1, 2, 3))
            full = np.zeros((N,) + rg + (cs,), np.float32)
            full[..., :Cn] = val
            sl = (slice(None), slice(k.ox, None, d.sout), slice(k.oy, None, d.sout), slice(k.oz, None, d.sout))
            if d.sout == 1:
                sl = (slice(None), slice(0, d.Xr), slice(0, d.Yr), slice(0, d.Zr))
            else:
                sl = (slice(None), slice(k.ox, k.ox + 2 * d.Xr, 2), slice(k.oy, k.oy + 2 * d.Yr, 2), slice(k.oz, k.oz + 2 * d.Zr, 2))
            if add is not None:
                full = full + add[sl]
            if d.out2:          # split output: columns >= out2_col0 go to the second tensor
                c0 = d.out2_col0
                out_a = cl_view(d.out, N, d.Xo, d.Yo, d.Zo, c0, d.o_ld)
                out_b = cl_view(d.out2, N, d.Xo, d.Yo, d.Zo, cs - c0, d.o2_ld)
                out_a[sl] = full[..., :c0]
                out_b[sl] = full[..., c0:]
            else:
                out[sl] = full
        if d.bst_partials:
            # backward InstanceNorm statistics of the written gradient (ctseg_conv_desc::bst_*): the three sums of
            # instnorm_prelu_bwd_reduce over the values this pass stored, in partial row 0 of every sample
            C, c0 = d.bst_C, d.bst_col0
            if d.out2:
                assert c0 == d.out2_col0
                g = cl_view(d.out2, N, d.Xo, d.Yo, d.Zo, C, d.o2_ld)
            else:
                g = cl_view(d.out, N, d.Xo, d.Yo, d.Zo, cs, d.o_ld)[..., c0:c0 + C]
            yv = cl_view(d.bst_y, N, d.Xo, d.Yo, d.Zo, C, d.bst_y_ld)
            mr = mem(d.bst_mean_rstd, N * C * 2).reshape(N, 1, 1, 1, C, 2)
            a = mem(d.bst_alpha, 1)[0]
            xh = (yv - mr[..., 0]) * mr[..., 1]
            dxh = g * np.where(xh > 0, 1.0, a).astype(np.float32)
            p = mem(d.bst_partials, N * d.bst_P * 3 * d.bst_ld).reshape(N, d.bst_P, 3, d.bst_ld)
            p[:] = 0
            p[:, 0, 0, :C] = dxh.sum(axis=(1, 2, 3))
            p[:, 0, 1, :C] = (dxh * xh).sum(axis=(1, 2, 3))
            p[:, 0, 2, :C] = np.where(xh > 0, 0, g * xh).sum(axis=(1, 2, 3))

    def conv_wgrad(self, d):
        assert d.dtype == F32
        N, Cg, Cn = d.N, d.Cg, d.Cn
        inp = cl_view(d.in_, N, d.Xi, d.Yi, d.Zi, Cg, d.g_ld)
        if d.dyn_g:      # ctseg_wgrad_desc::dyn_*: the upper columns of dY formed from (g, y) of the norm behind them
            c0, C2, S = d.dyn_col0, Cn - d.dyn_col0, d.Xr * d.Yr * d.Zr
            xh, rstd = self._xhat(d.dyn_y, d.dyn_y_ld, d.dyn_mean_rstd, N, S, C2)
            gv = self._rows(d.dyn_g, N, S, C2, d.dyn_g_ld)
            sm = mem(d.dyn_sums, N * C2 * 2).reshape(N, 1, C2, 2)
            dxh = gv * np.where(xh > 0, 1.0, mem(d.dyn_alpha, 1)[0]).astype(np.float32)
            up = (rstd * (dxh - sm[..., 0] - xh * sm[..., 1])).astype(np.float32)
            dy = np.concatenate([self._rows(d.dy, N, S, c0, d.d_ld), up], axis=2).reshape(N, d.Xr, d.Yr, d.Zr, Cn)
        else:
            dy = cl_view(d.dy, N, d.Xr, d.Yr, d.Zr, Cn, d.d_ld)
        ws = mem(d.ws, N * d.splits * d.kpad_w * d.cn_pad).reshape(N * d.splits, d.kpad_w, d.cn_pad)
        ws[:] = 0
        dyf = dy.reshape(-1, Cn)
        for j in range(d.ntaps):
            tp = d.taps[j]
            g = _gather(inp, (d.Xr, d.Yr, d.Zr), d.sin, (_i8(tp), _i8(tp >> 8), _i8(tp >> 16))).reshape(-1, Cg)
            ws[0, j * Cg:(j + 1) * Cg, :Cn] = g.T @ dyf
        ws[0, d.ntaps * Cg, :Cn] = dyf.sum(0)

    def conv_wgrad_reduce(self, ws, nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, dw, db):
        w = mem(ws, nslabs * kpad_w * cn_pad).reshape(nslabs, kpad_w, cn_pad).sum(0)
        r = w[:T * AS, col0:col0 + nb].reshape(T, AS, nb)[:, :A, :]           # [t][a][b]
        mem(dw, nb * A * T)[:] = np.transpose(r, (2, 1, 0)).reshape(-1)      # [b][a][t]
        if db:
            mem(db, nb)[:] = w[T * AS, col0:col0 + nb]

    def conv_wgrad_reduce_batch_ok(self, ws, cn_pad, col0, nb):
        return int(col0 % 4 == 0 and cn_pad % 4 == 0 and col0 + (nb + 3) // 4 * 4 <= cn_pad and ws % 16 == 0)

    def conv_wgrad_reduce_batch(self, jobs, n_jobs, total_blocks):
        """ctseg_conv_wgrad_reduce_batch: the per-pass reduce, job by job (the block bookkeeping is checked against the contract)"""
        import sys
        nat = sys.modules["capstone_amd._native"]
        arr = (nat.ReduceJob * n_jobs).from_address(jobs)
        b0 = 0
        for j in range(n_jobs):
            J = arr[j]
            assert J.lanes == (8 if J.nslabs >= 64 else 32) and J.block0 == b0, (j, J.lanes, J.block0, b0)
            b0 += -(-((J.T * J.Astride + 1) * ((J.nb + 3) // 4)) // J.lanes)
            self.conv_wgrad_reduce(J.ws, J.nslabs, J.kpad_w, J.cn_pad, J.A, J.Astride, J.T, J.col0, J.nb, J.dw, J.db)
        assert b0 == total_blocks, (b0, total_blocks)

    def pack_weights(self, src, blocks, n_blocks, rows, n_rows, dst, dtype):
        """ctseg_pack_weights: the structured re-layout, row by row as the kernel does it"""
        import sys
        nat = sys.modules["capstone_amd._native"]
        assert dtype == F32
        arr = (nat.PackBlock * n_blocks).from_address(blocks)
        rw = mem(rows, 2 * n_rows, np.int32).reshape(n_rows, 2)
        hi = max(int(arr[b].part[k].o + (arr[b].part[k].n_hi - arr[b].part[k].n_lo) * arr[b].part[k].SN +
                     (arr[b].part[k].g_hi - arr[b].part[k].g_lo) * arr[b].part[k].SG + arr[b].T)
                 for b in range(n_blocks) for k in range(arr[b].nparts))
        S = mem(src, hi)
        for b in range(n_blocks):
            B = arr[b]
            mine = rw[rw[:, 0] == b, 1]
            if len(mine) == 0:
                continue
            D = mem(dst + 4 * B.dst_off, (int(mine.max()) + 1) * B.kpad).reshape(-1, B.kpad)
            for n in mine:
                row = np.zeros(B.kpad, np.float32)
                for k in range(B.nparts):
                    P = B.part[k]
                    if P.n_lo <= n < P.n_hi:
                        g = np.arange(P.g_lo, P.g_hi)
                        for j in range(B.ntaps):
                            row[j * B.gs + g] = S[P.o + (n - P.n_lo) * P.SN + (g - P.g_lo) * P.SG + B.tap[j]]
                D[n] = row

    def gather_cast(self, src, idx, dst, dtype, n):
        assert dtype == F32
        i = mem(idx, n, np.int32)
        mem(dst, n)[:] = mem(src, int(i.max()) + 1)[i]

    # ---------------------------------------------------------------------------------------------
    def instnorm_finalize(self, partials, N, P, ld, col0, C, count, eps, scratch, mean_rstd):
        p = mem(partials, N * P * 2 * ld).reshape(N, P, 2, ld).astype(np.float64).sum(1)
        mean = p[:, 0, col0:col0 + C] / count
        var = np.maximum(p[:, 1, col0:col0 + C] / count - mean * mean, 0)
        mr = mem(mean_rstd, N * C * 2).reshape(N, C, 2)
        mr[:, :, 0] = mean
        mr[:, :, 1] = 1.0 / np.sqrt(var + eps)

    @staticmethod
    def _rows(ptr, N, S, C, ld):
        return cl_view(ptr, N, S, 1, 1, C, ld).reshape(N, S, C) if ptr else None

    def instnorm_prelu_fwd(self, dtype, y, y_ld, mean_rstd, alpha, res, res_ld, out, out_ld, N, S, C):
        assert dtype == F32
        Cp = (C + 3) // 4 * 4
        yv = self._rows(y, N, S, C, y_ld).copy()
        if mean_rstd:
            mr = mem(mean_rstd, N * C * 2).reshape(N, 1, C, 2)
            a = mem(alpha, 1)[0]
            yv = (yv - mr[..., 0]) * mr[..., 1]
            yv = np.where(yv > 0, yv, a * yv)
        if res:
            yv = yv + self._rows(res, N, S, C, res_ld)
        o = self._rows(out, N, S, Cp, out_ld)
        o[..., :C] = yv
        o[..., C:] = 0

    def _xhat(self, y, y_ld, mean_rstd, N, S, C):
        mr = mem(mean_rstd, N * C * 2).reshape(N, 1, C, 2)
        return (self._rows(y, N, S, C, y_ld) - mr[..., 0]) * mr[..., 1], mr[..., 1]

    def instnorm_prelu_bwd_reduce(self, dtype, g, g_ld, y, y_ld, mean_rstd, alpha, partials, P, ld, N, S, C):
        xh, _ = self._xhat(y, y_ld, mean_rstd, N, S, C)
        gv = self._rows(g, N, S, C, g_ld)
        a = mem(alpha, 1)[0]
        dxh = gv * np.where(xh > 0, 1.0, a).astype(np.float32)
        p = mem(partials, N * P * 3 * ld).reshape(N, P, 3, ld)
        p[:] = 0
        p[:, 0, 0, :C] = dxh.sum(1)
        p[:, 0, 1, :C] = (dxh * xh).sum(1)
        p[:, 0, 2, :C] = np.where(xh > 0, 0, gv * xh).sum(1)

    def instnorm_prelu_bwd_finalize(self, partials, N, P, ld, C, S, scratch, sums, dalpha):
        p = mem(partials, N * P * 3 * ld).reshape(N, P, 3, ld).astype(np.float64).sum(1)
        s = mem(sums, N * C * 2).reshape(N, C, 2)
        s[:, :, 0] = p[:, 0, :C] / S
        s[:, :, 1] = p[:, 1, :C] / S
        mem(scratch, N * C, np.float64)[:] = p[:, 2, :C].reshape(-1)
        if dalpha:
            mem(dalpha, 1)[0] = p[:, 2, :C].sum()

    def instnorm_prelu_dalpha(self, scratch, NC, dalpha):
        mem(dalpha, 1)[0] = mem(scratch, NC, np.float64).sum()

    def instnorm_prelu_bwd_apply(self, dtype, g, g_ld, y, y_ld, mean_rstd, alpha, sums, dy, dy_ld, g_copy, g_copy_ld, N, S, C,
                                 da_part=None, n_da=0, dalpha=None):
        if da_part:
            mem(dalpha, 1)[0] = mem(da_part, n_da, np.float64).sum()
        xh, rstd = self._xhat(y, y_ld, mean_rstd, N, S, C)
        gv = self._rows(g, N, S, C, g_ld)
        a = mem(alpha, 1)[0]
        s = mem(sums, N * C * 2).reshape(N, 1, C, 2)
        dxh = gv * np.where(xh > 0, 1.0, a).astype(np.float32)
        Cp = (C + 3) // 4 * 4
        o = self._rows(dy, N, S, Cp, dy_ld)
        o[..., :C] = rstd * (dxh - s[..., 0] - xh * s[..., 1])
        o[..., C:] = 0
        if g_copy:
            self._rows(g_copy, N, S, Cp, g_copy_ld)[:] = self._rows(g, N, S, Cp, g_ld)

    def instnorm_prelu_bwd_apply_colsum(self, dtype, g, g_ld, y, y_ld, mean_rstd, alpha, sums, dy, dy_ld, g_copy, g_copy_ld, N, S, C,
                                        cs_part, p_cap, cs_out, da_part=None, n_da=0, dalpha=None):
        self.instnorm_prelu_bwd_apply(dtype, g, g_ld, y, y_ld, mean_rstd, alpha, sums, dy, dy_ld, g_copy, g_copy_ld, N, S, C,
                                      da_part, n_da, dalpha)
        mem(cs_out, C)[:] = self._rows(dy, N, S, C, dy_ld).reshape(-1, C).sum(0, dtype=np.float64)

    def colsum(self, dtype, x, ld, rows, C, partials, P, out):
        mem(out, C)[:] = cl_view(x, 1, rows, 1, 1, C, ld).reshape(rows, C).astype(np.float64).sum(0)

    # ---------------------------------------------------------------------------------------------
    def squash_masks(self, masks, B, K, S, labels, labels_i64, hist):
        m = mem(masks, B * K * S, np.uint8).reshape(B, K, S).astype(np.int64)
        lab = (m * np.arange(1, K + 1)[None, :, None]).max(1)
        mem(labels, B * S, np.uint8)[:] = lab.reshape(-1).astype(np.uint8)
        if labels_i64:
            mem(labels_i64, B * S, np.int64)[:] = lab.reshape(-1)
        if hist:
            h = mem(hist, B * (K + 1), np.int64).reshape(B, K + 1)
            for b in range(B):
                h[b] += np.bincount(lab[b], minlength=K + 1)[:K + 1]

    def seg_loss(self, logits, ld, labels, B, S, C, class_weight, do_stats, part, P, cnt, do_grad, coef, dlogits, g_ld, gdtype,
                 pred_out):
        x = cl_view(logits, B, S, 1, 1, C, ld).reshape(B, S, C)
        t = mem(labels, B * S, np.uint8).reshape(B, S).astype(np.int64)
        cw = mem(class_weight, C) if class_weight else np.ones(C, np.float32)
        m = x.max(-1, keepdims=True)
        e = np.exp(x - m)
        ssum = e.sum(-1, keepdims=True, dtype=np.float32)
        p = e / ssum
        pred = p.argmax(-1)
        ls, m1 = np.log(ssum)[..., 0], m[..., 0]      # the kernels' order: log(sum) + (m - x_t), (x_t - m) - log(sum)
        oh = np.eye(C, dtype=np.float32)[t]
        xt, pt = (x * oh).sum(-1), (p * oh).sum(-1)
        w = cw[t]
        if pred_out:
            mem(pred_out, B * S, np.uint8)[:] = pred.reshape(-1).astype(np.uint8)
        if do_stats:
            R = 2 + 3 * C
            pr = mem(part, B * P * R, np.float64).reshape(B, P, R)
            pr[:] = 0
            pr[:, 0, 0] = (w * (ls + (m1 - xt))).astype(np.float64).sum(1)
            pr[:, 0, 1] = w.astype(np.float64).sum(1)
            pr[:, 0, 2:2 + C] = p.astype(np.float64).sum(1)
            pr[:, 0, 2 + C:2 + 2 * C] = (p * oh).astype(np.float64).sum(1)
            fo = -(1 - pt) ** 2 * ((xt - m1) - ls)
            pr[:, 0, 2 + 2 * C:] = (fo[..., None] * oh).astype(np.float64).sum(1)
            c = mem(cnt, B * 3 * C, np.int64).reshape(B, 3, C)
            ph = np.eye(C, dtype=np.int64)[pred]
            c[:, 0] += (ph * oh.astype(np.int64)).sum(1)
            c[:, 1] += ph.sum(1)
            c[:, 2] += oh.astype(np.int64).sum(1)
        if do_grad:
            assert gdtype == F32
            cf = mem(coef, B * (1 + 3 * C)).reshape(B, 1 + 3 * C)
            a, b, f = cf[:, None, 1:1 + C], cf[:, None, 1 + C:1 + 2 * C], cf[:, None, 1 + 2 * C:]
            gk = b + a * oh
            dot = (gk * p).sum(-1, keepdims=True)
            ft = (f * oh).sum(-1)
            om, logpt = 1 - pt, (xt - m1) - ls
            fterm = ft * (2 * om * pt * logpt - om * om)
            d = cf[:, None, 0:1] * w[..., None] * (p - oh) + p * (gk - dot) + fterm[..., None] * (oh - p)
            o = cl_view(dlogits, B, S, 1, 1, g_ld, g_ld).reshape(B, S, g_ld)
            o[..., :C] = d
            o[..., C:] = 0

    def reduce_partials_f64(self, part, B, P, R, out):
        mem(out, B * R, np.float64)[:] = mem(part, B * P * R, np.float64).reshape(B, P, R).sum(1).reshape(-1)

    def dice_counts(self, pred, truth, B, S, C, cnt):
        p = mem(pred, B * S, np.uint8).reshape(B, S)
        t = mem(truth, B * S, np.uint8).reshape(B, S)
        c = mem(cnt, B * 3 * C, np.int64).reshape(B, 3, C)
        for b in range(B):
            c[b, 1] += np.bincount(p[b], minlength=C)[:C]
            c[b, 2] += np.bincount(t[b], minlength=C)[:C]
            c[b, 0] += np.bincount(p[b][p[b] == t[b]], minlength=C)[:C]

    def adam_step(self, p, g, m, v, n, lr, b1, b2, eps, step, gscale):
        P, G, M, V = (mem(q, n) for q in (p, g, m, v))
        gr = G * np.float32(gscale)
        M[:] = M + (gr - M) * np.float32(1 - b1)
        V[:] = V * np.float32(b2) + np.float32(1 - b2) * gr * gr
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        P[:] = P - np.float32(lr / bc1) * (M / (np.sqrt(V) / np.float32(np.sqrt(bc2)) + np.float32(eps)))

    def scale_inplace(self, x, dtype, n, dev_scale, host_scale):
        assert dtype == 0, "the emulator stores fp32 only"
        f = np.float32(host_scale) * (mem(dev_scale, 1)[0] if dev_scale else np.float32(1))
        if f != 1:
            X = mem(x, n)
            X[:] = X * f

    def cast(self, src, sd, dst, dd, n):
        assert sd == F32 and dd == F32
        mem(dst, n)[:] = mem(src, n)

    def loss_dice_summary(self, red, B, R, cnt, C, out):
        r = mem(red, B * R, np.float64).reshape(B, R)
        c = mem(cnt, B * 3 * C, np.int64).reshape(B, 3, C).astype(np.float32)
        o = mem(out, 1 + C)
        o[0] = np.float32(r[:, 0].sum() / r[:, 1].sum())
        inter, pred, true = c[:, 0, 1:], c[:, 1, 1:], c[:, 2, 1:]
        ok = true > 0
        score = np.where(ok, 2.0 * inter / np.where(ok, true + pred, 1.0), 0.0).astype(np.float32)
        n_ok = ok.sum(0).astype(np.float32)
        pc = np.where(n_ok > 0, score.sum(0) / np.maximum(n_ok, 1), 0.0).astype(np.float32)
        o[2:2 + C - 1] = pc
        o[1] = pc.mean(dtype=np.float32)

    def nc_to_cl(self, src, dst, dtype, N, C, S, ld):
        s = mem(src, N * C * S).reshape(N, C, S)
        d = mem(dst, N * S * ld).reshape(N, S, ld)
        d[:] = 0
        d[..., :C] = np.transpose(s, (0, 2, 1))

    def cl_to_nc(self, src, dtype, dst, N, C, S, ld):
        s = mem(src, N * S * ld).reshape(N, S, ld)
        mem(dst, N * C * S).reshape(N, C, S)[:] = np.transpose(s[..., :C], (0, 2, 1))

    def resize3d_to_hwd(self, image, image_dtype, masks, K, D, H, W, Do, Ho, Wo, window, lo, hi, image_out, masks_out, labels_out, hist):
        def idx(o, i):
            sc = np.float32(i) / np.float32(o)
            return np.minimum(np.floor(np.arange(o, dtype=np.float32) * sc).astype(np.int64), i - 1)
        iD, iH, iW = idx(Do, D), idx(Ho, H), idx(Wo, W)

        def pick(vol):          # (D,H,W) -> (Ho,Wo,Do)
            return np.transpose(vol[iD][:, iH][:, :, iW], (1, 2, 0))
        if image:
            dt = {0: np.float32, 2: np.int16, 3: np.uint8}[image_dtype]
            v = pick(mem(image, D * H * W, dt).reshape(D, H, W)).astype(np.float32)
            if window:
                v = np.clip(v, np.float32(lo), np.float32(hi))
                if window == 2:
                    v = (v - np.float32(lo)) / np.float32(float(hi) - float(lo) + 1e-8)
            mem(image_out, Ho * Wo * Do).reshape(Ho, Wo, Do)[:] = v
        if masks:
            m = mem(masks, K * D * H * W, np.uint8).reshape(K, D, H, W)
            r = np.stack([pick(m[k]) for k in range(K)])
            if masks_out:
                mem(masks_out, K * Ho * Wo * Do, np.uint8).reshape(K, Ho, Wo, Do)[:] = (r != 0)
            if labels_out:
                lab = (r.astype(np.int32) * np.arange(1, K + 1).reshape(K, 1, 1, 1)).max(0)
                mem(labels_out, Ho * Wo * Do, np.uint8).reshape(Ho, Wo, Do)[:] = lab
                if hist:
                    mem(hist, K + 1, np.int64)[:] += np.bincount(lab.reshape(-1), minlength=K + 1)

    def window_gather(self, vol, Cin, X, Y, Z, x0, y0, z0, rx, ry, rz, cval, dst, dtype, ld):
        assert dtype == F32
        v = mem(vol, Cin * X * Y * Z).reshape(Cin, X, Y, Z)
        d = mem(dst, rx * ry * rz * ld).reshape(rx, ry, rz, ld)
        d[:] = 0
        d[..., :Cin] = np.float32(cval)
        xs, ys, zs = (np.arange(r) + o for r, o in ((rx, x0), (ry, y0), (rz, z0)))
        ix, iy, iz = (np.nonzero((a >= 0) & (a < n))[0] for a, n in ((xs, X), (ys, Y), (zs, Z)))
        if len(ix) and len(iy) and len(iz):
            sub = v[:, xs[ix][0]:xs[ix][-1] + 1, ys[iy][0]:ys[iy][-1] + 1, zs[iz][0]:zs[iz][-1] + 1]
            d[ix[0]:ix[-1] + 1, iy[0]:iy[-1] + 1, iz[0]:iz[-1] + 1, :Cin] = np.moveaxis(sub, 0, -1)

    def window_gather_batch(self, vol, Cin, X, Y, Z, starts, nw, rx, ry, rz, cval, dst, dtype, ld):
        st = mem(starts, nw * 3, np.int32).reshape(nw, 3)
        for w in range(nw):
            self.window_gather(vol, Cin, X, Y, Z, int(st[w, 0]), int(st[w, 1]), int(st[w, 2]), rx, ry, rz, cval,
                               dst + w * rx * ry * rz * ld * 4, dtype, ld)

    def window_blend_batch(self, logits, ld, C, rx, ry, rz, starts, nw, imp, inv_count, out, X, Y, Z, out_ld, bbox=None):
        st = mem(starts, nw * 3, np.int32).reshape(nw, 3)
        for w in range(nw):
            self.window_blend(logits + w * rx * ry * rz * ld * 4, ld, C, rx, ry, rz, int(st[w, 0]), int(st[w, 1]), int(st[w, 2]), imp,
                              inv_count, out, X, Y, Z, out_ld)

    def window_blend(self, logits, ld, C, rx, ry, rz, x0, y0, z0, imp, inv_count, out, X, Y, Z, out_ld):
        l = mem(logits, rx * ry * rz * ld).reshape(rx, ry, rz, ld)
        w = mem(imp, rx * ry * rz).reshape(rx, ry, rz)
        ic = mem(inv_count, X * Y * Z).reshape(X, Y, Z) if inv_count else np.ones((X, Y, Z), np.float32)
        o = mem(out, X * Y * Z * out_ld).reshape(X, Y, Z, out_ld)
        for x in range(rx):
            gx = x0 + x
            if not 0 <= gx < X:
                continue
            for y in range(ry):
                gy = y0 + y
                if not 0 <= gy < Y:
                    continue
                zlo, zhi = max(0, -z0), min(rz, Z - z0)
                if zhi > zlo:
                    wn = w[x, y, zlo:zhi] * ic[gx, gy, z0 + zlo:z0 + zhi]
                    o[gx, gy, z0 + zlo:z0 + zhi, :C] += wn[:, None] * l[x, y, zlo:zhi, :C]


def patch_native(nat, emu):
    """route capstone_amd._native.call (direct engine calls) through the emulator; returns an undo callable"""
    orig_call, orig_stream = nat.call, nat.stream_ptr
    nat.call = lambda name, *args: getattr(emu, name[len("ctseg_"):])(*args)
    nat.stream_ptr = lambda: None
    orig_req = nat.require_gpu
    nat.require_gpu = lambda t, what: None
    orig_query = nat.query
    own = {"ctseg_conv_split_ok": emu.conv_split_ok, "ctseg_conv_narrow_ok": lambda d: 0, "ctseg_wgrad_narrow_ok": lambda d: 0,
           "ctseg_conv_bwd_stats_slots": lambda d: 1,
           # (the library offers dY-on-load for bf16 storage only; the emulated fp32 plans take the branch so that its host logic runs)
           "ctseg_wgrad_dy_norm_ok": lambda d: 1 if os.environ.get("CTSEG_EMU_WGRAD_DYN", "1") == "1" else 0}
    nat.query = lambda name, d: own[name](d) if name in own else orig_query(name, d)

    def undo():
        nat.call, nat.stream_ptr, nat.require_gpu, nat.query = orig_call, orig_stream, orig_req, orig_query
    return undo


@contextlib.contextmanager
def emulated(e, plan_run=True):
    """the C ABI routed through emulator ``e``: direct engine calls (patch_native) and, with ``plan_run``, recorded programs too
    (Plan.run); yields ``e`` and restores both in reverse order"""
    from capstone_amd import _native as nat
    from capstone_amd import plan as plan_mod
    undo = patch_native(nat, e)
    if plan_run:
        orig = plan_mod.Plan.__dict__["run"]         # the staticmethod itself: restoring the bare function would bind self
        plan_mod.Plan.run = staticmethod(lambda prog, stream, lo=0, hi=None: e.run(prog[lo:hi]))
    try:
        yield e
    finally:
        if plan_run:
            plan_mod.Plan.run = orig
        undo()
