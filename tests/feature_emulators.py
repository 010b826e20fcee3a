"""Entry-point emulators of the feature families, as mixins for tests/abi_emulator.Emulator: TEST INFRASTRUCTURE.

Each class holds the entries of one family of include/ctseg_hip.h on host memory and inherits from nothing; an entry that has a
numpy oracle IS that oracle (distance_oracles, plane_oracles, resample_oracles).  A test module states what it needs in one line,

    class E(Augment3dEntries, Distmap3dEntries, Emulator): pass

Families that count their launches keep a counter of their own: ``distmap2d_calls``, ``distmap3d_calls``, and ``calls`` for the
stages of the surface metrics and of the components, which run as one launch group and are counted as one.
"""
import numpy as np

from abi_emulator import cl_view, mem
from capstone_amd import _native as nat
from capstone_amd import components, surface
from component_oracles import keep_oracle, label_oracle
from distance_oracles import d2w_to, ranks, separable_d2_to, surface_of
from distance_oracles import oracle as distance_oracle
from distance_oracles import signed_map
from plane_oracles import ELASTIC, F32, F64, GRID, I64, NP_OF_CODE, oracle_batch, r_batch, r_fields
from resample_oracles import NP_DT, deformed, displacement, lattice_oracle, oracle_accumulate, oracle_finish
from resample_oracles import oracle as resample_oracle


class MixupEntries:
    """the three mixup entries: the pair pass as two runs of the emulated single-target pass"""

    def squash_masks_present(self, masks, B, K, S, labels, labels_i64, hist, present):
        self.squash_masks(masks, B, K, S, labels, labels_i64, hist)
        m = mem(masks, B * K * S, np.uint8).reshape(B, K, S)
        mem(present, B * K, np.int32).reshape(B, K)[:] |= (m == 1).any(2)

    def mixup_images(self, x, perm, B, n, lam, out):
        xs = mem(x, B * n).reshape(B, n)
        l0, l1 = np.float32(lam), np.float32(1.0 - lam)
        mem(out, B * n).reshape(B, n)[:] = l0 * xs + l1 * xs[np.clip(mem(perm, B, np.int32), 0, B - 1)]

    def seg_loss_pair(self, logits, ld, labels, perm, B, S, C, class_weight, do_grad, part, P, cnt, coef, dlogits, g_ld, gdtype):
        lab = mem(labels, B * S, np.uint8).reshape(B, S)
        sides = [np.ascontiguousarray(lab), np.ascontiguousarray(lab[np.clip(mem(perm, B, np.int32), 0, B - 1)])]
        cw = [np.ascontiguousarray(r) for r in mem(class_weight, 2 * C).reshape(2, C)] if class_weight else [None, None]
        R = 2 + 3 * C
        if not do_grad:
            pr = mem(part, B * P * 2 * R, np.float64).reshape(B, P, 2, R)
            c = mem(cnt, B * 2 * 3 * C, np.int64).reshape(B, 2, 3, C)
            for s in (0, 1):
                p1, c1 = np.zeros((B, P, R)), np.zeros((B, 3, C), np.int64)
                self.seg_loss(logits, ld, sides[s].ctypes.data, B, S, C, cw[s].ctypes.data if cw[s] is not None else None, 1,
                              p1.ctypes.data, P, c1.ctypes.data, 0, None, None, 0, nat.F32, None)
                pr[:, :, s] = p1
                c[:, s] += c1
            return
        assert gdtype == nat.F32
        cf = mem(coef, B * 2 * (1 + 3 * C)).reshape(B, 2, 1 + 3 * C)
        total = np.zeros((B, S, g_ld), np.float32)
        for s in (0, 1):
            d1, cfs = np.zeros((B, S, g_ld), np.float32), np.ascontiguousarray(cf[:, s])
            self.seg_loss(logits, ld, sides[s].ctypes.data, B, S, C, cw[s].ctypes.data if cw[s] is not None else None, 0, None, P,
                          None, 1, cfs.ctypes.data, d1.ctypes.data, g_ld, nat.F32, None)
            total += d1
        cl_view(dlogits, B, S, 1, 1, g_ld, g_ld).reshape(B, S, g_ld)[:] = total


class BoundaryEntries:
    """ctseg_boundary_stats / ctseg_boundary_grad in float64 numpy"""

    @staticmethod
    def _inputs(logits, ld, maps, perm, B, S, C):
        x = cl_view(logits, B, S, 1, 1, C, ld).reshape(B, S, C).astype(np.float64)
        e = np.exp(x - x.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        D = mem(maps, B * (C - 1) * S).reshape(B, C - 1, S).astype(np.float64)
        sides = [D] if not perm else [D, D[np.clip(mem(perm, B, np.int32), 0, B - 1)]]
        return p, sides

    def boundary_stats(self, logits, ld, maps, perm, B, S, C, part, P):
        p, sides = self._inputs(logits, ld, maps, perm, B, S, C)
        ns = len(sides)
        pr = mem(part, B * P * ns * (C - 1), np.float64).reshape(B, P, ns, C - 1)
        pr[:] = 0
        for s, D in enumerate(sides):
            pr[:, 0, s] = (np.transpose(p[..., 1:], (0, 2, 1)) * D).sum(-1)

    def boundary_grad(self, logits, ld, maps, perm, B, S, C, bw, P, dlogits, g_ld, gdtype, accumulate):
        assert gdtype == nat.F32
        p, sides = self._inputs(logits, ld, maps, perm, B, S, C)
        ns = len(sides)
        w = mem(bw, B * ns * (C - 1)).reshape(B, ns, C - 1).astype(np.float64)
        g = np.zeros((B, S, C))
        for s, D in enumerate(sides):
            g[..., 1:] += np.transpose(w[:, s, :, None] * D, (0, 2, 1))
        d = p * (g - (g * p).sum(-1, keepdims=True))
        o = cl_view(dlogits, B, S, 1, 1, g_ld, g_ld).reshape(B, S, g_ld)
        if accumulate:
            o[..., :C] += d.astype(np.float32)
        else:
            o[..., :C] = d
            o[..., C:] = 0


class BatchNormEntries:
    """the BatchNorm entry points of include/ctseg_hip.h on host memory (fp32 storage), in their specified arithmetic"""

    def batchnorm_finalize(self, partials, N, P, ld, col0, C, count, eps, momentum, gamma, beta, rm, rv, nbt, mean_rstd, ss):
        p = mem(partials, N * P * 2 * ld).reshape(N * P, 2, ld).astype(np.float64).sum(0)
        mean = p[0, col0:col0 + C] / count
        var = np.maximum(p[1, col0:col0 + C] / count - mean * mean, 0)
        rstd = 1.0 / np.sqrt(var + eps)
        g, b = mem(gamma, C).astype(np.float64), mem(beta, C).astype(np.float64)
        mr, t = mem(mean_rstd, 2 * C).reshape(C, 2), mem(ss, 2 * C).reshape(C, 2)
        mr[:, 0], mr[:, 1] = mean, rstd
        t[:, 0], t[:, 1] = g * rstd, b - mean * g * rstd
        r_m, r_v = mem(rm, C), mem(rv, C)
        r_m[:] = (1 - momentum) * r_m + momentum * mean
        r_v[:] = (1 - momentum) * r_v + momentum * var * count / (count - 1)
        mem(nbt, 1, np.int64)[0] += 1

    def batchnorm_eval_table(self, rm, rv, gamma, beta, C, eps, ss):
        sc = mem(gamma, C).astype(np.float64) / np.sqrt(mem(rv, C).astype(np.float64) + eps)
        t = mem(ss, 2 * C).reshape(C, 2)
        t[:, 0], t[:, 1] = sc, mem(beta, C) - mem(rm, C) * sc

    def scale_shift_prelu_fwd(self, dtype, y, y_ld, ss, alpha, res, res_ld, out, out_ld, N, S, C):
        assert dtype == nat.F32
        t = mem(ss, 2 * C).reshape(C, 2)
        z = self._rows(y, N, S, C, y_ld) * t[:, 0] + t[:, 1]
        z = np.where(z > 0, z, mem(alpha, 1)[0] * z)
        if res:
            z = z + self._rows(res, N, S, C, res_ld)
        o = self._rows(out, N, S, (C + 3) // 4 * 4, out_ld)
        o[..., :C] = z
        o[..., C:] = 0

    def _bn(self, g, g_ld, y, y_ld, mean_rstd, gamma, beta, alpha, N, S, C):
        mr = mem(mean_rstd, 2 * C).reshape(C, 2)
        xh = (self._rows(y, N, S, C, y_ld) - mr[:, 0]) * mr[:, 1]
        z = mem(gamma, C) * xh + mem(beta, C)
        gv = self._rows(g, N, S, C, g_ld)
        return xh, z, gv, gv * np.where(z > 0, 1.0, mem(alpha, 1)[0]).astype(np.float32), mr[:, 1]

    def batchnorm_prelu_bwd_reduce(self, dtype, g, g_ld, y, y_ld, mean_rstd, gamma, beta, alpha, partials, P, ld, N, S, C):
        xh, z, gv, dz, _ = self._bn(g, g_ld, y, y_ld, mean_rstd, gamma, beta, alpha, N, S, C)
        p = mem(partials, N * P * 3 * ld).reshape(N, P, 3, ld)
        p[:] = 0
        p[:, 0, 0, :C] = dz.sum(1)
        p[:, 0, 1, :C] = (dz * xh).sum(1)
        p[:, 0, 2, :C] = np.where(z > 0, 0, gv * z).sum(1)

    def batchnorm_prelu_bwd_finalize(self, partials, N, P, ld, C, count, sums, dgamma, dbeta, da_part):
        p = mem(partials, N * P * 3 * ld).reshape(N * P, 3, ld).astype(np.float64).sum(0)
        s = mem(sums, 2 * C).reshape(C, 2)
        s[:, 0], s[:, 1] = p[0, :C] / count, p[1, :C] / count
        mem(dbeta, C)[:], mem(dgamma, C)[:] = p[0, :C], p[1, :C]
        mem(da_part, C, np.float64)[:] = p[2, :C]

    def batchnorm_prelu_bwd_apply(self, dtype, g, g_ld, y, y_ld, mean_rstd, gamma, beta, alpha, sums, dy, dy_ld, g_copy, g_copy_ld,
                                  N, S, C, da_part, n_da, dalpha):
        if da_part:
            mem(dalpha, 1)[0] = mem(da_part, n_da, np.float64).sum()
        xh, z, gv, dz, rstd = self._bn(g, g_ld, y, y_ld, mean_rstd, gamma, beta, alpha, N, S, C)
        s = mem(sums, 2 * C).reshape(C, 2)
        Cp = (C + 3) // 4 * 4
        o = self._rows(dy, N, S, Cp, dy_ld)
        o[..., :C] = mem(gamma, C) * rstd * (dz - s[:, 0] - xh * s[:, 1])
        o[..., C:] = 0
        if g_copy:
            self._rows(g_copy, N, S, Cp, g_copy_ld)[:] = self._rows(g, N, S, Cp, g_ld)


class Pipeline2dEntries:
    """ctseg_pipeline2d_batch: plane_oracles.oracle_batch on the stores the table points into"""

    def pipeline2d_batch(self, image_store, dtype, image_elems, mask_store, mask_bytes, table, table_host, B, K, mode, Ho, Wo, C,
                         win_lo, win_hi, shift, mean, denom, image_out, masks_out, labels_out, hist, present):
        t = mem(table_host, B * 8, np.int64).reshape(B, 8)
        assert np.array_equal(t, mem(table, B * 8, np.int64).reshape(B, 8))
        if mode == 0 and Ho != Wo and (t[:, 6] & 1).any():
            raise nat.NativeError("pipeline2d_batch: rot90 by an odd k needs a square output")
        store = mem(image_store, image_elems, NP_OF_CODE[dtype]) if image_store else None
        mstore = mem(mask_store, mask_bytes, np.uint8) if mask_store else None
        raws, masks = [], ([] if mask_store else None)
        for io, mo, H, W in t[:, :4]:
            raws.append(store[io:io + H * W].reshape(H, W) if store is not None else np.zeros((H, W), np.float32))
            if mask_store:
                masks.append(mstore[mo:mo + K * H * W].reshape(K, H, W))
        # windows back from (lo, hi): width = hi - lo (even in every preset), level = lo + width // 2
        windows = [(int(h - l), int(l) + int(h - l) // 2) for l, h in zip(list(win_lo or []), list(win_hi or []))] or [(2, 1)]
        rows = [(b,) + tuple(int(v) for v in t[b, 4:]) for b in range(B)]
        o = oracle_batch(raws, masks, rows, "crop" if mode == 0 else "resize", (Ho, Wo), windows, bool(shift),
                         list(mean) if mean else None, list(denom) if mean else None)
        if image_out:
            mem(image_out, B * C * Ho * Wo).reshape(B, C, Ho, Wo)[:] = o["image"]
        if masks_out:
            mem(masks_out, B * K * Ho * Wo, np.uint8).reshape(B, K, Ho, Wo)[:] = o["masks"]
        if labels_out:
            mem(labels_out, B * Ho * Wo, np.uint8).reshape(B, Ho, Wo)[:] = o["labels"]
        if hist:
            mem(hist, B * (K + 1), np.int64).reshape(B, K + 1)[:] += o["hist"][:, :K + 1]
        if present:
            mem(present, B * K, np.int32).reshape(B, K)[:] |= o["present"]


class Warp2dEntries:
    """ctseg_pipeline2d_warp_batch: plane_oracles.r_batch (and r_fields for the fields launch)"""

    def pipeline2d_warp_batch(self, image_store, dtype, image_elems, mask_store, mask_bytes, table, table_host, B, K, Ho, Wo, C, win_lo,
                              win_hi, shift, mean, denom, gauss_w, radius, alpha, xx, xx_elems, yy, yy_elems, fields, field_tmp, n_slots,
                              inter, inter_bytes, image_out, masks_out, labels_out, hist, present, launches):
        t = mem(table_host, B * 19, I64).reshape(B, 19)
        assert np.array_equal(t, mem(table, B * 19, I64).reshape(B, 19))
        assert inter and inter_bytes >= B * (C * 8 + (K if mask_store else 0)) * Ho * Wo
        if Ho != Wo and (t[:, 6] & 1).any():
            raise nat.NativeError("pipeline2d_warp_batch: rot90 by an odd k needs a square output")
        if ((t[:, 4] < 0) | (t[:, 5] < 0) | (t[:, 4] + Ho > t[:, 2]) | (t[:, 5] + Wo > t[:, 3])).any():
            raise nat.NativeError("pipeline2d_warp_batch: crop leaves the slice")
        store = mem(image_store, image_elems, NP_OF_CODE[dtype])
        mstore = mem(mask_store, mask_bytes, np.uint8) if mask_store else None
        gw = mem(gauss_w, radius + 1, F64) if gauss_w else None
        xs, ys = mem(xx, xx_elems, F32), mem(yy, yy_elems, F32)
        raws, masks, samples = [], ([] if mask_store else None), []
        for b, r in enumerate(t):
            io, mo, H, W = r[:4]
            raws.append(store[io:io + H * W].reshape(H, W))
            if mask_store:
                masks.append(mstore[mo:mo + K * H * W].reshape(K, H, W))
            s = dict(i=b, y0=int(r[4]), x0=int(r[5]), k=int(r[6]), flip=int(r[7]), kind=int(r[8]))
            if s["kind"] == ELASTIC:
                s.update(minv=r[10:16].copy().view(F64), seed=int(r[9:10].view(np.uint64)[0]))
                if launches & 1:
                    f = mem(fields, n_slots * 2 * Ho * Wo, F32).reshape(n_slots, 2, Ho, Wo)
                    f[r[18]] = np.stack(r_fields(s["seed"], Ho, Wo, gw, alpha))
            elif s["kind"] == GRID:
                s.update(xx=xs[r[16]:r[16] + Wo], yy=ys[r[17]:r[17] + Ho])
            samples.append(s)
        if not launches & 4:
            return
        windows = [(int(h - l), int(l) + int(h - l) // 2) for l, h in zip(list(win_lo), list(win_hi))]
        o = r_batch(raws, masks, samples, (Ho, Wo), windows, bool(shift), list(mean) if mean else None, list(denom) if mean else None, gw, alpha)
        mem(image_out, B * C * Ho * Wo).reshape(B, C, Ho, Wo)[:] = o["image"]
        if masks_out:
            mem(masks_out, B * K * Ho * Wo, np.uint8).reshape(B, K, Ho, Wo)[:] = o["masks"]
        if labels_out:
            mem(labels_out, B * Ho * Wo, np.uint8).reshape(B, Ho, Wo)[:] = o["labels"]
        if hist:
            mem(hist, B * (K + 1), I64).reshape(B, K + 1)[:] += o["hist"][:, :K + 1]
        if present:
            mem(present, B * K, np.int32).reshape(B, K)[:] |= o["present"]


class Distmap2dEntries:
    """ctseg_distmap2d_batch IS distance_oracles.oracle on planes"""
    distmap2d_calls = 0

    def distmap2d_batch(self, masks, P, H, W, mode, table, workspace, workspace_bytes, out, d2_fg, d2_bg):
        assert masks and table and workspace and out and workspace_bytes >= 4 * P * H * W and mode in (0, 1)
        assert np.array_equal(mem(table, 256), np.float32(np.arange(256) / 255.0))
        planes = mem(masks, P * H * W, np.uint8).reshape(P, H, W)
        d2f, d2b, ref = distance_oracle(planes, 2)
        mem(out, P * H * W).reshape(P, H, W)[:] = ref if mode == 0 else signed_map(planes, d2f, d2b, 2)
        if d2_fg:
            mem(d2_fg, P * H * W, np.int32).reshape(P, H, W)[:] = d2f
        if d2_bg:
            mem(d2_bg, P * H * W, np.int32).reshape(P, H, W)[:] = d2b
        self.distmap2d_calls += 1


class Distmap3dEntries:
    """ctseg_distmap3d_batch IS distance_oracles.oracle on volumes"""
    distmap3d_calls = 0

    def distmap3d_batch(self, masks, P, X, Y, Z, mode, table, workspace, workspace_bytes, out, d2_fg, d2_bg):
        n = P * X * Y * Z
        assert masks and table and workspace and out and workspace_bytes >= 6 * n and mode in (0, 1)
        assert np.array_equal(mem(table, 256), np.float32(np.arange(256) / 255.0))
        vols = mem(masks, n, np.uint8).reshape(P, X, Y, Z)
        d2f, d2b, ref = distance_oracle(vols, 3)
        mem(out, n).reshape(P, X, Y, Z)[:] = ref if mode == 0 else signed_map(vols, d2f, d2b, 3)
        if d2_fg:
            mem(d2_fg, n, np.int32).reshape(P, X, Y, Z)[:] = d2f
        if d2_bg:
            mem(d2_bg, n, np.int32).reshape(P, X, Y, Z)[:] = d2b
        self.distmap3d_calls += 1


class Augment3dEntries:
    """ctseg_augment3d_to_hwd IS resample_oracles.oracle (the plain resize is the base emulator's own)"""

    def augment3d_to_hwd(self, image, image_dtype, masks, Kn, D, H, W, Do, Ho, Wo, matrix, interp, border, cval, mask_src, window,
                         lo, hi, gain, bias, image_out, masks_out, labels_out, hist):
        A = mem(matrix, 12).reshape(3, 4).copy()
        src = mem(mask_src, Kn, np.int32).tolist() if mask_src else None
        assert np.isfinite(A).all() and interp in (0, 1) and border in (0, 1) and (src is None or sorted(src) == list(range(Kn)))
        im = mem(image, D * H * W, NP_DT[image_dtype]).reshape(D, H, W) if image else None
        m = mem(masks, Kn * D * H * W, np.uint8).reshape(Kn, D, H, W) if masks else None
        img, mo, lab, hs, _ = resample_oracle(im, m, (Do, Ho, Wo), A, interp, border, cval, src, window, lo, hi, gain, bias)
        if image:
            mem(image_out, Ho * Wo * Do).reshape(Ho, Wo, Do)[:] = img
        if masks_out:
            mem(masks_out, Kn * Ho * Wo * Do, np.uint8).reshape(Kn, Ho, Wo, Do)[:] = mo
        if labels_out:
            mem(labels_out, Ho * Wo * Do, np.uint8).reshape(Ho, Wo, Do)[:] = lab
            if hist:
                mem(hist, Kn + 1, np.int64)[:] += hs


class Deform3dEntries:
    """ctseg_deform3d_lattice and ctseg_augment3d_deform_to_hwd; the second runs the affine entry (Augment3dEntries) under the
    displacement"""

    def deform3d_lattice(self, seed, cells, magnitude, lattice, lattice_elems):
        G, m = mem(cells, 3, np.int32).tolist(), mem(magnitude, 3).tolist()
        assert all(g >= 1 for g in G) and all(np.isfinite(v) and v >= 0 for v in m)
        L = lattice_oracle(seed, G, m)
        assert lattice_elems == L.size
        mem(lattice, L.size)[:] = L.reshape(-1)

    def augment3d_deform_to_hwd(self, *args):
        *affine, lattice, cells = args
        size, G = tuple(affine[7:10]), mem(cells, 3, np.int32).tolist()
        assert lattice and all(g >= 1 and (1 if a == 1 else 4) * g <= n for a, (g, n) in enumerate(zip(G, size)))
        n = [g + 3 for g in G]
        with deformed(displacement(size, G, mem(lattice, 3 * n[0] * n[1] * n[2]).reshape(3, *n).copy())):
            self.augment3d_to_hwd(*affine)


class Tta3dEntries:
    """ctseg_tta_accumulate / ctseg_tta_finish ARE resample_oracles.oracle_accumulate / oracle_finish"""

    def tta_accumulate(self, logits, ld, C, D, H, W, matrix, chan_src, weight, mode, interp, Dt, Ht, Wt, layout, acc, acc_ld):
        M = mem(matrix, 12).reshape(3, 4).copy()
        src = mem(chan_src, C, np.int32).tolist() if chan_src else None
        assert logits and acc and np.isfinite(M).all() and np.isfinite(weight) and weight > 0 and mode in (0, 1) and interp in (0, 1)
        assert layout in (0, 1) and ld % 4 == 0 and 1 <= C <= min(ld, 16) and acc_ld % 4 == 0 and acc_ld >= C + 1
        assert src is None or sorted(src) == list(range(C))
        block = mem(logits, H * W * D * ld).reshape(H, W, D, ld)[..., :C]
        rows = mem(acc, Dt * Ht * Wt * acc_ld).reshape(-1, acc_ld)
        oracle_accumulate(rows, block, M, src, weight, mode, interp, (Dt, Ht, Wt), layout)

    def tta_finish(self, acc, acc_ld, C, St, mode, labels, probs, hist):
        assert acc and labels and mode in (0, 1) and acc_ld % 4 == 0 and acc_ld >= C + 1
        lab, pr, hs, _ = oracle_finish(mem(acc, St * acc_ld).reshape(St, acc_ld), C, mode)
        mem(labels, St, np.uint8)[:] = lab
        if probs:
            mem(probs, St * C).reshape(St, C)[:] = pr
        if hist:
            mem(hist, C, np.int64)[:] += hs


class SurfaceEntries:
    """ctseg_surface_edges, the squared distances to the edges as the metrics ask for them (d2_fg alone) and ctseg_surface_select"""
    calls = 0

    def surface_edges(self, pred, target, B, X, Y, Z, n_classes, axes, edges, counts):
        assert pred and target and edges and counts and 1 <= axes <= 7
        n, K = B * X * Y * Z, n_classes - 1
        p, t = (mem(a, n, np.uint8).reshape(B, X, Y, Z) for a in (pred, target))
        e = mem(edges, 2 * K * n, np.uint8).reshape(2, B, K, X, Y, Z)
        for s, L in enumerate((p, t)):
            for b in range(B):
                for k in range(K):
                    e[s, b, k] = surface_of(L[b], k + 1, axes)
        mem(counts, 2 * B * K, np.int32).reshape(2, B, K)[:] += e.reshape(2, B, K, -1).sum(-1, dtype=np.int64).astype(np.int32)
        self.calls += 1

    def distmap3d_batch(self, masks, P, X, Y, Z, mode, table, workspace, workspace_bytes, out, d2_fg, d2_bg):
        n = P * X * Y * Z
        assert masks and table and workspace and out and d2_fg and not d2_bg and workspace_bytes >= 6 * n and mode in (0, 1)
        vols = mem(masks, n, np.uint8).reshape(P, X, Y, Z) != 0
        mem(d2_fg, n, np.int32).reshape(P, X, Y, Z)[:] = np.stack([separable_d2_to(v) for v in vols])
        self.calls += 1

    def surface_select(self, edges, d2, counts, B, X, Y, Z, n_classes, q, workspace, workspace_bytes, stats, fstats):
        rows, S = 2 * B * (n_classes - 1), X * Y * Z
        assert workspace and workspace_bytes >= rows * surface.SELECT_ROW_BYTES and 0 <= q <= 100
        e = mem(edges, rows * S, np.uint8).reshape(rows, S) != 0
        d = mem(d2, rows * S, np.int32).reshape(rows, S)
        n = mem(counts, rows, np.int32)
        st, fs = mem(stats, rows * 4, np.int32).reshape(rows, 4), mem(fstats, rows * 2, np.float64).reshape(rows, 2)
        for r in range(rows):
            o = (r + rows // 2) % rows
            st[r], fs[r] = 0, 0.0
            if n[r] > 0 and n[o] > 0:
                v = np.sort(d[o][e[r]])
                assert len(v) == n[r] and v[0] >= 0
                lo, hi, g = ranks(len(v), q)
                st[r] = [v[lo], v[hi], v[-1], 1]
                fs[r] = [np.sqrt(v.astype(np.float64)).sum(), g]
        self.calls += 1


class SpacingEntries:
    """ctseg_distmap3d_weighted and ctseg_surface_select_f32: the float32 stages of the surface metrics in physical units"""
    calls = 0

    def distmap3d_weighted(self, masks, P, X, Y, Z, w, workspace, workspace_bytes, d2_fg, d2_bg):
        n = P * X * Y * Z
        assert masks and w and workspace and d2_fg and not d2_bg and workspace_bytes >= 6 * n
        vols = mem(masks, n, np.uint8).reshape(P, X, Y, Z) != 0
        wt = mem(w, P * 3, F32).reshape(P, 3)
        assert np.isfinite(wt).all() and (wt > 0).all()
        mem(d2_fg, n, F32).reshape(P, X, Y, Z)[:] = np.stack([d2w_to(v, wt[p]) for p, v in enumerate(vols)])
        self.calls += 1

    def surface_select_f32(self, edges, d2, counts, B, X, Y, Z, n_classes, q, workspace, workspace_bytes, stats, fstats):
        rows, S = 2 * B * (n_classes - 1), X * Y * Z
        assert workspace and workspace_bytes >= rows * surface.SELECT_F32_ROW_BYTES and 0 <= q <= 100
        e = mem(edges, rows * S, np.uint8).reshape(rows, S) != 0
        d = mem(d2, rows * S, F32).reshape(rows, S)
        n = mem(counts, rows, np.int32)
        st, fs = mem(stats, rows * 4, np.int32).reshape(rows, 4), mem(fstats, rows * 2, F64).reshape(rows, 2)
        for r in range(rows):
            o = (r + rows // 2) % rows
            st[r], fs[r] = 0, 0.0
            if n[r] > 0 and n[o] > 0:
                v = np.sort(d[o][e[r]])
                assert len(v) == n[r] and v[0] >= 0
                lo, hi, g = ranks(len(v), q)
                st[r, :3] = np.array([v[lo], v[hi], v[-1]], F32).view(np.int32)
                st[r, 3] = 1
                fs[r] = [np.sqrt(v.astype(F64)).sum(), g]
        self.calls += 1


class ComponentsEntries:
    """ctseg_components_label / ctseg_components_keep ARE component_oracles.label_oracle / keep_oracle"""
    calls = 0

    def components_label(self, labels, B, X, Y, Z, n_classes, connectivity, axes, ids, sizes):
        assert labels and ids and sizes and 1 <= connectivity <= 3 and 1 <= axes <= 7 and B * X * Y * Z < 1 << 31
        n = B * X * Y * Z
        i, s = label_oracle(mem(labels, n, np.uint8).reshape(B, X, Y, Z).copy(), connectivity, n_classes, axes)
        mem(ids, n, np.int32)[:] = i.reshape(-1)
        mem(sizes, n, np.int32)[:] = s.reshape(-1)
        self.calls += 1

    def components_keep(self, labels, ids, sizes, B, X, Y, Z, n_classes, class_mask, keep_largest, min_size, workspace,
                        workspace_bytes, out, table):
        n, K = B * X * Y * Z, n_classes - 1
        assert labels and ids and sizes and workspace and out and table and workspace_bytes >= B * K * components.KEEP_ROW_BYTES
        assert keep_largest in (0, 1) and min_size >= 0 and class_mask & ~((1 << n_classes) - 2) == 0
        L = mem(labels, n, np.uint8).reshape(B, X, Y, Z)
        o, t = keep_oracle(L, mem(ids, n, np.int32).reshape(L.shape), mem(sizes, n, np.int32).reshape(L.shape), n_classes, class_mask,
                           bool(keep_largest), min_size)
        mem(out, n, np.uint8)[:] = o.reshape(-1)
        mem(table, B * K * 4, np.int32)[:] = t.reshape(-1)
        self.calls += 1
