"""Numpy oracles of the patch sampling passes: TEST INFRASTRUCTURE, restated from the rules in include/ctseg_hip.h
(ctseg_patch_centres, ctseg_patch3d_to_hwd), independent of torch and of the product.

Centres: Python integers and ``np.flatnonzero(mask[k])[r]``.  Crop: ``crop`` is numpy indexing of the exact crop
``src[c - patch // 2 + o]``; ``patch_oracle`` is the affine pass of resample_oracles.py on the SOURCE grid (no virtual resized
volume: the index rule is the identity and "outside" is outside [0, dim)) with the translation column t' = f32(t + f32(c)), every
float32 operation rounded once.
"""
import numpy as np

import resample_oracles as R

COUNT_BLOCK = 16384              # voxels per (class, block) count of the count pass, from the header


def workspace_bytes(K, D, H, W):
    return 4 * (K * (-(-(D * H * W) // COUNT_BLOCK)) + 16)


def clamp_centre(c, dims, patch):
    out = []
    for ca, dim, pa in zip(c, dims, patch):
        out.append(dim // 2 if dim < pa else min(max(ca, pa // 2), dim - (pa - pa // 2)))
    return out


def centres(masks, draws, class_mask=None, patch=None):
    """masks (K,D,H,W) u8, draws rows (fg, a, b) -> (P, 4) int32 rows (d, h, w, class)"""
    K, dims = masks.shape[0], masks.shape[1:]
    N = int(np.prod(dims))
    class_mask = (1 << K) - 1 if class_mask is None else class_mask
    flat = [np.flatnonzero(masks[k].reshape(-1)) for k in range(K)]
    eligible = [k for k in range(K) if (class_mask >> k) & 1 and len(flat[k]) > 0]
    out = []
    for fg, a, b in draws:
        if fg and eligible:
            cls = eligible[(int(a) * len(eligible)) >> 32]
            vox = int(flat[cls][(int(b) * len(flat[cls])) >> 32])
        else:
            cls, vox = -1, (int(b) * N) >> 32
        c = list(np.unravel_index(vox, dims))
        if patch is not None:
            c = clamp_centre(c, dims, patch)
        out.append([int(v) for v in c] + [cls])
    return np.asarray(out, dtype=np.int32)


def draw_for_rank(r, n):
    """the smallest b with b * n >> 32 == r"""
    b = -((-r << 32) // n)
    assert (b * n) >> 32 == r and 0 <= b < 2 ** 32
    return b


def crop(volume, patch, centre, border, fill):
    """volume (D,H,W) -> (d,h,w): volume[c - patch // 2 + o], ``fill`` outside (border 0) or the edge voxel (border 1)"""
    idx, ok = [], []
    for a in range(3):
        i = centre[a] - patch[a] // 2 + np.arange(patch[a])
        ok.append((i >= 0) & (i < volume.shape[a]))
        idx.append(np.clip(i, 0, volume.shape[a] - 1))
    v = volume[np.ix_(*idx)]
    if not border:
        inside = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        v = np.where(inside, v, np.asarray(fill, dtype=v.dtype))
    return v


def window_f32(v, window, lo, hi):
    f = np.float32
    v = v.astype(f)
    if window:
        v = np.clip(v, f(lo), f(hi))
        if window == 2:
            v = (v - f(lo)) / f(float(hi) - float(lo) + 1e-8)
    return v


def crop_oracle(image, masks, patch, centre, border=0, cval=0.0, window=0, lo=0.0, hi=1.0):
    """the exact crop by numpy slicing -> image (h,w,d) f32, masks (K,h,w,d) u8, labels (h,w,d) u8, hist (K+1); None where absent"""
    img = m = lab = hist = None
    if image is not None:
        v = window_f32(crop(image.astype(np.float32), patch, centre, border, np.float32(cval)), window, lo, hi)
        img = np.ascontiguousarray(np.transpose(v, (1, 2, 0)))
    if masks is not None:
        r = np.stack([crop(mk, patch, centre, border, 0) for mk in masks]).astype(np.int32)
        labels = ((r != 0) * np.arange(1, len(masks) + 1).reshape(-1, 1, 1, 1)).max(0)
        m = np.ascontiguousarray(np.transpose((r != 0).astype(np.uint8), (0, 2, 3, 1)))
        lab = np.ascontiguousarray(np.transpose(labels.astype(np.uint8), (1, 2, 0)))
        hist = np.bincount(labels.reshape(-1), minlength=len(masks) + 1).astype(np.int64)
    return img, m, lab, hist


def _axis(g, n, border):
    """whole-valued coordinates g of the source grid -> (index, inside)"""
    r = np.clip(g, -1, n).astype(np.int64)
    ok = (r >= 0) & (r < n)
    if border:
        r, ok = np.clip(r, 0, n - 1), np.ones_like(ok)
    return np.where(ok, r, 0), ok


def translated(A, centre):
    """t' = f32(t + f32(c)): one float32 add per axis"""
    A = np.array(A, dtype=np.float32).reshape(3, 4)
    A[:, 3] = A[:, 3] + np.asarray(centre[:3]).astype(np.float32)
    assert A.dtype == np.float32
    return A


def patch_oracle(image, masks, patch, A, centre, interp=0, border=0, cval=0.0, mask_src=None, window=0, lo=0.0, hi=1.0, gain=1.0,
                 bias=0.0):
    """the affine pass with the translated matrix, float32 -> image (h,w,d), masks (K,h,w,d), labels (h,w,d), hist (K+1)"""
    f = np.float32
    shape = (image if image is not None else masks).shape[-3:]
    q = R.coordinates(patch, translated(A, centre))
    near = [_axis(np.floor(q[a] + f(0.5)), shape[a], border) for a in range(3)]
    inside = near[0][1] & near[1][1] & near[2][1]
    img = m_out = labels = hist = None
    if image is not None:
        def fetch(ix):
            ok = ix[0][1] & ix[1][1] & ix[2][1]
            return np.where(ok, image[ix[0][0], ix[1][0], ix[2][0]].astype(f), f(cval))
        if interp == 0:
            v = fetch(near)
        else:
            b = [np.floor(q[a]) for a in range(3)]
            t = [q[a] - b[a] for a in range(3)]
            corner = [[_axis(np.clip(b[a], -2, shape[a]) + f(c), shape[a], border) for c in (0, 1)] for a in range(3)]

            def lerp(x, y, w):
                return x + w * (y - x)
            along_d = []
            for cd in (0, 1):
                along_h = []
                for ch in (0, 1):
                    x, y = (fetch((corner[0][cd], corner[1][ch], corner[2][cw])) for cw in (0, 1))
                    along_h.append(lerp(x, y, t[2]))
                along_d.append(lerp(along_h[0], along_h[1], t[1]))
            v = lerp(along_d[0], along_d[1], t[0])
        v = window_f32(v, window, lo, hi)
        if not (gain == 1.0 and bias == 0.0):
            v = v * f(gain) + f(bias)
        assert v.dtype == f
        img = np.ascontiguousarray(np.transpose(v, (1, 2, 0)))
    if masks is not None:
        src = list(range(len(masks))) if mask_src is None else list(mask_src)
        r = np.stack([np.where(inside, masks[s][near[0][0], near[1][0], near[2][0]], 0) for s in src]).astype(np.int32)
        lab = ((r != 0) * np.arange(1, len(src) + 1).reshape(-1, 1, 1, 1)).max(0)
        m_out = np.ascontiguousarray(np.transpose((r != 0).astype(np.uint8), (0, 2, 3, 1)))
        labels = np.ascontiguousarray(np.transpose(lab.astype(np.uint8), (1, 2, 0)))
        hist = np.bincount(lab.reshape(-1), minlength=len(src) + 1).astype(np.int64)
    return img, m_out, labels, hist


def centre_masks(dims, seed=0):
    """K = 4 masks over ``dims``: empty; one voxel at the last index; about half full; about 300 voxels, part of them inside the
    third"""
    rng = np.random.default_rng(seed + sum(dims))
    N = int(np.prod(dims))
    m = np.zeros((4, N), np.uint8)
    m[1, N - 1] = 1
    m[2] = (rng.random(N) < 0.5) * rng.integers(1, 256, N)          # set = any nonzero byte
    m[3, rng.choice(N, 300, replace=False)] = 255
    assert (m[2].astype(bool) & m[3].astype(bool)).any() and (~m[2].astype(bool) & m[3].astype(bool)).any()
    return m.reshape((4,) + tuple(dims))
