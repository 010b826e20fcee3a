"""Numpy oracles of the 2-D device input pipeline and of its warping presets: TEST INFRASTRUCTURE.

``o_*`` is a plain numpy restatement of the reference's arithmetic, written from its formulas and not imported from the product:
apply_window (capstone/transforms/transforms_2d.py:97-107), A.RandomCrop -> np.rot90 -> [:, ::-1], A.Resize (bilinear with
half-pixel centres on the float64 windowed image, nearest for masks), A.Normalize(max_pixel_value=1.0), _squash_masks and
weighted_mixup's structure indicator.  OpenCV and albumentations are not available, so parity with them is unpinned; this oracle
is what ctseg_pipeline2d_batch is held to, bit for bit.

``r_*`` restates the warps, again from the formulas.  It is the contract the three kernels of ctseg_pipeline2d_warp_batch are held
to, bit for bit:
  * displacement noise: u = (z >> 11) * 2**-53, z = splitmix64 mix of seed + ((f << 40 | i << 20 | j) + 1) * 0x9E3779B97F4A7C15
    (albumentations' random stream is not reproduced anywhere);
  * the blur: scipy.ndimage.gaussian_filter's arithmetic (mode "reflect", truncate 4.0, axis 0 then axis 1) in a FIXED summation
    order; this one is pinned against scipy itself, to summation-order noise (tests/test_warp2d.py);
  * cv2.warpAffine / cv2.remap / BORDER_REFLECT_101 in OpenCV's fixed point as this project understands it.  OpenCV and
    albumentations are not available, so parity with them is unpinned, as for A.Resize above.
"""
import numpy as np

DEV = "cuda:0"
WINDOWS3 = [(80, 40), (350, 20), (2800, 600)]
SOFT = [(350, 20)]
MEAN3, STD3 = (0.107, 0.135, 0.085), (0.271, 0.267, 0.152)
NP_OF_CODE = {0: np.float32, 2: np.int16, 3: np.uint8}
NONE, ELASTIC, GRID = 0, 1, 2
F32, F64, I64 = np.float32, np.float64, np.int64


# ---- the oracle of the crop / resize pipeline --------------------------------------------------------------------------------
def o_window(raw, width, level, shift):
    lo, hi = level - width // 2, level + width // 2
    if raw.dtype == np.float32:                            # numpy keeps a float32 array in float32
        v = np.clip(raw, np.float32(lo), np.float32(hi))
        if shift:
            v = (v - np.float32(lo)) / np.float32(hi - lo + 1e-8)
        assert v.dtype == np.float32
        return v.astype(np.float64)
    v = np.clip(raw.astype(np.float64), lo, hi)
    if shift:
        v = (v - lo) / (hi - lo + 1e-8)
    return v


def o_geometry_crop(x, Ho, Wo, y0, x0, k, flip):
    r = np.rot90(x[y0:y0 + Ho, x0:x0 + Wo], k)
    return r[:, ::-1] if flip else r


def o_lin_src(out, inn):
    f = ((np.arange(out, dtype=np.float64) + 0.5) * (inn / out) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    w = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= inn - 1
    s[low], w[low] = 0, 0
    s[high], w[high] = inn - 1, 0
    return s, np.minimum(s + 1, inn - 1), w


def o_resize_linear(x, Ho, Wo):
    assert x.dtype == np.float64
    sy, sy1, wy = o_lin_src(Ho, x.shape[0])
    sx, sx1, wx = o_lin_src(Wo, x.shape[1])
    h = x[:, sx] * (1 - wx)[None, :] + x[:, sx1] * wx[None, :]              # 1 - w stays float32; the products are float64
    v = h[sy] * (1 - wy)[:, None] + h[sy1] * wy[:, None]
    assert v.dtype == np.float64 and (1 - wx).dtype == np.float32
    return v


def o_near_src(out, inn):
    return np.minimum(np.floor(np.arange(out, dtype=np.float64) * (inn / out)).astype(np.int64), inn - 1)


def o_normalize(v, mean, denom):
    v = v.astype(np.float32)
    if mean is not None:
        v = v - np.float32(mean)
        v = v * np.float32(denom)
    return v


def oracle_batch(raws, masks, rows, mode, size, windows, shift, mean, denom):
    """raws: list of (H,W) arrays, masks: list of (K,H,W) u8 (or None), rows: (B,5) slice index, y0, x0, k, flip"""
    Ho, Wo = size
    images, mouts = [], []
    for i, y0, x0, k, flip in rows:
        chans = []
        for c, (width, level) in enumerate(windows):
            v = o_window(raws[i], width, level, shift)
            v = o_geometry_crop(v, Ho, Wo, y0, x0, k, flip) if mode == "crop" else o_resize_linear(v, Ho, Wo)
            chans.append(o_normalize(v, None if mean is None else mean[c], None if mean is None else denom[c]))
        images.append(np.stack(chans))
        if masks is not None:
            m = masks[i]
            if mode == "crop":
                mouts.append(np.stack([o_geometry_crop(p, Ho, Wo, y0, x0, k, flip) for p in m]))
            else:
                mouts.append(m[:, o_near_src(Ho, m.shape[1])][:, :, o_near_src(Wo, m.shape[2])])
    out = {"image": np.stack(images)}
    if masks is not None:
        mo = np.stack(mouts)
        K = mo.shape[1]
        labels = (mo.astype(np.int64) * np.arange(1, K + 1)[None, :, None, None]).max(1)
        out.update(masks=mo, labels=labels.astype(np.uint8), present=(mo == 1).any(axis=(2, 3)).astype(np.int32),
                   hist=np.stack([np.bincount(l.reshape(-1), minlength=K + 1) for l in labels]))
    return out


# ---- the restatement of the warps --------------------------------------------------------------------------------------------
def r_noise(seed, f, H, W):
    i, j = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        ctr = (np.uint64(f) << np.uint64(40)) | (i << np.uint64(20)) | j
        z = np.uint64(seed) + (ctr + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(11)).astype(F64) * 2.0 ** -53
    return 2.0 * u - 1.0


def r_reflect_sym(p, n):                                   # d c b a | a b c d
    p = np.mod(p, 2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def r_reflect_101(p, n):                                   # d c b | a b c d: -1 -> 1, n -> n - 2, repeated
    if n == 1:
        return np.zeros_like(p)
    p = np.mod(p, 2 * n - 2)
    return np.where(p < n, p, 2 * n - 2 - p)


def r_gauss_w(sigma):
    radius = int(4.0 * sigma + 0.5)
    k = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return (w / w.sum())[radius:]


def r_blur(a, w):
    """axis 0, then axis 1; per element the centre term first, then k = 1..radius: + (in[l-k] + in[l+k]) * w[k]"""
    for axis in (0, 1):
        n = a.shape[axis]
        idx = np.arange(n)
        out = np.take(a, idx, axis) * w[0]
        for k in range(1, len(w)):
            out = out + (np.take(a, r_reflect_sym(idx - k, n), axis) + np.take(a, r_reflect_sym(idx + k, n), axis)) * w[k]
        a = out
    return a


def r_fields(seed, H, W, w, alpha):
    return [np.float32(r_blur(r_noise(seed, f, H, W), w) * alpha) for f in (0, 1)]


def r_sat_rint(v):
    return np.rint(np.clip(v, -2147483648.0, 2147483647.0)).astype(I64)


def r_affine_fixed(M, H, W, delta, shift):
    """(X, Y) of every destination pixel: AB_BITS = 10"""
    y, x = np.arange(H, dtype=F64)[:, None], np.arange(W, dtype=F64)[None, :]
    X = (r_sat_rint((M[1] * y + M[2]) * 1024.0) + delta + r_sat_rint(M[0] * x * 1024.0)) >> shift
    Y = (r_sat_rint((M[4] * y + M[5]) * 1024.0) + delta + r_sat_rint(M[3] * x * 1024.0)) >> shift
    return X, Y


def r_bilinear(img, sx, sy, fx, fy, seen=None):
    H, W = img.shape
    if seen is not None:
        seen.append((sx.min(), (sx + 1).max() - (W - 1), sy.min(), (sy + 1).max() - (H - 1)))
    c0, c1, r0, r1 = r_reflect_101(sx, W), r_reflect_101(sx + 1, W), r_reflect_101(sy, H), r_reflect_101(sy + 1, H)
    gx, gy = F32(1) - fx, F32(1) - fy
    w = [gx * gy, fx * gy, gx * fy, fx * fy]
    assert all(t.dtype == F32 for t in w) and img.dtype == F64
    return img[r0, c0] * w[0].astype(F64) + img[r0, c1] * w[1].astype(F64) + img[r1, c0] * w[2].astype(F64) + img[r1, c1] * w[3].astype(F64)


def r_warp_affine(img, M, seen=None):
    X, Y = r_affine_fixed(M, *img.shape, 16, 5)
    return r_bilinear(img, X >> 5, Y >> 5, (X & 31).astype(F32) / F32(32), (Y & 31).astype(F32) / F32(32), seen)


def r_warp_affine_nearest(m, M):
    X, Y = r_affine_fixed(M, *m.shape[-2:], 512, 10)
    return m[..., r_reflect_101(Y, m.shape[-2]), r_reflect_101(X, m.shape[-1])]


def no_ties(map_v):
    """no float32 map value within 1e-6 of a rounding tie of lrint(map * 32) or lrint(map)"""
    t = map_v.astype(F64)
    return bool((np.abs(t * 32 - np.floor(t * 32) - 0.5) / 32 > 1e-6).all() and (np.abs(t - np.floor(t) - 0.5) > 1e-6).all())


def r_elastic_maps(seed, Ho, Wo, gw, alpha):
    dx, dy = r_fields(seed, Ho, Wo, gw, alpha)
    yy_, xx_ = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    return F32(xx_ + dx), F32(yy_ + dy)


def r_remap(img, map_x, map_y, seen=None):
    assert map_x.dtype == F32 and map_y.dtype == F32
    sx, sy = np.rint(map_x * F32(32)).astype(I64), np.rint(map_y * F32(32)).astype(I64)
    return r_bilinear(img, sx >> 5, sy >> 5, (sx & 31).astype(F32) / F32(32), (sy & 31).astype(F32) / F32(32), seen)


def r_remap_nearest(m, map_x, map_y):
    ix, iy = np.rint(map_x).astype(I64), np.rint(map_y).astype(I64)
    return m[..., r_reflect_101(iy, m.shape[-2]), r_reflect_101(ix, m.shape[-1])]


def r_invert(M):
    """cv2.warpAffine's inversion of the forward matrix"""
    M = np.asarray(M, F64).reshape(6)
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = M[4] * D, M[0] * D
    m0, m1, m3, m4 = a11, M[1] * -D, M[3] * -D, a22
    return np.array([m0, m1, -m0 * M[2] - m1 * M[5], m3, m4, -m3 * M[2] - m4 * M[5]])


def r_elastic_matrix(size, delta):
    h, w = size
    c = F32((h, w)) // 2
    s = min(h, w) // 3
    pts1 = F32([c + s, [c[0] + s, c[1] - s], c - s])
    pts2 = pts1 + F32(delta)
    return np.linalg.solve(np.concatenate([pts1.astype(F64), np.ones((3, 1))], 1), pts2.astype(F64)).T


def r_grid_table(width, num_steps, steps):
    """the reference's loop (albumentations F.grid_distortion), transcribed"""
    x_step = width // num_steps
    xx = np.zeros(width, np.float32)
    prev = 0
    for idx in range(num_steps + 1):
        x = idx * x_step
        start = int(x)
        end = int(x) + x_step
        if end > width:
            end = width
            cur = width
        else:
            cur = prev + x_step * steps[idx]
        xx[start:end] = np.linspace(prev, cur, end - start)
        prev = cur
    return xx


def r_batch(raws, masks, samples, size, windows, shift, mean, denom, gw, alpha, seen=None, check_ties=False):
    """samples: dicts of i, y0, x0, k, flip, kind and, per kind, minv (6,) + seed, or xx + yy.  -> image, masks, labels, hist, present"""
    Ho, Wo = size
    images, mouts = [], []
    for s in samples:
        y0, x0 = s["y0"], s["x0"]
        crop = raws[s["i"]][y0:y0 + Ho, x0:x0 + Wo]
        m = masks[s["i"]][:, y0:y0 + Ho, x0:x0 + Wo] if masks is not None else None
        map_x = map_y = None
        if s["kind"] == ELASTIC:
            map_x, map_y = r_elastic_maps(s["seed"], Ho, Wo, gw, alpha)
        elif s["kind"] == GRID:
            map_x, map_y = np.meshgrid(F32(s["xx"]), F32(s["yy"]))
        if map_x is not None and check_ties:
            assert no_ties(map_x) and no_ties(map_y)         # a tie would put the inputs at fault, not the tolerance
        chans = []
        for c, (width, level) in enumerate(windows):
            v = o_window(crop, width, level, shift)
            if s["kind"] == ELASTIC:
                v = r_warp_affine(v, s["minv"], seen)
            if map_x is not None:
                v = r_remap(v, map_x, map_y, seen)
            v = np.rot90(v, s["k"])
            v = v[:, ::-1] if s["flip"] else v
            chans.append(o_normalize(v, None if mean is None else mean[c], None if mean is None else denom[c]))
        images.append(np.stack(chans))
        if m is not None:
            if s["kind"] == ELASTIC:
                m = r_warp_affine_nearest(m, s["minv"])
            if map_x is not None:
                m = r_remap_nearest(m, map_x, map_y)
            m = np.rot90(m, s["k"], axes=(1, 2))
            mouts.append(m[:, :, ::-1] if s["flip"] else m)
    out = {"image": np.stack(images)}
    if masks is not None:
        mo = np.stack(mouts)
        K = mo.shape[1]
        labels = (mo.astype(I64) * np.arange(1, K + 1)[None, :, None, None]).max(1)
        out.update(masks=mo, labels=labels.astype(np.uint8), present=(mo == 1).any(axis=(2, 3)).astype(np.int32),
                   hist=np.stack([np.bincount(l.reshape(-1), minlength=K + 1) for l in labels]))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_raw(shape, dtype, seed):
    """values straddling every bound of the three windows ([0, 80], [-155, 195], [-800, 2000]) and the type's extremes"""
    rng = np.random.default_rng(seed)
    edges = np.array([-801, -800, -799, -156, -155, -154, -1, 0, 1, 79, 80, 81, 194, 195, 196, 1999, 2000, 2001], dtype=np.float64)
    if dtype == np.int16:
        pool = np.concatenate([edges, [-32768, 32767], rng.integers(-1100, 2300, 30)])
    elif dtype == np.uint8:
        pool = np.concatenate([edges[(edges >= 0) & (edges <= 255)], [255], rng.integers(0, 256, 30)])
    else:
        pool = np.concatenate([edges, edges + 0.5, edges - 0.25, [-3.0e4, 6.5e4, 1e-3], rng.normal(100, 700, 30)])
    return rng.choice(pool, size=shape).astype(dtype)


def make_masks(shape, seed, as_bool=False):
    """9 overlapping structures; structure 2 (index 1) lies wholly under structure 6 (index 5): present, but gone from the label
    histogram; structure 5 (index 4) is empty"""
    rng = np.random.default_rng(seed)
    m = rng.random((9,) + shape) < 0.2
    m[1] = m[5] & (rng.random(shape) < 0.6)
    m[4] = False
    return m if as_bool else m.astype(np.uint8)


def _write_npz(root, split, n, seed, bool_masks):
    d = root / "miccai_2d" / split
    d.mkdir(parents=True)
    rng = np.random.default_rng(seed)
    raws, masks, inds = [], [], []
    for i in range(n):
        shape = (int(rng.integers(12, 20)), int(rng.integers(12, 20)))
        raws.append(make_raw(shape, np.int16, seed + i))
        masks.append(make_masks(shape, seed + i, as_bool=bool_masks and i % 2 == 0))
        inds.append((rng.random(9) < 0.8).astype(np.float64))
        # written out of order: the dataset sorts by name
        np.savez(d / f"case{(n - 1 - i):03d}.npz", image=raws[-1][None], masks=masks[-1], mask_indicator=inds[-1])
    return raws[::-1], masks[::-1], inds[::-1]
