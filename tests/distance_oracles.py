"""Numpy oracles of the distance transforms and of what is built on them: TEST INFRASTRUCTURE, independent of scipy and of the kernels.

Squared distances to a set, for planes (nd = 2) and volumes (nd = 3) alike: brute force (for every point the minimum of the squared
Euclidean distance over all set points) and a separable form for shapes too large for brute force (one pass per axis, min over t'
of (t - t')^2 + f[t'] with one whole-array step per t').  Then the byte the reference stores in its uint8 result array,

    k = isqrt(d2_fg) & 255 outside, (-(isqrt(d2_bg) - 1)) & 255 inside, 0 on a plane / volume without foreground

and the map k / 255.0.  tests/golden/distmap2d_reference.npz and distmap3d_reference.npz hold mask stacks and the float64 output of
the reference's own compute_distance_map for them (tools/make_distmap2d_fixture.py, tools/make_distmap3d_fixture.py); ``oracle``
equals them exactly.  A plane or volume without any background has no defined reference value: the product writes 0 there, so does
the oracle, and the fixtures hold none.

The surface rule, the pairwise distances and the ranks of the surface metrics, in voxels (``surface_of``, ``d2_between``, ``ranks``)
and in physical units: with w = the float32 squares of the float32 voxel sizes, the float32 expression the header pins,

    fl(fl(wy dy^2) + fl(fl(wz dz^2) + fl(wx dx^2)))          (numpy float32 arithmetic: one rounding per operation, no FMA)

by brute force over the set (``pair_min``, ``d2w_between``, ``d2w_to``).  Last, the shapes the tests feed them.
"""
import numpy as np
import torch

from capstone_amd.data import utils as DU

DEV = "cuda:0"
BRUTE_MAX = 5 * 7 * 3 * 20           # points up to which the default oracle is brute force (the 3-D fixture's balls: 12 * 15 * 9)
BRUTE_PAIRS = 4_000_000
C = 10
MAX_ROW = 10_000                       # surface voxels per row in every test of the surface metrics: the bound of their summation error
F32 = np.float32


# ---- squared distances, any rank ---------------------------------------------------------------------------------------------
def isqrt(v):
    """floor(sqrt(v)) of a non-negative integer array, exactly"""
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r -= r * r > v
    r += (r + 1) * (r + 1) <= v
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


def brute_d2_to(sel):
    """bool array of any rank -> int64 of its shape: min over the set points of the squared distance; -1 everywhere when there is none"""
    if not sel.any():
        return np.full(sel.shape, -1, np.int64)
    pts = np.argwhere(sel).astype(np.int64)                                       # (N, rank)
    rest = np.indices(sel.shape[1:]).reshape(sel.ndim - 1, -1).T                  # (points of one slab, rank - 1)
    out = np.empty(sel.shape, np.int64)
    for x in range(sel.shape[0]):
        d = (x - pts[:, 0]) ** 2 + ((rest[:, None, :] - pts[None, :, 1:]) ** 2).sum(-1)   # (points of one slab, N)
        out[x] = d.min(axis=1).reshape(sel.shape[1:])
    return out


def separable_d2_to(sel):
    """one pass per axis: f <- min over t' of (t - t')^2 + f[t'], from f = 0 on the set and "none" elsewhere"""
    if not sel.any():
        return np.full(sel.shape, -1, np.int64)
    none = np.int64(1) << 40
    f = np.where(sel, np.int64(0), none)
    for axis in range(sel.ndim):
        n = sel.shape[axis]
        t = np.arange(n, dtype=np.int64).reshape([n if a == axis else 1 for a in range(sel.ndim)])
        best = np.full(sel.shape, none, np.int64)
        for s in range(n):
            np.minimum(best, (t - s) ** 2 + np.take(f, [s], axis=axis), out=best)
        f = np.minimum(best, none)
    return f


def bytes_of(fg, d2_fg, d2_bg):
    if not fg.any() or fg.all():
        return np.zeros(fg.shape, np.int64)
    return np.where(fg, (-(isqrt(np.maximum(d2_bg, 0)) - 1)) & 255, isqrt(np.maximum(d2_fg, 0)) & 255)


_CACHE = {}


def oracle(masks, nd, d2_to=None):
    """(..., nd trailing axes) uint8 -> d2_fg, d2_bg int64 and the float64 map k / 255.0, plane by plane or volume by volume (results
    are shared between tests).  Without ``d2_to``: brute force up to BRUTE_MAX points, the separable form above."""
    masks = np.asarray(masks)
    flat = masks.reshape((-1,) + masks.shape[-nd:])
    fn = d2_to or (brute_d2_to if flat[0].size <= BRUTE_MAX else separable_d2_to)
    out = []
    for v in flat:
        key = (fn.__name__, v.shape, v.tobytes())
        if key not in _CACHE:
            fg = v != 0
            d2f, d2b = fn(fg), fn(~fg)
            _CACHE[key] = (d2f, d2b, bytes_of(fg, d2f, d2b) / 255.0)
        out.append(_CACHE[key])
    return tuple(np.stack([o[i] for o in out]).reshape(masks.shape) for i in range(3))


def signed_map(masks, d2_fg, d2_bg, nd):
    """float64: d_out / 255 outside, -(d_in - 1) / 255 inside; 0 on a plane / volume without foreground or without background"""
    fg = np.asarray(masks) != 0
    v = np.where(fg, -(np.sqrt(np.maximum(d2_bg, 0).astype(np.float64)) - 1.0), np.sqrt(np.maximum(d2_fg, 0).astype(np.float64))) / 255.0
    axes = tuple(range(-nd, 0))
    defined = fg.any(axis=axes, keepdims=True) & ~fg.all(axis=axes, keepdims=True)
    return np.where(defined, v, 0.0)


# ---- the kernel against the oracle, bit for bit ------------------------------------------------------------------------------
def run_gpu(masks, nd, **kw):
    out = DU.compute_distance_map(torch.from_numpy(np.ascontiguousarray(masks)).to(DEV), return_d2=True, spatial_dims=nd, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def check_reference_mode(masks, nd, d2_to=None):
    got, d2f, d2b = run_gpu(masks, nd)
    ref_f, ref_b, ref = oracle(masks, nd, d2_to)
    assert d2f.dtype == np.int32 and d2b.dtype == np.int32 and got.dtype == np.float32 and got.shape == masks.shape
    assert np.array_equal(d2f, ref_f), int((d2f != ref_f).sum())
    assert np.array_equal(d2b, ref_b), int((d2b != ref_b).sum())
    assert np.array_equal(got, ref.astype(np.float32)), int((got != ref.astype(np.float32)).sum())
    return got


# ---- surfaces and distances between them -------------------------------------------------------------------------------------
def surface_of(L, c, axes=7):
    """(X, Y, Z) labels -> bool: voxels of label c with a missing or differing neighbour along an active axis (bit a = axis a)"""
    m = L == c
    inner = m.copy()
    for a in range(3):
        if not (axes >> a) & 1:
            continue
        p = np.zeros_like(m)
        sl, sr = [slice(None)] * 3, [slice(None)] * 3
        sl[a], sr[a] = slice(1, None), slice(None, -1)
        p[tuple(sl)] = m[tuple(sr)]                                      # the neighbour at -1 (outside: False)
        n = np.zeros_like(m)
        n[tuple(sr)] = m[tuple(sl)]                                      # the neighbour at +1
        inner &= p & n
    return m & ~inner


def d2_between(src, dst):
    """squared distance of every set voxel of `src` to the nearest set voxel of `dst`, in np.argwhere order of `src`"""
    a, b = np.argwhere(src).astype(np.int64), np.argwhere(dst).astype(np.int64)
    if len(a) * len(b) > BRUTE_PAIRS:
        return separable_d2_to(dst)[src]
    out = np.empty(len(a), np.int64)
    for i in range(0, len(a), 256):
        out[i:i + 256] = ((a[i:i + 256, None, :] - b[None, :, :]) ** 2).sum(-1).min(1)
    return out


def ranks(n, q):
    r = (n - 1) * (q / 100.0)
    lo = int(np.floor(r))
    return lo, min(lo + 1, n - 1), r - lo


def pair_min(a, b, w, dtype=F32):
    """(n, 3), (m, 3) integer points, w (3,) -> (n,) the minimum over b of the pinned expression, in `dtype` arithmetic"""
    w = w.astype(dtype)
    out = np.empty(len(a), dtype)
    for i in range(0, len(a), 256):
        d = ((a[i:i + 256, None, :] - b[None, :, :]) ** 2).astype(dtype)             # integer squares below 2^24: exact
        out[i:i + 256] = (w[1] * d[..., 1] + (w[2] * d[..., 2] + w[0] * d[..., 0])).min(1)
    return out


def d2w_between(src, dst, w, dtype=F32):
    a, b = np.argwhere(src).astype(np.int64), np.argwhere(dst).astype(np.int64)
    assert len(a) * len(b) <= BRUTE_PAIRS
    return pair_min(a, b, w, dtype)


def d2w_to(dst, w):
    """the weighted transform of one volume: 0 on `dst`, the minimum elsewhere, -1 everywhere when `dst` is empty"""
    out = np.zeros(dst.shape, F32)
    if not dst.any():
        out[:] = -1.0
    elif not dst.all():
        out[~dst] = d2w_between(~dst, dst, w)
    return out


# ---- the tables of the surface metrics --------------------------------------------------------------------------------------
_SURFACE_CACHE = {}


def surface_oracle(pred, target, q=95.0, n_classes=C, axes=7):
    """(B, X, Y, Z) label maps -> dict of the tables of surface_distances (numpy) and `edges` (2, B, C-1, X, Y, Z) uint8"""
    key = (pred.tobytes(), target.tobytes(), pred.shape, q, n_classes, axes)
    if key in _SURFACE_CACHE:
        return _SURFACE_CACHE[key]
    B, K = pred.shape[0], n_classes - 1
    edges = np.zeros((2, B, K) + pred.shape[1:], np.uint8)
    o = {k: np.zeros((2, B, K), np.int64) for k in ("counts", "d2_lo", "d2_hi", "d2_max")}
    f = {k: np.full((2, B, K), np.nan) for k in ("hd_directed", "hd_max_directed", "asd_directed", "root_sum", "gamma")}
    assd = np.full((B, K), np.nan)
    for b in range(B):
        for k in range(K):
            s = [surface_of(pred[b], k + 1, axes), surface_of(target[b], k + 1, axes)]
            edges[0, b, k], edges[1, b, k] = s
            o["counts"][:, b, k] = [s[0].sum(), s[1].sum()]
            if not s[0].any() or not s[1].any():
                continue
            tot = 0.0
            for d in (0, 1):
                d2 = np.sort(d2_between(s[d], s[1 - d]))
                lo, hi, g = ranks(len(d2), q)
                roots = np.sqrt(d2.astype(np.float64))
                o["d2_lo"][d, b, k], o["d2_hi"][d, b, k], o["d2_max"][d, b, k] = d2[lo], d2[hi], d2[-1]
                f["hd_directed"][d, b, k] = np.percentile(roots, q)
                f["hd_max_directed"][d, b, k] = roots[-1]
                f["asd_directed"][d, b, k] = roots.mean()
                f["root_sum"][d, b, k], f["gamma"][d, b, k] = roots.sum(), g
                tot += roots.sum()
            assd[b, k] = tot / (s[0].sum() + s[1].sum())
    res = dict(o, **f, edges=edges, assd=assd, hd=np.maximum(f["hd_directed"][0], f["hd_directed"][1]),
               valid=(o["counts"] > 0).all(0)[None].repeat(2, 0))
    _SURFACE_CACHE[key] = res
    return res


def nan_reduce(table):
    """(N, K) -> (mean, per class): NaN-ignoring mean over samples, then over the classes that have a value"""
    have = ~np.isnan(table)
    pc = np.where(have.any(0), np.where(have, table, 0.0).sum(0) / np.maximum(have.sum(0), 1), np.nan)
    return (pc[~np.isnan(pc)].mean() if (~np.isnan(pc)).any() else np.nan), pc


def check_tables(got, ref, B, K=C - 1):
    for k in ("hd_directed", "hd_max_directed", "asd_directed", "gamma", "root_sum", "valid", "counts", "d2_lo", "d2_hi", "d2_max"):
        assert got[k].shape == (2, B, K), k
    assert got["hd"].shape == got["assd"].shape == (B, K)
    assert got["counts"].dtype == np.int64 and got["d2_lo"].dtype == np.int32 and got["hd"].dtype == np.float64
    assert got["assd"].dtype == got["hd_directed"].dtype == got["asd_directed"].dtype == np.float64 and got["valid"].dtype == bool
    for k in ("counts", "d2_lo", "d2_hi", "d2_max", "valid"):
        assert np.array_equal(got[k], ref[k]), k
    assert ref["counts"].max() <= MAX_ROW
    for k in ("hd_directed", "hd", "hd_max_directed", "asd_directed", "assd"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
        assert np.array_equal(np.isnan(got[k]), ~ref["valid"][0] if got[k].ndim == 2 else ~ref["valid"]), k
    ok = ref["valid"]
    for k in ("hd_directed", "hd_max_directed"):
        err = np.abs(got[k][ok] - ref[k][ok])
        print(f"{k}: worst error {err.max() if err.size else 0.0:.3e}")
        assert (err <= 1e-9).all(), (k, float(err.max()))
    assert (np.abs(got["hd"][ok[0]] - ref["hd"][ok[0]]) <= 1e-9).all()
    for k in ("asd_directed", "assd", "root_sum"):
        sel = ok if got[k].ndim == 3 else ok[0]
        err = np.abs(got[k][sel] - ref[k][sel]) / np.maximum(np.abs(ref[k][sel]), 1e-300)
        err = np.where(ref[k][sel] == 0, np.abs(got[k][sel]), err)
        print(f"{k}: worst relative error {err.max() if err.size else 0.0:.3e}")
        assert (err <= 1e-11).all(), (k, float(err.max()))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def blobs(shape, seed, n=3, value=1):
    """n discs (balls in three dimensions) of `value`, centres and radii drawn from `seed`"""
    rng = np.random.default_rng(seed)
    grid = np.mgrid[tuple(slice(s) for s in shape)]
    m = np.zeros(shape, np.uint8)
    for _ in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(0.8, max(1.5, min(shape) / 3))
        m[sum((g - ci) ** 2 for g, ci in zip(grid, c)) <= r * r] = value
    return m


def ball_labels(shape, seed, shift=(0, 0, 0), n_classes=C):
    """a label map of one ball per class, radii and centres drawn from `seed`, every centre moved by `shift`; later classes
    overwrite earlier ones, so structures cut into each other"""
    rng = np.random.default_rng(seed)
    g = np.mgrid[:shape[0], :shape[1], :shape[2]]
    L = np.zeros(shape, np.uint8)
    for c in range(1, n_classes):
        ctr = [rng.uniform(0, s) + d for s, d in zip(shape, shift)]
        r = rng.uniform(0.8, max(1.6, min(max(shape) / 4, 6.0)))
        L[sum((g[a] - ctr[a]) ** 2 for a in range(3)) <= r * r] = c
    return L


def batch_of(shape):
    """B = 2: random balls shifted between prediction and truth; in sample 1 class 2 lies inside class 6, and class 8 touches every
    face of the volume (a frame of the border voxels), shifted nowhere but thinned in the prediction"""
    X, Y, Z = shape
    pred = np.stack([ball_labels(shape, 10), ball_labels(shape, 20)])
    target = np.stack([ball_labels(shape, 10, (1, -1, 2)), ball_labels(shape, 20, (0, 1, -1))])
    for L, grow in ((pred[1], 0), (target[1], 1)):
        L[X // 4:X // 4 + X // 2 + 1, Y // 4:Y // 4 + Y // 2 + 1, Z // 4:Z // 4 + Z // 2 + 1] = 6
        L[X // 2, Y // 2, Z // 2:Z // 2 + 1 + grow] = 2
    target[1][[0, -1]] = 8
    target[1][:, [0, -1]] = 8
    target[1][:, :, [0, -1]] = 8
    pred[1][0, 0, 0] = pred[1][-1, -1, -1] = 8
    return pred, target


def absent_batch(shape=(6, 7, 9)):
    """B = 3, class 4: absent from the truth of sample 0, from the prediction of sample 1, from both in sample 2; the prediction of
    sample 0 also holds a label >= C"""
    pred = np.stack([ball_labels(shape, 30 + b) for b in range(3)])
    target = np.stack([ball_labels(shape, 30 + b, (1, 0, -1)) for b in range(3)])
    for L in (pred, target):
        L[L == 4] = 0
    pred[0, 1:3, 1:3, 1:4] = 4
    target[1, 2:4, 3:5, 4:8] = 4
    pred[0, 4, 4:6, 2:5] = 12
    return pred, target


def pattern_planes(shape):
    """random discs; one foreground pixel in each corner in turn; everything foreground but one pixel; an empty and a full plane;
    horizontal and vertical stripes; a checkerboard; a foreground only in the last row / the last column"""
    H, W = shape
    z = lambda: np.zeros(shape, np.uint8)
    planes = [blobs(shape, 1), blobs(shape, 2, n=2, value=200)]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        p = z()
        p[y, x] = 1
        planes.append(p)
    p = np.ones(shape, np.uint8)
    p[H // 2, (2 * W) // 3] = 0
    planes += [p, z(), np.full(shape, 3, np.uint8)]
    p = z()
    p[::2, :] = 1
    planes.append(p)
    p = z()
    p[:, 1::2] = 1
    planes.append(p)
    planes.append((np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8))
    p = z()
    p[H - 1, :] = 1
    planes.append(p)
    p = z()
    p[:, W - 1] = 255
    planes.append(p)
    return np.stack(planes)


EMPTY, FULL = 11, 12                 # indices in pattern_volumes


def pattern_volumes(shape):
    """the 3-D analogue of pattern_planes: random balls; one foreground voxel in each of the eight corners in turn; everything
    foreground but one voxel; an empty and a full volume; stripes along each axis; a 3-D checkerboard; a foreground only in the last
    slab of each axis"""
    X, Y, Z = shape
    z = lambda: np.zeros(shape, np.uint8)
    vols = [blobs(shape, 1), blobs(shape, 2, n=2, value=200)]
    for x in (0, X - 1):
        for y in (0, Y - 1):
            for k in (0, Z - 1):
                v = z()
                v[x, y, k] = 1
                vols.append(v)
    v = np.ones(shape, np.uint8)
    v[X // 2, (2 * Y) // 3, Z // 3] = 0
    vols += [v, z(), np.full(shape, 3, np.uint8)]
    assert len(vols) == FULL + 1
    for sl in ((slice(None, None, 2),), (slice(None), slice(1, None, 2)), (slice(None), slice(None), slice(None, None, 2))):
        v = z()
        v[sl] = 1
        vols.append(v)
    i, j, k = np.ogrid[:X, :Y, :Z]
    vols.append(((i + j + k) % 2).astype(np.uint8))
    for sl in ((X - 1,), (slice(None), Y - 1), (slice(None), slice(None), Z - 1)):
        v = z()
        v[sl] = 255
        vols.append(v)
    return np.stack(vols)
