"""The warping presets on the device (``ctseg_pipeline2d_warp_batch``): ``ElasticTransform`` / ``GridDistortion`` parameter holders,
the host draws and tables, and ``WarpPipeline2D``.

Per batch the host draws, per sample, the crop origin, rot90 / flip, which warp applies, and that warp's parameters: for an elastic
sample the three-point affine (solved and inverted in float64, as ``cv2.getAffineTransform`` / ``cv2.warpAffine`` do) and one 64-bit
seed of the displacement noise; for a grid sample the per-cell steps, turned into the float32 ``xx`` / ``yy`` map tables by the
reference's ``np.linspace`` loop.  The device does the rest in three launches (csrc/warp2d.hip).  albumentations' random stream is
not reproduced: the noise is a stateless hash of (seed, field, i, j), see DESIGN.md 6.2.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from .. import _native as nat
from .pipeline2d import _IMG_CODES, BatchPipeline2D, SliceStore2D, _host_array, window_bounds

NONE, ELASTIC, GRID = 0, 1, 2
COLS = 19                                # 8 of ctseg_pipeline2d_batch + kind, seed, 6 matrix entries, xx_off, yy_off, slot
FIELDS, PASS1, PASS2 = 1, 2, 4
MAX_SIDE, LDS_DOUBLES = 256, 6144        # limits of the fields kernel (W2_LINE_MAX, W2_LDS_DOUBLES)
_BORDER_REFLECT_101, _INTER_LINEAR = 4, 1


def _refuse(name, interpolation, border_mode, value, mask_value):
    if interpolation != _INTER_LINEAR or border_mode != _BORDER_REFLECT_101:
        raise NotImplementedError(f"{name}: only interpolation=cv2.INTER_LINEAR (1) and border_mode=cv2.BORDER_REFLECT_101 (4), the "
                                  "reference's defaults, are carried to the device")
    if value is not None or mask_value is not None:
        raise NotImplementedError(f"{name}: value / mask_value belong to BORDER_CONSTANT, which is not carried to the device")


class ElasticTransform:
    """A.ElasticTransform's parameters (the reference's constructor defaults)"""

    def __init__(self, alpha=1, sigma=50, alpha_affine=50, interpolation=_INTER_LINEAR, border_mode=_BORDER_REFLECT_101, value=None,
                 mask_value=None, always_apply=False, approximate=False, p=0.5):
        _refuse("ElasticTransform", interpolation, border_mode, value, mask_value)
        if approximate:
            raise NotImplementedError("ElasticTransform: approximate=True (a blurred field by cv2.GaussianBlur) is not carried to the device")
        self.alpha, self.sigma, self.alpha_affine = float(alpha), float(sigma), float(alpha_affine)
        assert self.sigma > 0 and abs(self.alpha) < 2 ** 20
        self.p = 1.0 if always_apply else float(p)


class GridDistortion:
    """A.GridDistortion's parameters (the reference's constructor defaults)"""

    def __init__(self, num_steps=5, distort_limit=0.3, interpolation=_INTER_LINEAR, border_mode=_BORDER_REFLECT_101, value=None,
                 mask_value=None, always_apply=False, p=0.5):
        _refuse("GridDistortion", interpolation, border_mode, value, mask_value)
        self.num_steps = int(num_steps)
        assert self.num_steps >= 1
        lim = (-abs(distort_limit), abs(distort_limit)) if np.isscalar(distort_limit) else tuple(distort_limit)
        self.distort_limit = (float(lim[0]), float(lim[1]))
        self.p = 1.0 if always_apply else float(p)


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter1d's kernel, float64: (radius, w[0..radius]) of the normalised symmetric weights"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    return radius, np.ascontiguousarray(phi[radius:])


def elastic_matrix(size, delta):
    """F.elastic_transform's random affine for a (height, width) crop: pts1 -> pts1 + delta ((3, 2) float32), float64 2 x 3.
    The reference puts (height, width) into the (x, y) slots of its points; so does this."""
    height, width = size
    center = np.float32((height, width)) // 2
    sq = min(height, width) // 3
    pts1 = np.float32([center + sq, [center[0] + sq, center[1] - sq], center - sq])
    pts2 = pts1 + np.asarray(delta, dtype=np.float32).reshape(3, 2)
    A = np.concatenate([pts1.astype(np.float64), np.ones((3, 1))], axis=1)
    try:
        return np.linalg.solve(A, pts2.astype(np.float64)).T.copy()
    except np.linalg.LinAlgError:                      # (pts1 is never collinear for a crop of 3 x 3 or more)
        return np.array([[1.0, 0, 0], [0, 1.0, 0]])


def invert_affine(M):
    """cv2.warpAffine's inversion of a forward 2 x 3 matrix, in float64 (a singular one becomes all-zero scales, as there)"""
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = M[1, 1] * D, M[0, 0] * D
    m0, m1, m3, m4 = a11, M[0, 1] * -D, M[1, 0] * -D, a22
    b1 = -m0 * M[0, 2] - m1 * M[1, 2]
    b2 = -m3 * M[0, 2] - m4 * M[1, 2]
    return np.array([m0, m1, b1, m3, m4, b2], dtype=np.float64)


def grid_table(width, num_steps, steps):
    """F.grid_distortion's map of one axis: float32 [width]; the last cell is clamped to the width"""
    step = width // num_steps
    if step < 1:
        raise ValueError(f"GridDistortion: {num_steps} steps do not fit a side of {width}")
    xx = np.zeros(width, np.float32)
    prev = 0
    for idx in range(num_steps + 1):
        start = idx * step
        end = start + step
        if end > width:
            end = width
            cur = width
        else:
            cur = prev + step * steps[idx]
        xx[start:end] = np.linspace(prev, cur, end - start)
        prev = cur
    return xx


def pipeline2d_warp_batch(store: SliceStore2D, table: np.ndarray, size, windows, shift=True, mean=None, denom=None, sigma=50.0, alpha=1.0,
                          xx=None, yy=None, want_masks=True, want_labels=False, want_present=False, launches=FIELDS | PASS1 | PASS2,
                          buffers=None, out=None):
    """The launches for the rows of ``table`` (B, 19) int64.  -> image, masks, labels, hist, present (as ``pipeline2d_batch``) and the
    buffers dict (fields (n, 2, Ho, Wo) fp32 of the elastic samples, field_tmp, inter), which a later call may be handed back.
    ``out``: preallocated outputs by name (image, masks, labels, hist, present; hist and present zeroed by the caller)."""
    nat.require_gpu(store.images, "WarpPipeline2D")
    dev = store.images.device
    table = np.ascontiguousarray(table, dtype=np.int64)
    assert table.ndim == 2 and table.shape[1] == COLS
    B, (Ho, Wo), K = table.shape[0], (int(v) for v in size), store.K
    has_masks = store.masks is not None and (want_masks or want_labels or want_present)
    Cw = len(windows)
    wl, wh = window_bounds(windows)
    lo, hi = _host_array(C.c_int32, wl), _host_array(C.c_int32, wh)
    mean_a = denom_a = None
    if mean is not None:
        mean_a = _host_array(C.c_float, [float(v) for v in mean])
        denom_a = _host_array(C.c_float, [float(v) for v in denom])
    n_slots = int((table[:, 8] == ELASTIC).sum())
    radius, gw = gaussian_weights(sigma)
    buffers = dict(buffers or {})
    if n_slots and "fields" not in buffers:
        buffers["fields"] = torch.empty((n_slots, 2, Ho, Wo), dtype=torch.float32, device=dev)
    if n_slots and "field_tmp" not in buffers:
        buffers["field_tmp"] = torch.empty((n_slots, 2, Ho, Wo), dtype=torch.float64, device=dev)
    inter_bytes = B * (Cw * 8 + (K if has_masks else 0)) * Ho * Wo
    if "inter" not in buffers:
        buffers["inter"] = torch.empty(((inter_bytes + 7) // 8,), dtype=torch.float64, device=dev)
    gw_dev = torch.from_numpy(gw).to(dev) if n_slots else None
    xx_dev = torch.from_numpy(np.ascontiguousarray(xx, dtype=np.float32)).to(dev) if xx is not None and len(xx) else None
    yy_dev = torch.from_numpy(np.ascontiguousarray(yy, dtype=np.float32)).to(dev) if yy is not None and len(yy) else None
    out = dict(out or {})
    image = out["image"] if "image" in out else torch.empty((B, Cw, Ho, Wo), dtype=torch.float32, device=dev)
    m_out = lab = hist = present = None
    if has_masks:
        if want_masks:
            m_out = out["masks"] if "masks" in out else torch.empty((B, K, Ho, Wo), dtype=torch.uint8, device=dev)
        if want_labels:
            lab = out["labels"] if "labels" in out else torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev)
            hist = out["hist"] if "hist" in out else torch.zeros((B, K + 1), dtype=torch.int64, device=dev)
        if want_present:
            present = out["present"] if "present" in out else torch.zeros((B, K), dtype=torch.int32, device=dev)
    assert image.shape == (B, Cw, Ho, Wo) and image.dtype == torch.float32 and image.is_contiguous()
    table_dev = torch.from_numpy(table).to(dev)
    fields, tmp, inter = buffers.get("fields"), buffers.get("field_tmp"), buffers["inter"]
    assert inter.numel() * inter.element_size() >= inter_bytes
    assert not n_slots or (fields.numel() >= n_slots * 2 * Ho * Wo and tmp.numel() >= n_slots * 2 * Ho * Wo)
    nat.call("ctseg_pipeline2d_warp_batch", nat.ptr(store.images), _IMG_CODES[store.images.dtype], store.images.numel(),
             nat.ptr(store.masks) if has_masks else None, store.masks.numel() if has_masks else 0, table_dev.data_ptr(),
             table.ctypes.data, B, K, Ho, Wo, Cw, lo, hi, int(bool(shift)), mean_a, denom_a, nat.ptr(gw_dev), radius, float(alpha),
             nat.ptr(xx_dev), 0 if xx_dev is None else xx_dev.numel(), nat.ptr(yy_dev), 0 if yy_dev is None else yy_dev.numel(),
             nat.ptr(fields), nat.ptr(tmp), n_slots, nat.ptr(inter), inter.numel() * inter.element_size(), nat.ptr(image),
             nat.ptr(m_out), nat.ptr(lab), nat.ptr(hist), nat.ptr(present), int(launches))
    return image, m_out, lab, hist, present, buffers


class WarpPipeline2D:
    """window -> RandomCrop(size) -> warps -> [RandomRotate90 -> HorizontalFlip] -> Normalize, the "train" side of the reference's
    warping presets.  ``warps``: one ``ElasticTransform`` and / or one ``GridDistortion``; ``oneof=False`` applies the (single) warp
    with its own ``p``; ``oneof=True`` is ``A.OneOf(warps, p=0.5)``: with probability 0.5 one warp, chosen with equal weight, is
    forced.  A sample takes at most one warp.

    ``pipe(store, indices, params=None, generator=None, with_masks=False) -> (images, masks_or_labels, present)`` as
    ``BatchPipeline2D`` (``with_masks``: a squashing pipeline also hands over the K masks as ``_ctseg_masks``).  ``params``:
    the explicit draws, a dict of ``crop`` (B, 4) y0, x0, k, flip; ``kind`` (B,) 0 none / 1 elastic / 2 grid; ``seed`` (B,) uint64
    and ``matrix`` (B, 2, 3) forward affine (elastic samples); ``xsteps`` / ``ysteps`` (B, num_steps + 1) (grid samples) — what
    ``draw_params`` returns."""

    def __init__(self, windows, size, mean=None, std=None, warps=(), oneof=False, rot_flip=True, squash=False, shift=True):
        self._crop = BatchPipeline2D(windows, "crop", size, mean, std, squash=squash, shift=shift)
        self.windows, self.size, self.shift, self.squash = self._crop.windows, self._crop.size, self._crop.shift, self._crop.squash
        self.mean, self.std, self.denom = self._crop.mean, self._crop.std, self._crop.denom
        self.warps = list(warps)
        self.oneof, self.rot_flip = bool(oneof), bool(rot_flip)
        el = [w for w in self.warps if isinstance(w, ElasticTransform)]
        gr = [w for w in self.warps if isinstance(w, GridDistortion)]
        if len(el) + len(gr) != len(self.warps) or len(el) > 1 or len(gr) > 1:
            raise NotImplementedError("WarpPipeline2D: warps are at most one ElasticTransform and one GridDistortion")
        if not self.oneof and len(self.warps) > 1:
            raise NotImplementedError("WarpPipeline2D: two warps in sequence on one sample are not carried to the device (use oneof=True)")
        self.elastic, self.grid = (el[0] if el else None), (gr[0] if gr else None)
        Ho, Wo = self.size
        if max(Ho, Wo) > MAX_SIDE:
            raise NotImplementedError(f"WarpPipeline2D: sides up to {MAX_SIDE}")
        if self.elastic is not None and max(Ho, Wo) + 2 * gaussian_weights(self.elastic.sigma)[0] > LDS_DOUBLES:
            raise NotImplementedError(f"WarpPipeline2D: sigma {self.elastic.sigma} is too wide for the fields kernel")
        if self.grid is not None and min(Ho, Wo) < self.grid.num_steps:
            raise ValueError(f"GridDistortion: {self.grid.num_steps} steps do not fit {Ho} x {Wo}")
        self._rng = np.random.default_rng()

    def squashing(self, squash: bool = True):
        """the same pipeline with the other kind of masks result"""
        p = WarpPipeline2D(self.windows, self.size, warps=self.warps, oneof=self.oneof, rot_flip=self.rot_flip, squash=squash, shift=self.shift)
        p.mean, p.std, p.denom = self.mean, self.std, self.denom
        p._crop.mean, p._crop.std, p._crop.denom = self.mean, self.std, self.denom
        return p

    def draw_kinds(self, B, generator=None):
        g = generator if generator is not None else self._rng
        codes = np.array([ELASTIC if isinstance(w, ElasticTransform) else GRID for w in self.warps], dtype=np.int64)
        if len(codes) == 0:
            return np.zeros(B, dtype=np.int64)
        if self.oneof:
            chosen = codes[g.integers(0, len(codes), size=B)]
            return np.where(g.random(B) < 0.5, chosen, NONE)
        return np.where(g.random(B) < self.warps[0].p, codes[0], NONE)

    def draw_params(self, sizes, generator=None):
        g = generator if generator is not None else self._rng
        Ho, Wo = self.size
        crop = self._crop.draw_params(sizes, g)
        if not self.rot_flip:
            crop[:, 2:] = 0
        B = len(crop)
        out = {"crop": crop, "kind": self.draw_kinds(B, g), "seed": np.zeros(B, dtype=np.uint64), "matrix": np.zeros((B, 2, 3))}
        out["matrix"][:, 0, 0] = out["matrix"][:, 1, 1] = 1.0
        if self.elastic is not None:
            aa = self.elastic.alpha_affine
            for b in np.flatnonzero(out["kind"] == ELASTIC):
                out["matrix"][b] = elastic_matrix((Ho, Wo), g.uniform(-aa, aa, size=(3, 2)).astype(np.float32))
                out["seed"][b] = g.integers(0, 2 ** 64, dtype=np.uint64)
        if self.grid is not None:
            lo, hi = self.grid.distort_limit
            out["xsteps"] = 1 + g.uniform(lo, hi, size=(B, self.grid.num_steps + 1))
            out["ysteps"] = 1 + g.uniform(lo, hi, size=(B, self.grid.num_steps + 1))
        return out

    def build_table(self, store_rows, p):
        """(B, 4) rows of the store's table + the draws -> the (B, 19) table and the xx / yy map tables"""
        Ho, Wo = self.size
        B = len(store_rows)
        crop = np.asarray(p["crop"], dtype=np.int64).reshape(-1, 4)
        kind = np.asarray(p["kind"], dtype=np.int64).reshape(-1)
        if crop.shape[0] != B or kind.shape[0] != B:
            raise ValueError("WarpPipeline2D: one row of draws per index")
        if ((kind < NONE) | (kind > GRID)).any() or ((kind == ELASTIC).any() and self.elastic is None) or ((kind == GRID).any() and self.grid is None):
            raise ValueError("WarpPipeline2D: a kind this pipeline has no warp for")
        table = np.zeros((B, COLS), dtype=np.int64)
        table[:, :4] = store_rows
        table[:, 4:8] = crop
        table[:, 8] = kind
        table[:, 9] = np.asarray(p.get("seed", np.zeros(B, np.uint64)), dtype=np.uint64).view(np.int64)
        ident = np.array([1.0, 0, 0, 0, 1.0, 0]).view(np.int64)
        xx, yy, slot = [], [], 0
        for b in range(B):
            table[b, 10:16] = ident
            if kind[b] == ELASTIC:
                table[b, 10:16] = invert_affine(p["matrix"][b]).view(np.int64)
                table[b, 18] = slot
                slot += 1
            elif kind[b] == GRID:
                table[b, 16], table[b, 17] = Wo * len(xx), Ho * len(yy)
                xx.append(grid_table(Wo, self.grid.num_steps, p["xsteps"][b]))
                yy.append(grid_table(Ho, self.grid.num_steps, p["ysteps"][b]))
        return table, (np.concatenate(xx) if xx else None), (np.concatenate(yy) if yy else None)

    def __call__(self, store: SliceStore2D, indices, *, params=None, generator=None, with_masks=False):
        nat.require_gpu(store.images, "WarpPipeline2D")
        idx = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
        if len(idx) == 0 or idx.min() < 0 or idx.max() >= len(store):
            raise IndexError(f"WarpPipeline2D: slice indices outside [0, {len(store)})")
        rows = store.table[idx]
        p = self.draw_params(rows[:, 2:4], generator) if params is None else params
        table, xx, yy = self.build_table(rows, p)
        Ho, Wo = self.size
        c = table[:, 4:8]
        bad = (c[:, 0] < 0) | (c[:, 1] < 0) | (c[:, 0] + Ho > table[:, 2]) | (c[:, 1] + Wo > table[:, 3])
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            raise nat.NativeError(f"WarpPipeline2D: crop origin {c[b, :2].tolist()} + {Ho} x {Wo} leaves slice {int(idx[b])} "
                                  f"({table[b, 2]} x {table[b, 3]})")
        el = self.elastic
        image, m_out, lab, hist, present, _ = pipeline2d_warp_batch(
            store, table, self.size, self.windows, self.shift, self.mean, self.denom, sigma=el.sigma if el else 1.0,
            alpha=el.alpha if el else 0.0, xx=xx, yy=yy, want_masks=not self.squash or with_masks, want_labels=self.squash,
            want_present=True)
        masks = lab if self.squash else m_out
        if masks is not None:
            masks._ctseg_present = present
            if self.squash:
                masks._ctseg_labels = (lab.reshape(len(idx), -1), hist)
                if with_masks:
                    masks._ctseg_masks = m_out
        return image, masks, present
