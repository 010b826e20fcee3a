"""The batched 2-D input pipeline (``ctseg_pipeline2d_batch``): slice store, launch wrapper and ``BatchPipeline2D``.

``SliceStore2D`` holds every raw slice of a split on the device, uploaded once: the image elements back to back (``int16``,
``uint8`` or ``float32``), the mask bytes back to back as ``[K][H][W]`` planes, and a host table ``(N, 4)`` of
``image_off, mask_off, H, W`` (slices are cropped per patient and differ in size).  ``BatchPipeline2D`` runs window ->
crop/rot90/flip or resize -> normalize (-> squash) for a list of slice indices in one launch.  There is no CPU fallback.
"""
from typing import Optional, Sequence

import ctypes as C

import numpy as np
import torch

from .. import _native as nat

CROP, RESIZE = 0, 1
_MODES = {"crop": CROP, "resize": RESIZE, CROP: CROP, RESIZE: RESIZE}
_IMG_CODES = {torch.float32: nat.F32, torch.int16: nat.I16, torch.uint8: nat.U8}
_NP_KEEP = (np.dtype(np.int16), np.dtype(np.uint8), np.dtype(np.float32))


class SliceStore2D:
    """images: sequence of (H, W) arrays of one dtype (int16 / uint8 / float32 are kept, anything else is stored as float32);
    masks: sequence of (K, H, W) bool / uint8 arrays (or None: an image-only store)."""

    def __init__(self, images: Sequence, masks: Optional[Sequence] = None, device="cuda"):
        images = [np.asarray(im) for im in images]
        assert len(images) > 0, "an empty slice store"
        assert all(im.ndim == 2 for im in images), "slices are (H, W)"
        dt = images[0].dtype if images[0].dtype in _NP_KEEP else np.dtype(np.float32)
        sizes = np.array([im.shape for im in images], dtype=np.int64)
        npix = sizes[:, 0] * sizes[:, 1]
        self.K = 0
        table = np.zeros((len(images), 4), dtype=np.int64)
        table[:, 0] = np.concatenate(([0], np.cumsum(npix)[:-1]))
        table[:, 2:] = sizes
        flat_m = None
        if masks is not None:
            masks = [np.asarray(m) for m in masks]
            assert len(masks) == len(images)
            self.K = masks[0].shape[0]
            for m, im in zip(masks, images):
                assert m.shape == (self.K,) + im.shape, "masks are (K, H, W) of their slice"
            table[:, 1] = table[:, 0] * self.K
            flat_m = np.concatenate([np.ascontiguousarray(m).view(np.uint8).reshape(-1) if m.dtype == np.bool_
                                     else np.ascontiguousarray(m, dtype=np.uint8).reshape(-1) for m in masks])
        flat_i = np.concatenate([np.ascontiguousarray(im, dtype=dt).reshape(-1) for im in images])
        self.device = torch.device(device)
        self.table = table
        self.images = torch.from_numpy(flat_i).to(self.device)
        self.masks = torch.from_numpy(flat_m).to(self.device) if flat_m is not None else None

    def __len__(self):
        return len(self.table)

    def raw(self, index):
        """the untransformed slice as views of the store: image (H, W), masks (K, H, W) or None"""
        io, mo, H, W = (int(v) for v in self.table[index])
        image = self.images[io:io + H * W].view(H, W)
        masks = self.masks[mo:mo + self.K * H * W].view(self.K, H, W) if self.masks is not None else None
        return image, masks


def _host_array(ctype, values):
    return (ctype * len(values))(*values)


def window_bounds(windows):
    """[(width, level), ...] -> (lo, hi) integer lists of apply_window: level -+ width // 2"""
    return [int(l - (w // 2)) for w, l in windows], [int(l + (w // 2)) for w, l in windows]


def pipeline2d_batch(store: SliceStore2D, table: np.ndarray, mode: int, size, windows, shift=True, mean=None, denom=None,
                     want_image=True, want_masks=True, want_labels=False, want_present=False):
    """One launch for the rows of ``table`` (B, 8) int64: image_off, mask_off, H, W, y0, x0, k, flip.
    -> image (B,C,Ho,Wo) fp32, masks (B,K,Ho,Wo) u8, labels (B,Ho,Wo) u8, hist (B,K+1) int64, present (B,K) int32 (None when
    not asked for)."""
    nat.require_gpu(store.images, "BatchPipeline2D")
    dev = store.images.device
    table = np.ascontiguousarray(table, dtype=np.int64)
    B, (Ho, Wo), K = table.shape[0], (int(v) for v in size), store.K
    has_masks = store.masks is not None and (want_masks or want_labels or want_present)
    image = m_out = lab = hist = present = None
    lo = hi = mean_a = denom_a = None
    Cw = 0
    if want_image:
        Cw = len(windows)
        wl, wh = window_bounds(windows)
        lo, hi = _host_array(C.c_int32, wl), _host_array(C.c_int32, wh)
        if mean is not None:
            mean_a = _host_array(C.c_float, [float(v) for v in mean])
            denom_a = _host_array(C.c_float, [float(v) for v in denom])
        image = torch.empty((B, Cw, Ho, Wo), dtype=torch.float32, device=dev)
    if has_masks:
        if want_masks:
            m_out = torch.empty((B, K, Ho, Wo), dtype=torch.uint8, device=dev)
        if want_labels:
            lab = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev)
            hist = torch.zeros((B, K + 1), dtype=torch.int64, device=dev)
        if want_present:
            present = torch.zeros((B, K), dtype=torch.int32, device=dev)
    table_dev = torch.from_numpy(table).to(dev)
    nat.call("ctseg_pipeline2d_batch", nat.ptr(store.images) if want_image else None, _IMG_CODES[store.images.dtype],
             store.images.numel(), nat.ptr(store.masks) if has_masks else None, store.masks.numel() if has_masks else 0,
             table_dev.data_ptr(), table.ctypes.data, B, K, mode, Ho, Wo, Cw, lo, hi, int(bool(shift)), mean_a, denom_a,
             nat.ptr(image), nat.ptr(m_out), nat.ptr(lab), nat.ptr(hist), nat.ptr(present))
    return image, m_out, lab, hist, present


class BatchPipeline2D:
    """``windows``: [(width, level), ...] (1 or 3 of them); ``mode``: "crop" (RandomCrop -> RandomRotate90 -> HorizontalFlip) or
    "resize" (A.Resize); ``size``: (Ho, Wo); ``mean`` / ``std``: A.Normalize's per-channel statistics (max_pixel_value = 1.0), or
    None for no normalization; ``squash``: hand back the (B, Ho, Wo) label maps instead of the K masks.

    ``pipe(store, indices, params=None, generator=None) -> (images, masks_or_labels, present)``.  ``params`` is an explicit (B, 4)
    table of y0, x0, k, flip ("crop" only).  Without it the values are drawn on the host from ``generator`` (a
    ``numpy.random.Generator``) with the reference's probabilities: crop origin uniform over the valid range, rot90 with p = 0.5
    and then k uniform in 0..3 (0 or 2 for a non-square size), flip with p = 0.5.  albumentations' own stream is not reproduced.
    The masks result carries ``_ctseg_present`` and, when squashing, ``_ctseg_labels`` = (labels (B, S), hist); with
    ``with_masks=True`` a squashing pipeline also writes the K unsquashed masks in the same launch and hands them over as
    ``_ctseg_masks`` (structures can overlap: they cannot be taken back from the labels)."""

    def __init__(self, windows, mode, size, mean=None, std=None, squash: bool = False, shift: bool = True):
        self.windows = [tuple(int(v) for v in w) for w in windows]
        assert 1 <= len(self.windows) <= 4
        self.mode = _MODES[mode]
        self.size = (int(size[0]), int(size[1]))
        self.squash, self.shift = bool(squash), bool(shift)
        self.mean = self.std = self.denom = None
        if mean is not None:
            mean, std = np.atleast_1d(mean), np.atleast_1d(std)
            assert len(mean) == len(std) == len(self.windows), "one mean / std per window"
            self.mean = np.asarray(mean, dtype=np.float32)          # A.Normalize: mean * max_pixel_value, as float32
            self.std = np.asarray(std, dtype=np.float32)
            self.denom = np.reciprocal(self.std)
        self._rng = np.random.default_rng()

    def squashing(self, squash: bool = True):
        """the same pipeline with the other kind of masks result"""
        p = BatchPipeline2D(self.windows, self.mode, self.size, squash=squash, shift=self.shift)
        p.mean, p.std, p.denom = self.mean, self.std, self.denom
        return p

    def draw_params(self, sizes, generator=None):
        """(B, 2) slice sizes H, W -> (B, 4) y0, x0, k, flip"""
        g = generator if generator is not None else self._rng
        Ho, Wo = self.size
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        if (sizes[:, 0] < Ho).any() or (sizes[:, 1] < Wo).any():
            raise nat.NativeError(f"BatchPipeline2D: a {Ho} x {Wo} crop does not fit every slice (smallest: {sizes.min(0).tolist()})")
        B = len(sizes)
        out = np.zeros((B, 4), dtype=np.int64)
        out[:, 0] = g.integers(0, sizes[:, 0] - Ho + 1)
        out[:, 1] = g.integers(0, sizes[:, 1] - Wo + 1)
        k = g.integers(0, 4, size=B) if Ho == Wo else 2 * g.integers(0, 2, size=B)
        out[:, 2] = np.where(g.random(B) < 0.5, k, 0)
        out[:, 3] = g.random(B) < 0.5
        return out

    def __call__(self, store: SliceStore2D, indices, *, params=None, generator=None, with_masks=False):
        nat.require_gpu(store.images, "BatchPipeline2D")
        idx = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
        if len(idx) == 0 or idx.min() < 0 or idx.max() >= len(store):
            raise IndexError(f"BatchPipeline2D: slice indices outside [0, {len(store)})")
        table = np.zeros((len(idx), 8), dtype=np.int64)
        table[:, :4] = store.table[idx]
        if self.mode == CROP:
            p = self.draw_params(table[:, 2:4], generator) if params is None else np.asarray(params, dtype=np.int64).reshape(-1, 4)
            if p.shape[0] != len(idx):
                raise ValueError("BatchPipeline2D: one (y0, x0, k, flip) row per index")
            Ho, Wo = self.size
            bad = (p[:, 0] < 0) | (p[:, 1] < 0) | (p[:, 0] + Ho > table[:, 2]) | (p[:, 1] + Wo > table[:, 3])
            if bad.any():
                b = int(np.flatnonzero(bad)[0])
                raise nat.NativeError(f"BatchPipeline2D: crop origin {p[b, :2].tolist()} + {Ho} x {Wo} leaves slice "
                                      f"{int(idx[b])} ({table[b, 2]} x {table[b, 3]})")
            table[:, 4:] = p
        elif params is not None:
            raise ValueError("BatchPipeline2D: params belong to the crop mode")
        image, m_out, lab, hist, present = pipeline2d_batch(
            store, table, self.mode, self.size, self.windows, self.shift, self.mean, self.denom,
            want_masks=not self.squash or with_masks, want_labels=self.squash, want_present=True)
        masks = lab if self.squash else m_out
        if masks is not None:
            masks._ctseg_present = present
            if self.squash:
                masks._ctseg_labels = (lab.reshape(len(idx), -1), hist)
                if with_masks:
                    masks._ctseg_masks = m_out
        return image, masks, present
