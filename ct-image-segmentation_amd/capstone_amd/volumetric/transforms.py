"""Device-side 3-D input pipeline — drop-in for reference capstone/volumetric/transforms.py.

``Resize3D`` (:9-32, ``F.interpolate`` nearest to ``size`` = D×H×W) and ``ToTensorV3`` (:35-49, (C,D,H,W) -> (C,H,W,D)) keep
their names, constructor arguments and ``apply`` / ``apply_to_mask`` methods but take **GPU tensors** (the raw ``.npz`` arrays
uploaded once) and run as one HIP pass, ``ctseg_resize3d_to_hwd``: the resize writes (H,W,D)-contiguous storage straight away and
``Resize3D`` hands back the (D,H,W) *view* of it, so ``ToTensorV3``'s permute — the composition of
volumetric/predefined.py:4-7 — ends on a contiguous tensor with no further copy.

``InstancePipeline3D`` is the fused form used by ``datasets.MiccaiDataset3D``: image resize + permute (+ optional HU window,
capstone/transforms/transforms_2d.py:97-107, which the reference's 3-D path omits) and the nine masks resized, permuted and —
with ``squash=True`` — reduced to the label map of ``_squash_masks_3D`` (volumetric/utils.py:4-7) in the same pass: 1 byte
per voxel leaves the kernel instead of 9, and the trainer's squash pass disappears.

``Augment3D`` is the spatial and intensity augmentation of that pipeline, which the reference's 3-D path lacks: random rotation,
zoom, shift and mirror as one 3 x 4 matrix, drawn on the host and applied by ``ctseg_augment3d_to_hwd`` in the same single pass
(``augment3d_to_hwd``).  A left-right mirror swaps the paired structures' mask channels, see ``Augment3D.channel_src``.
``Deform3D`` adds a non-rigid part to that pass: a cubic B-spline free-form deformation over a coarse control lattice, which the
device fills from a drawn seed (``ctseg_deform3d_lattice``, then ``ctseg_augment3d_deform_to_hwd``).
``Intensity3D`` is the second, small stage on that pass' (H', W', D') output: Gaussian blur, additive Gaussian noise and a gamma
curve (``intensity3d`` -> ``ctseg_intensity3d``), which cannot go into the gather pass: a blur needs a voxel's neighbours on the
output grid, and noise and gamma come after the window.
``PatchSampler3D`` is the other route into the trainer: fixed-size patches of the raw volume at its own resolution, most of them
centred on a voxel of a randomly chosen structure.  The device picks the centres (``patch_centres`` -> ``ctseg_patch_centres``) and
the crop pass reads them there (``patch3d_to_hwd`` -> ``ctseg_patch3d_to_hwd``, the affine pass about a device-side centre).
There is no CPU fallback: CPU tensors raise ``NativeError``.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native as nat
from ..data.utils import compute_distance_map
from ..transforms.transforms_2d import WINDOWING_CONFIG

_IMG_DTYPES = {torch.float32: nat.F32, torch.int16: nat.I16, torch.uint8: nat.U8}


def _image_code(image):
    if image.dtype not in _IMG_DTYPES:
        image = image.float()
    return image.contiguous(), _IMG_DTYPES[image.dtype]


def _window_args(window):
    """window = None | (width, level) | (width, level, shift): the reference's apply_window(image, width, level, shift)"""
    if window is None:
        return 0, 0.0, 1.0
    width, level = window[0], window[1]
    shift = window[2] if len(window) > 2 else True
    return (2 if shift else 1), float(level - (width // 2)), float(level + (width // 2))


def _prepare_call(image, masks, size, who, want_masks, want_labels, outs=None):
    """the inputs and outputs of one resample call -> image (D,H,W) contiguous and its dtype code, masks (K,D,H,W) uint8
    contiguous and K, (D, H, W, D', H', W'), and the outputs (image, masks, labels, hist), None where not asked for.
    ``outs``: the caller's own outputs in that order (contiguous, ``hist`` zeroed) instead of new tensors"""
    ref = image if image is not None else masks
    nat.require_gpu(ref, who)
    D, H, W = ref.shape[-3:]
    Do, Ho, Wo = (int(v) for v in size)
    dev = ref.device
    img_out = m_out = lab = hist = None
    code, K = nat.F32, 0
    if image is not None:
        image, code = _image_code(image.reshape(D, H, W))
        if outs is None:
            img_out = torch.empty((Ho, Wo, Do), dtype=torch.float32, device=dev)
    if masks is not None:
        masks = masks.reshape(-1, D, H, W)
        if masks.dtype != torch.uint8:
            masks = masks.to(torch.uint8)
        masks = masks.contiguous()
        K = masks.shape[0]
        if want_masks and outs is None:
            m_out = torch.empty((K, Ho, Wo, Do), dtype=torch.uint8, device=dev)
        if want_labels and outs is None:
            lab = torch.empty((Ho, Wo, Do), dtype=torch.uint8, device=dev)
            hist = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    if outs is not None:
        img_out, m_out, lab, hist = outs
        for t, shape, dtype in ((img_out, (Ho, Wo, Do), torch.float32), (m_out, (K, Ho, Wo, Do), torch.uint8),
                                (lab, (Ho, Wo, Do), torch.uint8), (hist, (K + 1,), torch.int64)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"{who}: an output is a contiguous {dtype} tensor of shape {shape} on the inputs' device")
    return image, code, masks, K, (D, H, W, Do, Ho, Wo), (img_out, m_out, lab, hist)


def _c_matrix(matrix):
    """a (3, 4) matrix as the 12 floats an entry reads; the caller keeps the object alive across the call"""
    return (ctypes.c_float * 12)(*np.asarray(matrix, dtype=np.float32).reshape(12).tolist())


def _c_permutation(values, n, who, what):
    """``values`` (None: the identity) as the ``n`` int32 an entry reads, or None; ``who`` names the argument and ``what`` the
    things it permutes in the message.  The caller keeps the object alive across the call"""
    if values is None:
        return None
    src = [int(v) for v in values]
    if len(src) != n:
        raise nat.NativeError(f"{who} has {len(src)} entries for {n} {what}")
    return (ctypes.c_int32 * n)(*src)


def resize3d_to_hwd(image: Optional[torch.Tensor], masks: Optional[torch.Tensor], size: Sequence[int], window=None,
                    want_masks: bool = True, want_labels: bool = False):
    """image (D,H,W) f32/i16/u8, masks (K,D,H,W) u8 -> image (H',W',D') fp32, masks (K,H',W',D') u8, labels (H',W',D') u8, hist (K+1)"""
    image, code, masks, K, dims, outs = _prepare_call(image, masks, size, "Resize3D", want_masks, want_labels)
    nat.call("ctseg_resize3d_to_hwd", nat.ptr(image), code, nat.ptr(masks), K, *dims, *_window_args(window), *(nat.ptr(t) for t in outs))
    return outs


_BORDERS = {"constant": 0, "edge": 1}
_INTERPS = {"nearest": 0, "trilinear": 1}
# the control lattice of the deformed pass: one small fp32 tensor per (device, stream), grown when a larger one is asked for.  The
# lattice launch and the pass that reads it go to the same stream, so the next instance's lattice launch is ordered behind this
# instance's pass: reusing the buffer needs no synchronisation.
_LATTICES = {}


def _check_deform(cells, magnitude, size):
    """the limits of a lattice of ``cells`` over the ``size`` = (D', H', W') grid: a cell of at least 4 voxels (the kernel's slab)
    and a control-point displacement of at most 0.4 of a cell, below which a cubic B-spline deformation cannot fold"""
    for a, (g, m, n) in enumerate(zip(cells, magnitude, size)):
        if g < 1 or 4 * g > n:
            raise ValueError(f"Deform3D: {g} cells over {n} voxels along axis {'dhw'[a]}: a cell has at least 4 voxels")
        if not (np.isfinite(m) and 0.0 <= m <= 0.4 * n / g):
            raise ValueError(f"Deform3D: magnitude {m} along axis {'dhw'[a]} is outside [0, 0.4 cells] = [0, {0.4 * n / g:g}] voxels")


def _lattice(deform, device):
    """the cached lattice buffer filled for ``deform`` (any lattice the entry accepts: ``Deform3D.check`` has the preset's limits)"""
    cells = tuple(int(v) for v in deform["cells"])
    magnitude = tuple(float(v) for v in deform["magnitude"])
    n = 3 * (cells[0] + 3) * (cells[1] + 3) * (cells[2] + 3)
    key = (device, nat.stream_ptr())
    buf = _LATTICES.get(key)
    if buf is None or buf.numel() < n:
        _LATTICES[key] = buf = torch.empty(n, dtype=torch.float32, device=device)
    c_cells = (ctypes.c_int32 * 3)(*cells)
    c_mag = (ctypes.c_float * 3)(*magnitude)
    nat.call("ctseg_deform3d_lattice", int(deform["seed"]), ctypes.addressof(c_cells), ctypes.addressof(c_mag), nat.ptr(buf), n)
    return buf, c_cells


def augment3d_to_hwd(image: Optional[torch.Tensor], masks: Optional[torch.Tensor], size: Sequence[int], matrix, interp=1,
                     border="constant", cval: float = 0.0, mask_src=None, window=None, gain: float = 1.0, bias: float = 0.0,
                     want_masks: bool = True, want_labels: bool = False, deform: Optional[dict] = None):
    """``resize3d_to_hwd`` with the output voxel sent through ``matrix`` first: (3, 4), rows and columns ordered d, h, w, mapping an
    OUTPUT voxel of the ``size`` grid to the point of that same grid it samples (include/ctseg_hip.h has the rules).  ``interp``
    0 / "nearest" or 1 / "trilinear" for the image (masks are always nearest), ``border`` "constant" (image ``cval``, masks 0) or
    "edge"; output mask channel k reads input channel ``mask_src[k]``; the windowed value becomes ``v * gain + bias``.
    ``deform`` = {"seed", "cells", "magnitude"} (``Deform3D``): the device fills the control lattice from the seed and the pass
    adds its B-spline displacement to the sampling point, two launches instead of one.
    -> image (H',W',D') fp32, masks (K,H',W',D') u8, labels (H',W',D') u8, hist (K+1)"""
    image, code, masks, K, dims, outs = _prepare_call(image, masks, size, "Augment3D", want_masks, want_labels)
    mat = _c_matrix(matrix)
    src = _c_permutation(mask_src, K, "Augment3D: mask_src", "mask channels")
    args = (nat.ptr(image), code, nat.ptr(masks), K, *dims,
            ctypes.addressof(mat), _INTERPS.get(interp, interp), _BORDERS.get(border, border), float(cval),
            ctypes.addressof(src) if src is not None else None, *_window_args(window), float(gain), float(bias),
            *(nat.ptr(t) for t in outs))
    if deform is None:
        nat.call("ctseg_augment3d_to_hwd", *args)
    else:
        lattice, cells = _lattice(deform, (image if image is not None else masks).device)
        nat.call("ctseg_augment3d_deform_to_hwd", *args, nat.ptr(lattice), ctypes.addressof(cells))
    return outs


# the block counts of the centre pick: one int32 buffer per (device, stream), grown on demand, reused as the lattice above is (the
# next call's count pass is ordered behind this call's select pass on the same stream)
_PATCH_WORKSPACES = {}
_MAX_PATCHES = 16


def _c_draws(draws):
    """P rows (fg, a, b) as the P x 3 uint32 the centre pick reads: fg is any truth value, a and b are integers in [0, 2^32)"""
    rows = [(1 if fg else 0, int(a), int(b)) for fg, a, b in draws]
    if not 1 <= len(rows) <= _MAX_PATCHES:
        raise ValueError(f"patch_centres: {len(rows)} draws, 1 to {_MAX_PATCHES} patches are taken per call")
    if not all(0 <= v < 2 ** 32 for row in rows for v in row[1:]):
        raise ValueError("patch_centres: a and b are integers in [0, 2^32)")
    return (ctypes.c_uint32 * (3 * len(rows)))(*(v for row in rows for v in row)), len(rows)


def patch_centres(masks: torch.Tensor, draws, patch=None, class_mask: Optional[int] = None,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """P patch centres on the device (``ctseg_patch_centres``; include/ctseg_hip.h has the rule word for word).  ``masks``
    (K,D,H,W) uint8 on the device, K <= 15; ``draws`` = P <= 16 host rows (fg, a, b): with fg set, the class is the
    ``a * m >> 32``-th of the m eligible classes (bit k of ``class_mask`` set, default all, and mask k not empty) and the centre
    the ``b * n >> 32``-th of its n set voxels in raster order; otherwise (or with no eligible class) the class is -1 and the
    centre is voxel ``b * D*H*W >> 32``.  ``patch`` = (d, h, w) clamps the centre so that a patch starting at ``c - patch // 2``
    stays inside the volume.  ``workspace``: the caller's int32 scratch of ``ctseg_patch_centres_workspace`` bytes, any content
    (default: a cached one per device and stream).  -> (P, 4) int32 device tensor, rows (d, h, w, class); nothing is read back"""
    nat.require_gpu(masks, "patch_centres")
    if masks.dim() != 4 or masks.dtype != torch.uint8:
        raise ValueError("patch_centres: masks is a (K, D, H, W) uint8 tensor")
    masks = masks.contiguous()
    K, D, H, W = masks.shape
    c_draws, P = _c_draws(draws)
    need = nat.lib().ctseg_patch_centres_workspace(K, D, H, W)
    if need < 0:
        nat.check(-1, "ctseg_patch_centres_workspace")
    if workspace is None:
        key = (masks.device, nat.stream_ptr())
        workspace = _PATCH_WORKSPACES.get(key)
        if workspace is None or workspace.numel() * 4 < need:
            _PATCH_WORKSPACES[key] = workspace = torch.empty(need // 4, dtype=torch.int32, device=masks.device)
    elif workspace.dtype != torch.int32 or not workspace.is_contiguous() or workspace.device != masks.device:
        raise ValueError("patch_centres: workspace is a contiguous int32 tensor on the masks' device")
    c_patch = None if patch is None else (ctypes.c_int32 * 3)(*(int(v) for v in patch))
    centres = torch.empty((P, 4), dtype=torch.int32, device=masks.device)
    nat.call("ctseg_patch_centres", nat.ptr(masks), K, D, H, W, ctypes.addressof(c_draws), P,
             (1 << K) - 1 if class_mask is None else int(class_mask), ctypes.addressof(c_patch) if c_patch is not None else None,
             nat.ptr(workspace), workspace.numel() * 4, nat.ptr(centres))
    return centres


def patch_matrix(patch, matrix=None) -> np.ndarray:
    """the (3, 4) float32 matrix of a patch of ``patch`` = (d, h, w) voxels about its centre: ``matrix`` (a float64 map of the
    patch grid onto itself such as ``Augment3D.matrix(patch, params, np.float64)``; None: the identity) with ``patch // 2``
    subtracted from its translation, rounded to float32 once.  The identity gives whole sampling coordinates: an exact crop"""
    out = np.eye(3, 4, dtype=np.float64) if matrix is None else np.array(matrix, dtype=np.float64).reshape(3, 4)
    out[:, 3] -= np.asarray([int(v) // 2 for v in patch], dtype=np.float64)
    return out.astype(np.float32)


def patch3d_to_hwd(image: Optional[torch.Tensor], masks: Optional[torch.Tensor], patch: Sequence[int], matrix, centre: torch.Tensor,
                   interp=1, border="constant", cval: float = 0.0, mask_src=None, window=None, gain: float = 1.0, bias: float = 0.0,
                   want_masks: bool = True, want_labels: bool = False, outs=None):
    """``augment3d_to_hwd`` on a patch about a centre that stays on the device (``ctseg_patch3d_to_hwd``): ``matrix`` maps an
    output voxel of the ``patch`` = (d, h, w) grid to a point of the SOURCE grid, relative to ``centre``, an int32 device tensor
    whose first three entries are (d, h, w), such as a row of ``patch_centres``' table; the kernel adds the centre to the
    translation column, one float32 add per axis, and is the affine pass with that matrix from there on.  There is no resize: the
    patch has the source's resolution.  ``patch_matrix(patch)`` is the exact crop ``src[c - patch // 2 + o]``.  ``outs``: the
    caller's own output tensors (image, masks, labels, hist; ``hist`` zeroed) instead of new ones.
    -> image (h,w,d) fp32, masks (K,h,w,d) u8, labels (h,w,d) u8, hist (K+1)"""
    image, code, masks, K, dims, outs = _prepare_call(image, masks, patch, "patch3d_to_hwd", want_masks, want_labels, outs)
    ref = image if image is not None else masks
    if centre.dtype != torch.int32 or centre.numel() < 3 or not centre.is_contiguous() or centre.device != ref.device:
        raise ValueError("patch3d_to_hwd: centre is a contiguous int32 tensor of at least 3 entries (d, h, w) on the inputs' device")
    mat = _c_matrix(matrix)
    src = _c_permutation(mask_src, K, "patch3d_to_hwd: mask_src", "mask channels")
    nat.call("ctseg_patch3d_to_hwd", nat.ptr(image), code, nat.ptr(masks), K, *dims, ctypes.addressof(mat), nat.ptr(centre),
             _INTERPS.get(interp, interp), _BORDERS.get(border, border), float(cval),
             ctypes.addressof(src) if src is not None else None, *_window_args(window), float(gain), float(bias),
             *(nat.ptr(t) for t in outs))
    return outs


_MAX_SIGMA, _MAX_RADIUS = 4.0, 12


def gaussian_taps(sigma: float):
    """(r, taps) of one blurred axis: r = ceil(3 sigma) and the r + 1 float32 taps exp(-k^2 / (2 sigma^2)), k = 0..r, normalised in
    float64 so that w_0 + 2 sum_{k>=1} w_k = 1 and rounded once"""
    sigma = float(sigma)
    if not 0.0 < sigma <= _MAX_SIGMA:
        raise ValueError(f"intensity3d: sigma {sigma} is outside (0, {_MAX_SIGMA}] (0 skips the axis)")
    r = int(np.ceil(3.0 * sigma))
    k = np.arange(r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return r, (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def _check_range(value_range, who):
    if value_range is None:
        return None
    lo, hi = (float(v) for v in value_range)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"{who}: value_range is (lo, hi), finite, lo < hi")
    return lo, hi


def _check_intensity(sigma, noise_std, noise_seed, gamma, value_range, who="intensity3d"):
    """the stage's parameters as the entry takes them, or ``ValueError``: sigma per axis d, h, w, each 0 (axis skipped) or in
    (0, 4]; noise_std finite and >= 0; a seed of 64 bits; gamma in [0.25, 4] over a value range, or exactly 1 without one"""
    sigma = tuple(float(v) for v in sigma)
    if len(sigma) != 3 or not all(0.0 <= v <= _MAX_SIGMA for v in sigma):
        raise ValueError(f"{who}: sigma has one entry per axis d, h, w, each in [0, {_MAX_SIGMA}]")
    noise_std, gamma, noise_seed = float(noise_std), float(gamma), int(noise_seed)
    if not (np.isfinite(noise_std) and noise_std >= 0.0):
        raise ValueError(f"{who}: noise_std is finite and not negative")
    if not -2 ** 63 <= noise_seed < 2 ** 64:
        raise ValueError(f"{who}: noise_seed has 64 bits")
    value_range = _check_range(value_range, who)
    if value_range is None and gamma != 1.0:
        raise ValueError(f"{who}: gamma {gamma} needs a value_range (lo, hi)")
    if not 0.25 <= gamma <= 4.0:
        raise ValueError(f"{who}: gamma {gamma} is outside [0.25, 4]")
    return sigma, noise_std, noise_seed - 2 ** 64 if noise_seed >= 2 ** 63 else noise_seed, gamma, value_range


def intensity3d(image: torch.Tensor, sigma=(0, 0, 0), noise_std: float = 0.0, noise_seed: int = 0, gamma: float = 1.0,
                value_range=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the intensity stage on one (H', W', D') fp32 device tensor: blur, then noise, then gamma (include/ctseg_hip.h,
    ``ctseg_intensity3d``, has the rules).  ``sigma`` = the Gaussian's sigma in voxels per axis d, h, w: 0 skips an axis, otherwise
    0 < sigma <= 4; ``noise_std`` > 0 adds ``noise_std * n(noise_seed, voxel index)``, a stateless standard normal field;
    ``value_range`` = (lo, hi) switches the gamma step on: the value is clamped to the range and sent through
    ``lo + (hi - lo) * t ** gamma`` (``gamma`` = 1: the clamp alone).  ``out`` = None (a new tensor), ``image`` itself (in place)
    or another tensor of its shape.  One launch per blurred axis with the rest folded into the last of them; no scratch volume.
    Bad parameters raise ``ValueError``, a CPU tensor ``NativeError``"""
    sigma, noise_std, noise_seed, gamma, value_range = _check_intensity(sigma, noise_std, noise_seed, gamma, value_range)
    if out is None:
        out = torch.empty_like(image, memory_format=torch.contiguous_format)
    for t, what in ((image, "image"), (out, "out")):
        if t.dim() != 3 or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != image.shape or t.device != image.device:
            raise ValueError(f"intensity3d: {what} is a contiguous float32 (H', W', D') tensor; image and out agree in shape and device")
    nat.require_gpu(image, "intensity3d")
    radius, taps = (ctypes.c_int32 * 3)(), (ctypes.c_float * (3 * (_MAX_RADIUS + 1)))()
    for a, s in enumerate(sigma):
        if s > 0.0:
            radius[a], w = gaussian_taps(s)
            taps[a * (_MAX_RADIUS + 1):a * (_MAX_RADIUS + 1) + len(w)] = w.tolist()
    Ho, Wo, Do = image.shape
    lo, hi = value_range if value_range is not None else (0.0, 0.0)
    nat.call("ctseg_intensity3d", nat.ptr(image), nat.ptr(out), Do, Ho, Wo, ctypes.addressof(radius), ctypes.addressof(taps), noise_std,
             noise_seed, int(value_range is not None), lo, hi, gamma)
    return out


def _axis_ranges(v, what, who="Augment3D"):
    """(lo, hi) for all three axes, or ((lo, hi), (lo, hi), (lo, hi)) per axis d, h, w -> (3, 2) float64"""
    a = np.asarray(v, dtype=np.float64)
    if a.shape == (2,):
        a = np.tile(a, (3, 1))
    if a.shape != (3, 2) or (a[:, 0] > a[:, 1]).any():
        raise ValueError(f"{who}: {what} is (lo, hi) or one (lo, hi) per axis, lo <= hi")
    return a


class Deform3D:
    """Random free-form deformation for ``Augment3D(deform=...)``: a cubic B-spline over a lattice of ``cells`` = cells per axis
    d, h, w of the output grid, whose control points move by up to ``magnitude`` output voxels per axis (uniform, from a drawn
    seed, on the device); ``p`` = probability that an augmented instance is deformed.  ``check(size)`` raises ``ValueError`` for a
    grid on which a cell has under 4 voxels or a magnitude exceeds 0.4 of a cell, the bound below which the map cannot fold."""

    def __init__(self, cells=(3, 8, 8), magnitude=(1.0, 4.0, 4.0), p: float = 1.0):
        self.cells = tuple(int(v) for v in cells)
        self.magnitude = tuple(float(v) for v in magnitude)
        if len(self.cells) != 3 or len(self.magnitude) != 3 or min(self.cells) < 1:
            raise ValueError("Deform3D: cells and magnitude have one entry per axis d, h, w; at least one cell per axis")
        if not all(np.isfinite(m) and m >= 0.0 for m in self.magnitude):
            raise ValueError("Deform3D: magnitudes are finite and not negative")
        self.p = float(p)

    def check(self, size):
        _check_deform(self.cells, self.magnitude, tuple(int(v) for v in size))


class Intensity3D:
    """Random blur, noise and gamma for ``Augment3D(intensity=...)``, run by ``intensity3d`` on the resampled image.  Each of the
    three is chosen on its own: ``blur_sigma`` = (lo, hi) of the Gaussian's sigma in output voxels, or one pair per axis d, h, w
    (one uniform places all three axes inside their ranges), with probability ``blur_p``; ``noise_std`` = (lo, hi) of the standard
    deviation of the added Gaussian noise, with probability ``noise_p``; ``gamma`` = (lo, hi) of the exponent, drawn log-uniformly,
    exp(ln lo + (ln hi - ln lo) u), with probability ``gamma_p``, over ``value_range`` = (lo, hi) of the windowed image, to which
    the gamma step also clamps.  None switches a component off.  The limits of ``ctseg_intensity3d`` are checked here: sigma in
    [0, 4], std >= 0, gamma in [0.25, 4] and only with a ``value_range``."""

    def __init__(self, value_range=None, blur_sigma=None, blur_p: float = 0.2, noise_std=None, noise_p: float = 0.15, gamma=None,
                 gamma_p: float = 0.3):
        who = "Intensity3D"
        self.value_range = _check_range(value_range, who)
        self.blur_sigma = None if blur_sigma is None else _axis_ranges(blur_sigma, "blur_sigma", who)
        if self.blur_sigma is not None and not (np.isfinite(self.blur_sigma).all() and self.blur_sigma.min() >= 0.0
                                                and self.blur_sigma.max() <= _MAX_SIGMA):
            raise ValueError(f"{who}: blur_sigma lies in [0, {_MAX_SIGMA}]")
        self.noise_std = None if noise_std is None else tuple(float(v) for v in noise_std)
        if self.noise_std is not None and not (len(self.noise_std) == 2 and np.isfinite(self.noise_std).all()
                                               and 0.0 <= self.noise_std[0] <= self.noise_std[1]):
            raise ValueError(f"{who}: noise_std is (lo, hi), finite, 0 <= lo <= hi")
        self.gamma = None if gamma is None else tuple(float(v) for v in gamma)
        if self.gamma is not None:
            if not (len(self.gamma) == 2 and 0.25 <= self.gamma[0] <= self.gamma[1] <= 4.0):
                raise ValueError(f"{who}: gamma is (lo, hi) with 0.25 <= lo <= hi <= 4")
            if self.value_range is None:
                raise ValueError(f"{who}: gamma needs a value_range (lo, hi)")
        self.blur_p, self.noise_p, self.gamma_p = float(blur_p), float(noise_p), float(gamma_p)

    def params(self, applied: bool, blur_chance, sigma_u, noise_chance, std_u, noise_seed, gamma_chance, gamma_u):
        """the seven drawn values -> None (not applied, or no component chosen) or the keyword arguments of ``intensity3d``"""
        blur = applied and self.blur_sigma is not None and blur_chance < self.blur_p
        noise = applied and self.noise_std is not None and noise_chance < self.noise_p
        curve = applied and self.gamma is not None and gamma_chance < self.gamma_p
        if not (blur or noise or curve):
            return None
        sigma = (0.0, 0.0, 0.0)
        if blur:
            sigma = tuple((self.blur_sigma[:, 0] + (self.blur_sigma[:, 1] - self.blur_sigma[:, 0]) * sigma_u).tolist())
        std = self.noise_std[0] + (self.noise_std[1] - self.noise_std[0]) * std_u if noise else 0.0
        g = float(np.exp(np.log(self.gamma[0]) + (np.log(self.gamma[1]) - np.log(self.gamma[0])) * gamma_u)) if curve else 1.0
        return {"sigma": sigma, "noise_std": float(std), "noise_seed": int(noise_seed), "gamma": g,
                "value_range": self.value_range if curve else None}


class Augment3D:
    """Random affine + mirror + intensity augmentation of a volume, applied by ``InstancePipeline3D(augment=...)`` in its one pass.

    All axes are ordered d, h, w: the reference's (D, H, W) arrays, W being the patient's left-right axis.
    ``rotate`` = half-ranges in radians of the angles about the d, h and w axes (the turn about d is the in-plane one), about the
    centre of the output grid; ``scale`` = (lo, hi) of the zoom factors, drawn per axis, or one (lo, hi) per axis (a factor above
    1 magnifies); ``translate`` = half-ranges in output voxels; ``flip_prob`` = probability of a mirror per axis;
    ``swap_pairs`` = mask channels that trade places under a w mirror (default: OpticNerve, Parotid, Submandibular L/R of
    ``STRUCTURES``); ``gain`` / ``bias`` = (lo, hi) of ``v * gain + bias`` after the window, or None; ``interp`` "trilinear" or
    "nearest" for the image (masks are always nearest); ``border`` "constant" (``cval`` / 0) or "edge"; ``p`` = probability that
    anything is applied at all; ``deform`` = a ``Deform3D`` or None: a non-rigid displacement added to the affine sampling point;
    ``intensity`` = an ``Intensity3D`` or None: blur, noise and gamma on the resampled image, a second stage after the pass.

    The matrix maps an output voxel o to the point q = L o + offset it samples (the sampling direction), composed in float64 as
        L = R_w(angle_w) . R_h(angle_h) . R_d(angle_d) . diag(1 / scale) . F,      offset = c - L c + shift,   c = (size - 1) / 2
    so, read from the right: the output voxel is mirrored (F = diag of +-1, exact integers), divided by the zoom, then turned
    about d, about h and about w; the shift comes last.  With axes ordered (d, h, w) and (c, s) = (cos, sin) of the angle,
        R_d = [[1, 0, 0], [0, c, -s], [0, s, c]],   R_h = [[c, 0, s], [0, 1, 0], [-s, 0, c]],   R_w = [[c, -s, 0], [s, c, 0], [0, 0, 1]].
    The result is rounded to float32 once."""

    def __init__(self, rotate=(0.0, 0.0, 0.0), scale=(1.0, 1.0), translate=(0.0, 0.0, 0.0), flip_prob=(0.0, 0.0, 0.0),
                 swap_pairs=((3, 4), (5, 6), (7, 8)), gain=None, bias=None, interp="trilinear", border="constant", cval: float = 0.0,
                 p: float = 1.0, deform: Optional[Deform3D] = None, intensity: Optional[Intensity3D] = None):
        self.rotate = np.abs(np.asarray(rotate, dtype=np.float64).reshape(3))
        self.scale = _axis_ranges(scale, "scale")
        if (self.scale <= 0).any():
            raise ValueError("Augment3D: scale factors are positive")
        self.translate = np.abs(np.asarray(translate, dtype=np.float64).reshape(3))
        self.flip_prob = np.asarray(flip_prob, dtype=np.float64).reshape(3)
        self.swap_pairs = tuple((int(a), int(b)) for a, b in swap_pairs)
        self.gain = None if gain is None else tuple(float(v) for v in gain)
        self.bias = None if bias is None else tuple(float(v) for v in bias)
        if interp not in _INTERPS or border not in _BORDERS:
            raise ValueError(f"Augment3D: interp is one of {sorted(_INTERPS)}, border one of {sorted(_BORDERS)}")
        self.interp, self.border, self.cval, self.p = interp, border, float(cval), float(p)
        self.deform, self.intensity = deform, intensity
        self._rng = np.random.default_rng()

    @staticmethod
    def identity_params() -> dict:
        return {"applied": False, "angles": (0.0, 0.0, 0.0), "scales": (1.0, 1.0, 1.0), "shifts": (0.0, 0.0, 0.0),
                "flips": (False, False, False), "gain": 1.0, "bias": 0.0}

    def draw(self, generator=None) -> dict:
        """one instance's parameters, uniform in the ranges, from a ``numpy.random.Generator``; the draws are made in one fixed
        order and number whatever the ranges are (applied, angles, scales, shifts, flips, gain, bias): 15 uniforms per call.
        With a ``deform``, two more values follow them in every call, a uniform (deformed or not) and the lattice's seed, and
        the dict gains ``"deform"``: None or {"seed", "cells", "magnitude"}.  With an ``intensity``, seven more values follow
        those in every call (blur chance, sigma uniform, noise chance, std uniform, noise seed, gamma chance, gamma uniform) and
        the dict gains ``"intensity"``: None or {"sigma", "noise_std", "noise_seed", "gamma", "value_range"}"""
        g = generator if generator is not None else self._rng
        u = g.random(15)
        params = self._affine_params(u)
        if self.deform is not None:
            chance, seed = g.random(), int(g.integers(0, 2 ** 63))
            on = params["applied"] and chance < self.deform.p
            params["deform"] = {"seed": seed, "cells": self.deform.cells, "magnitude": self.deform.magnitude} if on else None
        if self.intensity is not None:
            blur_chance, sigma_u, noise_chance, std_u = g.random(), g.random(), g.random(), g.random()
            seed = int(g.integers(0, 2 ** 63))
            gamma_chance, gamma_u = g.random(), g.random()
            params["intensity"] = self.intensity.params(params["applied"], blur_chance, sigma_u, noise_chance, std_u, seed,
                                                        gamma_chance, gamma_u)
        return params

    def _affine_params(self, u) -> dict:
        if not u[0] < self.p:
            return self.identity_params()
        sym = 2.0 * u[1:10] - 1.0
        lo, hi = self.scale[:, 0], self.scale[:, 1]
        gain = 1.0 if self.gain is None else self.gain[0] + (self.gain[1] - self.gain[0]) * u[13]
        bias = 0.0 if self.bias is None else self.bias[0] + (self.bias[1] - self.bias[0]) * u[14]
        return {"applied": True, "angles": tuple((sym[0:3] * self.rotate).tolist()),
                "scales": tuple((lo + (hi - lo) * u[4:7]).tolist()), "shifts": tuple((sym[6:9] * self.translate).tolist()),
                "flips": tuple(bool(v) for v in u[10:13] < self.flip_prob), "gain": float(gain), "bias": float(bias)}

    @staticmethod
    def matrix(size, params, dtype=np.float32) -> np.ndarray:
        """(3, 4) float32 sampling matrix of ``params`` on the ``size`` = (D', H', W') grid: the class docstring has the order;
        ``dtype=np.float64`` hands out the composition before its one rounding (``tta.view_to_target_matrix`` inverts that)"""
        c = (np.asarray(size, dtype=np.float64).reshape(3) - 1.0) / 2.0
        ad, ah, aw = (float(v) for v in params["angles"])
        cd, sd, ch, sh, cw, sw = np.cos(ad), np.sin(ad), np.cos(ah), np.sin(ah), np.cos(aw), np.sin(aw)
        Rd = np.array([[1, 0, 0], [0, cd, -sd], [0, sd, cd]], dtype=np.float64)
        Rh = np.array([[ch, 0, sh], [0, 1, 0], [-sh, 0, ch]], dtype=np.float64)
        Rw = np.array([[cw, -sw, 0], [sw, cw, 0], [0, 0, 1]], dtype=np.float64)
        S = np.diag(1.0 / np.asarray(params["scales"], dtype=np.float64).reshape(3))
        F = np.diag([-1.0 if f else 1.0 for f in params["flips"]])
        L = Rw @ Rh @ Rd @ S @ F
        out = np.empty((3, 4), dtype=np.float64)
        out[:, :3] = L
        out[:, 3] = c - L @ c + np.asarray(params["shifts"], dtype=np.float64).reshape(3)
        return out.astype(dtype)

    def channel_src(self, params, K: int) -> list:
        """output mask channel k reads input channel ``channel_src[k]``: the identity, or ``swap_pairs`` swapped when the w mirror
        (the patient's left-right) was drawn; ``mask_indicator`` takes the same permutation"""
        src = list(range(K))
        if params["flips"][2]:
            for a, b in self.swap_pairs:
                if a < K and b < K:
                    src[a], src[b] = b, a
        return src


class Resize3D:
    def __init__(self, size=(96, 256, 256), always_apply=True, p=1.0):
        self.size = tuple(size)      # DxHxW, as the reference

    def apply(self, image: torch.Tensor, **params) -> torch.Tensor:
        """(1,D,H,W) -> (1,D',H',W') (values of F.interpolate(image[None], size)[0]; storage is (H',W',D')-contiguous)"""
        out = resize3d_to_hwd(image, None, self.size)[0]
        return out.permute(2, 0, 1).unsqueeze(0)

    def apply_to_mask(self, image: torch.Tensor, **params) -> torch.Tensor:
        """(D,H,W) -> (D',H',W')"""
        out = resize3d_to_hwd(None, image.unsqueeze(0), self.size)[1]
        return out[0].permute(2, 0, 1)

    def get_transform_init_args_names(self):
        return []


class ToTensorV3:
    def __init__(self, always_apply=True, p=1.0):
        pass

    def apply(self, img, **params):
        return img.permute(0, 2, 3, 1)

    def apply_to_mask(self, mask, **params):
        return mask.permute(1, 2, 0)

    def get_transform_init_args_names(self):
        return ("transpose_mask",)


class InstancePipeline3D:
    """``transform(image=..., masks=...) -> {"image": (1,H,W,D) fp32, "masks": ...}`` like the albumentations Compose of
    volumetric/predefined.py:4-7.  ``squash=False``: "masks" = (9,H,W,D) uint8 (the reference's batch element);
    ``squash=True``: "masks" = (H,W,D) uint8 label map with ``"hist"`` = per-class voxel counts riding along.
    ``dist_maps=True`` adds ``"dist_maps"``: the (9,H,W,D) fp32 distance maps of the nine RESIZED masks
    (``data.utils.compute_distance_map(spatial_dims=3)``, ``signed`` as there).  Structures overlap, so the label map cannot give
    them back: a squashing pipeline then has the same resize launch write the nine masks beside the label map.
    ``augment`` = an ``Augment3D``: the one launch is ``ctseg_augment3d_to_hwd`` instead, with parameters drawn from ``generator``
    (a ``numpy.random.Generator``) or given as ``params`` (``Augment3D.draw``'s dict); the result then carries ``"params"`` and
    ``"channel_src"``, the K input channels behind the output mask channels, which ``mask_indicator`` has to follow.  The
    distance maps are those of the augmented masks.  An ``Augment3D`` with a ``deform`` is checked against ``size`` here, and an
    instance whose ``params["deform"]`` is set takes the lattice launch and the deformed pass instead.  An instance whose
    ``params["intensity"]`` is set sends the image, and nothing else, through ``intensity3d`` after the pass, in place."""

    def __init__(self, size=(96, 256, 256), squash: bool = False, window: Optional[Tuple] = None, dist_maps: bool = False,
                 signed: bool = False, augment: Optional[Augment3D] = None):
        self.size, self.squash, self.window, self.dist_maps, self.signed = tuple(size), squash, window, dist_maps, signed
        self.augment = augment
        if augment is not None and augment.deform is not None:
            augment.deform.check(self.size)

    def __call__(self, image: torch.Tensor, masks, params=None, generator=None) -> dict:
        if isinstance(masks, (list, tuple)):
            masks = torch.stack(list(masks))
        want_masks = self.dist_maps or not self.squash
        extra = {}
        if self.augment is None:
            img, m, lab, hist = resize3d_to_hwd(image, masks, self.size, self.window, want_masks=want_masks, want_labels=self.squash)
        else:
            aug = self.augment
            if params is None:
                params = aug.draw(generator)
            src = aug.channel_src(params, masks.reshape((-1,) + tuple(masks.shape[-3:])).shape[0])
            img, m, lab, hist = augment3d_to_hwd(image, masks, self.size, aug.matrix(self.size, params), aug.interp, aug.border,
                                                 aug.cval, src, self.window, params["gain"], params["bias"], want_masks=want_masks,
                                                 want_labels=self.squash, deform=params.get("deform"))
            if params.get("intensity") is not None and img is not None:
                intensity3d(img, **params["intensity"], out=img)
            extra = {"channel_src": src, "params": params}
        out = {"image": img.unsqueeze(0), "masks": lab if self.squash else m, **extra}
        if self.squash:
            out["hist"] = hist
        if self.dist_maps:
            out["dist_maps"] = compute_distance_map(m, signed=self.signed, spatial_dims=3)
        return out


class PatchSampler3D:
    """Foreground-biased patches of a raw volume at its own resolution (MONAI's ``RandCropByPosNegLabel``, nnU-Net's foreground
    oversampling), which the reference's 3-D path lacks: ``num_patches`` patches of ``patch`` = (D', H', W') voxels (the order of
    ``InstancePipeline3D.size``), each with probability ``fg_prob`` centred on a voxel of a structure drawn with equal chance per
    class among those of ``class_mask`` (bit k = mask k; default all) that the volume has, otherwise on a uniform voxel.  The
    device picks the centres (``patch_centres``) and every patch is one ``patch3d_to_hwd`` launch reading its centre there: nothing
    in the call reads device memory back.  ``squash`` / ``window`` as ``InstancePipeline3D``.
    ``augment`` = an ``Augment3D`` that contributes rotation, zoom, mirrors and gain / bias about the patch centre (its matrix on
    the patch grid, composed in float64, moved by ``patch // 2`` and rounded once: ``patch_matrix``), its ``interp`` / ``border`` /
    ``cval``, and its ``intensity`` stage after the pass; ``translate`` (the centre is the translation) and ``deform`` raise
    ``ValueError``.  Without one the matrix is the identity with translation ``-(patch // 2)``: an exact crop.

    ``draw`` takes, per patch and in this order, a fixed number of values from the ``numpy.random.Generator``: one uniform (the fg
    chance), two integers in [0, 2^32) (``a``: the class, ``b``: the rank), then ``Augment3D.draw``'s own values when there is
    an ``augment`` (15 uniforms, 7 more values with an ``intensity``).  A seed therefore reproduces an epoch."""

    def __init__(self, patch, num_patches: int = 2, fg_prob: float = 2 / 3, class_mask: Optional[int] = None, squash: bool = False,
                 window: Optional[Tuple] = None, augment: Optional[Augment3D] = None):
        self.patch = tuple(int(v) for v in patch)
        self.num_patches, self.fg_prob, self.class_mask = int(num_patches), float(fg_prob), class_mask
        if len(self.patch) != 3 or min(self.patch) < 1:
            raise ValueError("PatchSampler3D: patch is (D', H', W'), every side at least 1")
        if not 1 <= self.num_patches <= _MAX_PATCHES:
            raise ValueError(f"PatchSampler3D: num_patches lies in [1, {_MAX_PATCHES}]")
        if not 0.0 <= self.fg_prob <= 1.0:
            raise ValueError("PatchSampler3D: fg_prob is a probability")
        if augment is not None and (augment.translate != 0).any():
            raise ValueError("PatchSampler3D: augment.translate must be 0 (the patch centre is the translation)")
        if augment is not None and augment.deform is not None:
            raise ValueError("PatchSampler3D: an augment with a deform is not supported on patches")
        self.squash, self.window, self.augment = squash, window, augment
        self._rng = np.random.default_rng()

    def draw(self, generator=None) -> list:
        """one volume's draws: ``num_patches`` tuples (fg, a, b, params), ``params`` = ``Augment3D.draw``'s dict or None"""
        g = generator if generator is not None else self._rng
        out = []
        for _ in range(self.num_patches):
            chance, a, b = g.random(), int(g.integers(0, 2 ** 32)), int(g.integers(0, 2 ** 32))
            out.append((chance < self.fg_prob, a, b, self.augment.draw(g) if self.augment is not None else None))
        return out

    def matrix(self, params=None) -> np.ndarray:
        """the (3, 4) float32 matrix of one patch: see ``patch_matrix``"""
        return patch_matrix(self.patch, None if params is None else Augment3D.matrix(self.patch, params, np.float64))

    def __call__(self, image: torch.Tensor, masks, generator=None, draws=None) -> dict:
        """image (1,D,H,W) or (D,H,W), masks (K,D,H,W) on the device; ``draws`` = ``draw``'s list (rows (fg, a, b) alone mean no
        augmentation), drawn from ``generator`` when None -> {"image": (P,1,h,w,d) fp32, "masks": (P,K,h,w,d) uint8 or, squashing,
        the (P,h,w,d) label maps with "hist": (P,K+1), "centres": the (P,4) int32 device table, "channel_src": one list per
        patch, "draws"}"""
        if isinstance(masks, (list, tuple)):
            masks = torch.stack(list(masks))
        masks = masks.reshape((-1,) + tuple(masks.shape[-3:]))
        if masks.dtype != torch.uint8:
            masks = masks.to(torch.uint8)
        masks = masks.contiguous()
        if draws is None:
            draws = self.draw(generator)
        draws = [tuple(d) + (None,) * (4 - len(d)) for d in draws]
        P, K, dev = len(draws), masks.shape[0], masks.device
        Do, Ho, Wo = self.patch
        centres = patch_centres(masks, [d[:3] for d in draws], self.patch, self.class_mask)
        img = torch.empty((P, 1, Ho, Wo, Do), dtype=torch.float32, device=dev)
        m = lab = hist = None
        if self.squash:
            lab = torch.empty((P, Ho, Wo, Do), dtype=torch.uint8, device=dev)
            hist = torch.zeros((P, K + 1), dtype=torch.int64, device=dev)
        else:
            m = torch.empty((P, K, Ho, Wo, Do), dtype=torch.uint8, device=dev)
        aug, srcs = self.augment, []
        for i, (_, _, _, params) in enumerate(draws):
            src = aug.channel_src(params, K) if aug is not None and params is not None else list(range(K))
            srcs.append(src)
            outs = (img[i, 0], None if m is None else m[i], None if lab is None else lab[i], None if hist is None else hist[i])
            if aug is None or params is None:
                patch3d_to_hwd(image, masks, self.patch, self.matrix(), centres[i], 0, window=self.window, outs=outs)
                continue
            patch3d_to_hwd(image, masks, self.patch, self.matrix(params), centres[i], aug.interp, aug.border, aug.cval, src,
                           self.window, params["gain"], params["bias"], outs=outs)
            if params.get("intensity") is not None:
                intensity3d(img[i, 0], **params["intensity"], out=img[i, 0])
        out = {"image": img, "masks": lab if self.squash else m, "centres": centres, "channel_src": srcs, "draws": draws}
        if self.squash:
            out["hist"] = hist
        return out


windowed_degree_0 = {"train": InstancePipeline3D(), "test": InstancePipeline3D()}      # volumetric/predefined.py:4-7
# the reference has no augmenting 3-D preset.  Up to 15 degrees in plane and 3 degrees out of it, +-10 % zoom, a few voxels of shift
# and the left-right mirror; no intensity jitter: the 3-D path has no window, so the image scale is raw and unknown here
augmented_degree_1 = {
    "train": InstancePipeline3D(augment=Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), translate=(2, 8, 8),
                                                  flip_prob=(0, 0, 0.5))),
    "test": InstancePipeline3D(),
}
# degree 1 plus a free-form deformation of every other augmented instance: 3 x 8 x 8 cells of 32 voxels over the 96 x 256 x 256 grid,
# control points moved by up to 1 voxel through the slices and 4 in plane (0.03 and 0.125 of a cell: far below the folding bound)
augmented_degree_2 = {
    "train": InstancePipeline3D(augment=Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), translate=(2, 8, 8),
                                                  flip_prob=(0, 0, 0.5),
                                                  deform=Deform3D(cells=(3, 8, 8), magnitude=(1.0, 4.0, 4.0), p=0.5))),
    "test": InstancePipeline3D(),
}
# degree 2 on the soft-tissue window, shifted to (0, 1), which gives the image the known scale an intensity stage needs: what differs
# between scanners and reconstruction kernels is sharpness (a blur of up to half a voxel through the slices and 0.5 to 1 in plane),
# noise (up to 5 % of the window) and the contrast curve (gamma between 0.7 and 1 / 0.7).  The "test" side takes the same window
_SOFT_TISSUE = (*WINDOWING_CONFIG["soft_tissue"], True)
augmented_degree_3 = {
    "train": InstancePipeline3D(window=_SOFT_TISSUE,
                                augment=Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), translate=(2, 8, 8), flip_prob=(0, 0, 0.5),
                                                  deform=Deform3D(cells=(3, 8, 8), magnitude=(1.0, 4.0, 4.0), p=0.5),
                                                  intensity=Intensity3D(value_range=(0, 1), blur_sigma=((0, 0.5), (0.5, 1.0), (0.5, 1.0)),
                                                                        noise_std=(0, 0.05), gamma=(0.7, 1 / 0.7)))),
    "test": InstancePipeline3D(window=_SOFT_TISSUE),
}
