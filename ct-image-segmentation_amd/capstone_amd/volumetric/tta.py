"""Test-time augmentation and native-grid prediction for the 3-D U-Net (not in the reference, whose 3-D path stops at the logits).

A VIEW is the scan as ``augment3d_to_hwd`` shows it under one set of ``Augment3D`` parameters: mirrored, turned, zoomed.  The
network predicts every view; ``ctseg_tta_accumulate`` carries each prediction back onto one TARGET grid, the model's ``(H', W',
D')`` grid or the raw scan's own ``(D, H, W)`` array, and adds it into an accumulator there, and ``ctseg_tta_finish`` turns the
accumulator into a label map (include/ctseg_hip.h has the rules of both).  The merge is one gather, one softmax and one
read-modify-write per voxel and view, in one HIP pass; there are no atomics, so the same views in the same order give the same bits.

The left-right mirror (w) swaps the paired structures: a mirrored view's "left parotid" channel holds the patient's right parotid.
``class_channel_src`` is the map that undoes it (background stays, the nine structures follow ``Augment3D.channel_src``); a plain
``torch.flip`` ensemble averages the pairs into each other.

Memory: the accumulator has ``acc_ld`` = C + 1 rounded up to a multiple of 4 floats per TARGET voxel, ``4 * acc_ld`` bytes: 48 bytes
for the 10 classes, 0.30 GB on the (96, 256, 256) model grid and 1.76 GB on a native 140 x 512 x 512 scan.  ``TestTimeAugmenter3D``
keeps one and reuses it across calls of the same shape.  There is no CPU fallback: CPU tensors raise ``NativeError``.
"""
import ctypes
import itertools
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _native as nat
from ..models.losses import _as_cl
from .transforms import _INTERPS, Augment3D, _c_matrix, _c_permutation, augment3d_to_hwd

_MODES = {"logits": 0, "probabilities": 1}
_LAYOUTS = {"hwd": 0, "dhw": 1}
_AXES = {"d": 0, "h": 1, "w": 2}


def acc_width(C: int) -> int:
    """floats per accumulator row: the C classes and the weight sum, rounded up to whole 16-byte chunks"""
    return (int(C) + 1 + 3) // 4 * 4


def tta_accumulate(acc: torch.Tensor, logits: torch.Tensor, matrix, chan_src=None, weight: float = 1.0, mode="probabilities",
                   interp="trilinear", target: Optional[Sequence[int]] = None, layout="hwd") -> torch.Tensor:
    """adds one view's prediction into ``acc`` (``ctseg_tta_accumulate``).  ``logits`` (1, C, H, W, D) fp32, the network's output
    for the view (channels-last storage is read in place); ``matrix`` (3, 4), rows and columns ordered d, h, w, maps a voxel of the
    ``target`` = (Dt, Ht, Wt) grid (default: the view's own) to the point of the view it samples; accumulator column k takes view
    channel ``chan_src[k]``; ``mode`` "probabilities" or "logits"; ``interp`` "trilinear" or "nearest"; ``layout`` "hwd" (rows in
    the model's order) or "dhw" (the raw scan's).  ``acc``: fp32, Dt * Ht * Wt rows of ``acc.shape[-1]`` floats, zeroed by the
    caller before the first view."""
    nat.require_gpu(logits, "tta_accumulate")
    nat.require_gpu(acc, "tta_accumulate")
    if logits.dim() != 5 or logits.shape[0] != 1:
        raise nat.NativeError(f"tta_accumulate: logits are (1, C, H, W, D), one sample per call; got {tuple(logits.shape)}")
    C, H, W, D = (int(v) for v in logits.shape[1:])
    Dt, Ht, Wt = (D, H, W) if target is None else (int(v) for v in target)
    acc_ld = int(acc.shape[-1])
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() != Dt * Ht * Wt * acc_ld:
        raise nat.NativeError(f"tta_accumulate: acc is a contiguous fp32 tensor of {Dt * Ht * Wt} rows of {acc_ld}; got "
                              f"{acc.dtype} {tuple(acc.shape)}")
    ptr, ld, _keep = _as_cl(logits if logits.dtype == torch.float32 else logits.float())
    mat = _c_matrix(matrix)
    src = _c_permutation(chan_src, C, "tta_accumulate: chan_src", "channels")
    nat.call("ctseg_tta_accumulate", ptr, ld, C, D, H, W, ctypes.addressof(mat), ctypes.addressof(src) if src is not None else None,
             float(weight), _MODES.get(mode, mode), _INTERPS.get(interp, interp), Dt, Ht, Wt, _LAYOUTS.get(layout, layout),
             nat.ptr(acc), acc_ld)
    return acc


def tta_finish(acc: torch.Tensor, C: int, mode="probabilities", want_probs: bool = False):
    """the accumulator -> (labels (St,) uint8, probs (St, C) fp32 or None, hist (C,) int64), ``ctseg_tta_finish``: the first maximal
    class per voxel, 0 where no view reached; ``mode`` as it was accumulated"""
    nat.require_gpu(acc, "tta_finish")
    acc_ld = int(acc.shape[-1])
    St = acc.numel() // acc_ld
    labels = torch.empty(St, dtype=torch.uint8, device=acc.device)
    probs = torch.empty((St, C), dtype=torch.float32, device=acc.device) if want_probs else None
    hist = torch.zeros(C, dtype=torch.int64, device=acc.device)
    nat.call("ctseg_tta_finish", nat.ptr(acc), acc_ld, int(C), St, _MODES.get(mode, mode), nat.ptr(labels), nat.ptr(probs), nat.ptr(hist))
    return labels, probs, hist


def view_to_target_matrix(size, params, native_shape=None, dtype=np.float32) -> np.ndarray:
    """(3, 4) matrix that sends a TARGET voxel to the point of the view's grid that shows it, for the view ``params`` on the
    ``size`` = (D', H', W') grid.  The view samples q = A o + b (``Augment3D.matrix``), so a voxel r of the plain resized volume is
    seen at o = A^-1 r - A^-1 b; a voxel n of the raw scan of ``native_shape`` sits at r = S n, S = diag(size / native), the
    pull-back of the resize's index rule floor(r * native / size).  Composed in float64 and rounded to ``dtype`` once."""
    Ab = Augment3D.matrix(size, params, dtype=np.float64)
    inv = np.linalg.inv(Ab[:, :3])
    S = np.eye(3)
    if native_shape is not None:
        S = np.diag(np.asarray(size, dtype=np.float64).reshape(3) / np.asarray(native_shape, dtype=np.float64).reshape(3))
    out = np.empty((3, 4), dtype=np.float64)
    out[:, :3] = inv @ S
    out[:, 3] = -inv @ Ab[:, 3]
    return out.astype(dtype)


def class_channel_src(params, augment: Optional[Augment3D] = None, n_structures: int = 9) -> list:
    """accumulator class k takes view channel ``src[k]``: background stays, the structures follow the view's mask permutation"""
    augment = augment if augment is not None else Augment3D()
    return [0] + [1 + s for s in augment.channel_src(params, n_structures)]


def mirror_views(axes=("w",)) -> list:
    """the parameter dicts of the mirror group over ``axes`` (of "d", "h", "w"), the identity first: 2 ** len(axes) views, the
    first axis given toggling slowest"""
    idx = [_AXES[a] for a in axes]
    views = []
    for bits in itertools.product((False, True), repeat=len(idx)):
        flips = [False, False, False]
        for i, b in zip(idx, bits):
            flips[i] = b
        views.append(dict(Augment3D.identity_params(), applied=any(bits), flips=tuple(flips)))
    return views


class TestTimeAugmenter3D:
    """``views``: ``Augment3D`` parameter dicts (``mirror_views()``, ``Augment3D.draw``), one network pass each; ``size``: the
    model's grid (D', H', W'); ``mode`` "probabilities" (mean of softmaxes) or "logits"; ``interp`` of the merge, "trilinear" or
    "nearest"; ``weights``: one positive weight per view (default 1); ``window``: the HU window of ``InstancePipeline3D``, applied
    to raw scans by ``predict``; ``augment``: the ``Augment3D`` whose ``swap_pairs``, image ``interp``, ``border`` and ``cval``
    build the views (default: ``Augment3D()``).  The accumulator (``4 * acc_ld`` bytes per target voxel, see the module docstring)
    is kept and reused across calls of the same shape."""
    __test__ = False      # (not a test class, whatever its name starts with)

    def __init__(self, views, size=(96, 256, 256), mode="probabilities", interp="trilinear", weights=None, window=None,
                 augment: Optional[Augment3D] = None):
        self.views = [dict(v) for v in views]
        if not self.views:
            raise ValueError("TestTimeAugmenter3D: at least one view")
        if any(v.get("deform") is not None for v in self.views):
            raise ValueError("TestTimeAugmenter3D: a deformed view (params['deform'] is set) has no inverse matrix to merge its "
                             "prediction through; draw the views from an Augment3D without deform")
        if any(v.get("intensity") is not None for v in self.views):
            raise ValueError("TestTimeAugmenter3D: a view with an intensity stage (params['intensity'] is set: blur, noise, gamma) "
                             "is no view of the same scan; draw the views from an Augment3D without intensity")
        self.size = tuple(int(v) for v in size)
        if mode not in _MODES or interp not in _INTERPS:
            raise ValueError(f"TestTimeAugmenter3D: mode is one of {sorted(_MODES)}, interp one of {sorted(_INTERPS)}")
        self.mode, self.interp, self.window = mode, interp, window
        self.weights = [1.0] * len(self.views) if weights is None else [float(w) for w in weights]
        if len(self.weights) != len(self.views) or not all(np.isfinite(w) and w > 0 for w in self.weights):
            raise ValueError("TestTimeAugmenter3D: one finite positive weight per view")
        self.augment = augment if augment is not None else Augment3D()
        self._acc = None

    def _accumulator(self, rows, C, device):
        acc = self._acc
        if acc is None or acc.shape != (rows, acc_width(C)) or acc.device != device:
            self._acc = acc = torch.empty((rows, acc_width(C)), dtype=torch.float32, device=device)
        return acc.zero_()

    def _predict(self, model, image, native, want_probs, window):
        nat.require_gpu(image, "TestTimeAugmenter3D")
        if image.dim() != 3:
            raise nat.NativeError(f"TestTimeAugmenter3D: a (D, H, W) scan; got {tuple(image.shape)}")
        aug, size = self.augment, self.size
        shape = tuple(int(v) for v in image.shape)
        target, layout = (shape, "dhw") if native else (size, "hwd")
        rows = target[0] * target[1] * target[2]
        acc = C = None
        with torch.no_grad():
            for params, weight in zip(self.views, self.weights):
                x = augment3d_to_hwd(image, None, size, Augment3D.matrix(size, params), aug.interp, aug.border, aug.cval, None, window,
                                     params.get("gain", 1.0), params.get("bias", 0.0))[0]
                logits = model(x[None, None])
                if acc is None:
                    C = int(logits.shape[1])
                    acc = self._accumulator(rows, C, image.device)
                tta_accumulate(acc, logits, view_to_target_matrix(size, params, shape if native else None),
                               class_channel_src(params, aug, C - 1), weight, self.mode, self.interp, target, layout)
            labels, probs, hist = tta_finish(acc, C, self.mode, want_probs)
            uncovered = (acc[:, C] == 0).sum()
        grid = shape if native else (size[1], size[2], size[0])
        return SimpleNamespace(labels=labels.view(grid), uncovered=uncovered, hist=hist,
                               probs=probs.view(grid + (C,)) if want_probs else None)

    def predict(self, model, image: torch.Tensor, native: bool = False, want_probs: bool = False):
        """``image``: a raw (D, H, W) scan on the device (fp32, int16 or uint8); ``model``: the network, called as
        ``model(x)`` on (1, 1, H', W', D') -> (1, C, H', W', D') logits under ``no_grad``.  -> a namespace: ``labels`` uint8 on the
        model grid (H', W', D') or, with ``native``, on the scan's own (D, H, W); ``uncovered`` (a 0-dim device tensor), the
        number of target voxels no view reached (they carry label 0); ``hist`` (C,) int64, the label counts; ``probs`` fp32,
        ``labels.shape + (C,)``, if asked."""
        return self._predict(model, image, native, want_probs, self.window)

    def predict_batch(self, model, images: torch.Tensor):
        """``images``: a (B, 1, H, W, D) batch on the model's grid, as the data module hands it out (``size`` must be that grid;
        no window is applied again).  A permuted contiguous copy per sample, one ``predict`` each -> a namespace: ``labels``
        (B, H, W, D) uint8 and ``uncovered`` (B,)."""
        nat.require_gpu(images, "TestTimeAugmenter3D")
        if images.dim() != 5 or images.shape[1] != 1:
            raise nat.NativeError(f"TestTimeAugmenter3D: a (B, 1, H, W, D) batch; got {tuple(images.shape)}")
        H, W, D = (int(v) for v in images.shape[2:])
        if (D, H, W) != self.size:
            raise ValueError(f"TestTimeAugmenter3D: the batch's grid (D, H, W) = {(D, H, W)} is not size = {self.size}")
        res = [self._predict(model, images[b, 0].permute(2, 0, 1).contiguous(), False, False, None) for b in range(images.shape[0])]
        return SimpleNamespace(labels=torch.stack([r.labels for r in res]), uncovered=torch.stack([r.uncovered for r in res]))
