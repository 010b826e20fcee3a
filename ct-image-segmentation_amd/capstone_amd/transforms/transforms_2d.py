"""Drop-in names of reference capstone/transforms/transforms_2d.py on the device.

``WINDOWING_CONFIG``, ``apply_window``, ``WindowedChannels``, ``WindowingBase`` and its three subclasses keep the reference's
constructor arguments and ``apply`` method but take **GPU tensors**, like the 3-D ``Resize3D``: one (H, W) or (H, W, 1) slice in,
(H, W, C) out, computed by the windowing stage of ``ctseg_pipeline2d_batch`` (an identity crop, no normalization).  The value is
the reference's float64 value cast to fp32 (the fused pipeline keeps the float64 internally and casts where ``A.Normalize``
does).  CPU tensors raise ``NativeError``: there is no CPU fallback.
"""
from typing import List, Tuple

import numpy as np
import torch

from .. import _native as nat
from .pipeline2d import CROP, SliceStore2D, pipeline2d_batch

WINDOWING_CONFIG = {"brain": (80, 40), "soft_tissue": (350, 20), "bone": (2800, 600)}


def _windowed(image: torch.Tensor, windows, shift: bool) -> torch.Tensor:
    nat.require_gpu(image, "apply_window")
    if image.dim() == 3:
        assert image.shape[2] == 1, "a slice is (H, W) or (H, W, 1)"
        image = image[:, :, 0]
    H, W = image.shape
    if image.dtype not in (torch.int16, torch.uint8, torch.float32):
        image = image.float()
    store = SliceStore2D.__new__(SliceStore2D)
    store.K, store.masks, store.images, store.device = 0, None, image.contiguous().reshape(-1), image.device
    store.table = np.array([[0, 0, H, W]], dtype=np.int64)
    table = np.array([[0, 0, H, W, 0, 0, 0, 0]], dtype=np.int64)
    out = pipeline2d_batch(store, table, CROP, (H, W), windows, shift, want_masks=False)[0]
    return out[0].permute(1, 2, 0)                          # (H, W, C) view of the (C, H, W) result


def apply_window(image: torch.Tensor, window_width: int, window_level: int, shift: bool = True) -> torch.Tensor:
    """reference :97-107 -> (H, W, 1) fp32"""
    return _windowed(image, [(window_width, window_level)], shift)


class WindowedChannels:
    def __init__(self, windows=["brain", "soft_tissue", "bone"], shift: bool = True, always_apply: bool = False, p: float = 1.0):
        self.windows = windows
        self.shift = shift

    def apply(self, image: torch.Tensor, **params) -> torch.Tensor:
        return _windowed(image, [WINDOWING_CONFIG[w] for w in self.windows], self.shift)     # (H, W, C), C = number of windows

    def __call__(self, image, **params):
        return {"image": self.apply(image), **params}

    def get_transform_init_args_names(self) -> List:
        return []


class WindowingBase:
    def __init__(self, window_width: int, window_level: int, shift: bool = True, always_apply: bool = False, p: float = 1.0) -> None:
        self.window_width = window_width
        self.window_level = window_level
        self.shift = shift

    def apply(self, image: torch.Tensor, **params) -> torch.Tensor:
        return apply_window(image, self.window_width, self.window_level, self.shift)

    def __call__(self, image, **params):
        return {"image": self.apply(image), **params}

    def get_transform_init_args_names(self) -> Tuple:
        return ("window_width", "window_level")


class BrainWindowing(WindowingBase):
    def __init__(self, shift: bool = True, always_apply: bool = False, p: float = 1.0) -> None:
        super().__init__(*WINDOWING_CONFIG["brain"], shift=shift, always_apply=always_apply, p=p)


class SoftTissueWindowing(WindowingBase):
    def __init__(self, shift: bool = True, always_apply: bool = False, p: float = 1.0) -> None:
        super().__init__(*WINDOWING_CONFIG["soft_tissue"], shift=shift, always_apply=always_apply, p=p)


class BoneWindowing(WindowingBase):
    def __init__(self, shift: bool = True, always_apply: bool = False, p: float = 1.0) -> None:
        super().__init__(*WINDOWING_CONFIG["bone"], shift=shift, always_apply=always_apply, p=p)
