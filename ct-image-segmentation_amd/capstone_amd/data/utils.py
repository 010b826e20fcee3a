"""Device counterpart of reference capstone/data/utils.py: ``compute_distance_map`` (``ctseg_distmap2d_batch``).

The reference allocates its result with ``np.zeros_like(mask)`` and its masks are ``uint8`` (process_miccai.py:68,110), so the
assignment of ``distance(negmask) * negmask - (distance(posmask) - 1) * posmask`` truncates toward zero and wraps modulo 256 before
the final ``/ 255.0``.  With exact integer squared distances the stored byte is

    k = isqrt(d2_to_foreground) & 255            outside (mask == 0)
    k = (-(isqrt(d2_to_background) - 1)) & 255   inside  (mask != 0)
    k = 0                                        on a plane whose class is absent

and the map is ``k / 255.0``: a pure integer function of the mask, which the device reproduces bit for bit (the default, what the
reference's models were trained with).  ``signed=True`` is the evidently intended map of the LIVIAETS original the reference
adapted: ``d_out / 255`` outside and ``-(d_in - 1) / 255`` inside, in float32.  A plane with no background pixel at all has no
defined reference value (scipy's output there is an artefact); it is all zero here, in both modes.  There is no CPU fallback.
"""
import numpy as np
import torch

from .. import _native as nat

REFERENCE, SIGNED = 0, 1
MAX_SIDE = 1024                          # DM_MAX_SIDE of csrc/distmap2d.hip
_TABLES = {}


def _byte_table(device):
    """float32(k / 255.0) for the 256 bytes: the float32 rounding of the reference's float64 value, by construction"""
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(np.float32(np.arange(256) / 255.0)).to(device)
    return _TABLES[key]


def compute_distance_map(masks: torch.Tensor, signed: bool = False, return_d2: bool = False):
    """masks: device uint8 / bool (C, H, W) or (B, C, H, W), nonzero = foreground -> fp32 maps of the same shape; with
    ``return_d2`` also the int32 squared distances to the nearest foreground and background pixel (-1 where the plane has none)."""
    nat.require_gpu(masks, "compute_distance_map")
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() not in (3, 4):
        raise ValueError(f"compute_distance_map: a uint8 / bool (C, H, W) or (B, C, H, W) tensor, not {masks.dtype} {tuple(masks.shape)}")
    m = masks.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    H, W = (int(v) for v in m.shape[-2:])
    P = m.numel() // max(H * W, 1)
    if P < 1 or H < 1 or W < 1 or max(H, W) > MAX_SIDE:
        raise nat.NativeError(f"compute_distance_map: at least one plane with sides in 1..{MAX_SIDE} (got {tuple(masks.shape)})")
    dev = m.device
    out = torch.empty(m.shape, dtype=torch.float32, device=dev)
    d2_fg = torch.empty(m.shape, dtype=torch.int32, device=dev) if return_d2 else None
    d2_bg = torch.empty(m.shape, dtype=torch.int32, device=dev) if return_d2 else None
    workspace = torch.empty((P * H * W,), dtype=torch.int32, device=dev)    # the column pass's two uint16 per pixel
    nat.call("ctseg_distmap2d_batch", nat.ptr(m), P, H, W, SIGNED if signed else REFERENCE, nat.ptr(_byte_table(dev)),
             nat.ptr(workspace), workspace.numel() * 4, nat.ptr(out), nat.ptr(d2_fg), nat.ptr(d2_bg))
    return (out, d2_fg, d2_bg) if return_d2 else out
