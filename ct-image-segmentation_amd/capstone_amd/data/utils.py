"""Device counterpart of reference capstone/data/utils.py: ``compute_distance_map`` (``ctseg_distmap2d_batch`` for planes,
``ctseg_distmap3d_batch`` for volumes: the reference's function is rank-agnostic, ``spatial_dims`` says which is meant here).

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
MAX_SIDE = 1024                          # DM_MAX_SIDE of csrc/distmap_common.h: planes and volumes alike
WORKSPACE_BYTES_3D = 6                   # per voxel, ctseg_distmap3d_batch (include/ctseg_hip.h)
_TABLES = {}


def _byte_table(device):
    """float32(k / 255.0) for the 256 bytes: the float32 rounding of the reference's float64 value, by construction"""
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(np.float32(np.arange(256) / 255.0)).to(device)
    return _TABLES[key]


def compute_distance_map(masks: torch.Tensor, signed: bool = False, return_d2: bool = False, spatial_dims: int = 2):
    """masks: device uint8 / bool (C, H, W) or (B, C, H, W), nonzero = foreground -> fp32 maps of the same shape; with
    ``return_d2`` also the int32 squared distances to the nearest foreground and background pixel (-1 where the plane has none).
    ``spatial_dims=3``: (C, H, W, D) or (B, C, H, W, D) volumes and the 3-D distances (``ctseg_distmap3d_batch``)."""
    nat.require_gpu(masks, "compute_distance_map")
    if spatial_dims not in (2, 3):
        raise ValueError(f"compute_distance_map: spatial_dims 2 or 3, not {spatial_dims!r}")
    nd = spatial_dims
    if masks.dtype not in (torch.uint8, torch.bool) or masks.dim() not in (nd + 1, nd + 2):
        want = "(C, H, W) or (B, C, H, W)" if nd == 2 else "(C, H, W, D) or (B, C, H, W, D)"
        raise ValueError(f"compute_distance_map: a uint8 / bool {want} tensor, not {masks.dtype} {tuple(masks.shape)}")
    m = masks.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    sides = tuple(int(v) for v in m.shape[-nd:])
    n = m.numel()
    P = n // max(int(np.prod(sides)), 1)
    if P < 1 or min(sides) < 1 or max(sides) > MAX_SIDE:
        raise nat.NativeError(f"compute_distance_map: at least one {'plane' if nd == 2 else 'volume'} with sides in 1..{MAX_SIDE} "
                              f"(got {tuple(masks.shape)})")
    dev = m.device
    out = torch.empty(m.shape, dtype=torch.float32, device=dev)
    d2_fg = torch.empty(m.shape, dtype=torch.int32, device=dev) if return_d2 else None
    d2_bg = torch.empty(m.shape, dtype=torch.int32, device=dev) if return_d2 else None
    if nd == 2:
        workspace = torch.empty((4 * n,), dtype=torch.uint8, device=dev)    # the column pass's two uint16 per pixel
        entry = "ctseg_distmap2d_batch"
    else:
        workspace = torch.empty((WORKSPACE_BYTES_3D * n,), dtype=torch.uint8, device=dev)
        entry = "ctseg_distmap3d_batch"
    nat.call(entry, nat.ptr(m), P, *sides, SIGNED if signed else REFERENCE, nat.ptr(_byte_table(dev)),
             nat.ptr(workspace), workspace.numel(), nat.ptr(out), nat.ptr(d2_fg), nat.ptr(d2_bg))
    return (out, d2_fg, d2_bg) if return_d2 else out
