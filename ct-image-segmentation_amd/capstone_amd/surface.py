"""Surface metrics on the device: the percentile Hausdorff distance (HD95 by default) and the average symmetric surface distance
between two label maps, per sample and class.  The reference scores with Dice only; the data it targets (MICCAI 2015 head-and-neck
organs at risk) is scored by Dice and the 95 % Hausdorff distance.

Definitions, for class c of sample b:

* surface of c in a label map L: the voxels with ``L == c`` of which an axis neighbour (+-1 along each active axis) lies outside the
  volume or has ``L != c``: ``m ^ scipy.ndimage.binary_erosion(m)`` with scipy's defaults, the edge rule of MONAI's
  ``get_mask_edges``.  Volumes ``(B, H, W, D)`` use all three axes; planes ``(B, H, W)`` are ``(H, W, 1)`` volumes whose third
  axis contributes no neighbours.
* directed distances pred -> target: ``sqrt(d2(v))`` for every v on the prediction's surface, d2 the exact integer squared
  Euclidean distance in voxels to the nearest voxel of the truth's surface; target -> pred is the mirror image.
* percentile distance: ``np.percentile(distances, q)`` with linear interpolation per direction; the symmetric value is the larger
  of the two.  ``q = 100`` is the classical Hausdorff distance.
* ASSD: (sum of both directions' distances) / (number of both surfaces' voxels).
* a class absent from the prediction or from the truth of a sample has NaN in every table: for a distance, 0 means perfect.
  ``reduce_nan_mean`` is the reduction: NaN-ignoring mean over samples per class, then over the classes that have a value.

Distances are in voxels of the grid the labels live on, or, with ``spacing=``, in the unit of the voxel sizes given (millimetres
for CT headers).  Under anisotropic spacing the nearest surface voxel is another voxel, so the physical value is no rescaling of
the voxel one: that path runs its own transform.

Three device stages per launch, no host synchronisation between them: ``ctseg_surface_edges`` (surface masks of both maps, one
byte per voxel and volume, and their voxel counts), ``ctseg_distmap3d_batch`` on those masks (unchanged: its float map is written
and ignored) and ``ctseg_surface_select`` (exact order statistics by a radix select, the maximum, the float64 sum of the roots).
Without a spacing the working set is 15 bytes per voxel and volume (1 mask + 4 squared distances + 4 float map + 6 transform
workspace), times ``2 * (n_classes - 1)`` = 18 volumes per sample: 1.7 GB for one 256 x 256 x 96 sample.  Samples are therefore
processed in groups that keep the working set under ``MAX_WORKING_SET`` bytes (at least one sample per launch).  There is no CPU
fallback.

With ``spacing=`` the middle and last stages are ``ctseg_distmap3d_weighted`` and ``ctseg_surface_select_f32``.  The transform takes
a table of squared voxel sizes per volume and gives float32 squared distances, each the minimum over the other surface's voxels of
``fl(fl(wy dy^2) + fl(fl(wz dz^2) + fl(wx dx^2)))``, one float32 rounding per ``fl``: defined bit for bit, and within 3 * 2^-24
relative of the real squared distance, so within 2^-23 of the distance after the root.  It writes no value map, so the working
set that sizes the launch groups is 11 bytes per voxel and volume on this path (1 mask + 4 squared distances + 6 transform
workspace, ``BYTES_PER_VOXEL_WEIGHTED``): 1.25 GB for the same sample.  The select orders those floats by their bit patterns.
``spacing=(1, 1, 1)`` reproduces the voxel path exactly (``fl(1 * d^2)`` is exact).

``surface_dice`` is the third figure, the surface Dice at tolerance (normalised surface Dice, NSD): the share of the two surfaces
that lies within ``tau`` of the other surface.  It needs no distances, only whether something lies within a few voxels, so it runs
none of the stages above: ``ctseg_surface_dice`` is one launch for the whole batch, without a workspace, that stages tiles of both
label maps in LDS and searches a box bounded by the tolerance.  Its acceptance rule is pinned like the distances: a voxel v of
one surface is *within* iff some voxel u of the other surface of the same class has ``dx^2 + dy^2 + dz^2 <= floor(tau^2)`` in
integers, or with ``spacing=`` the float32 expression above ``<= float32(tau^2)``, which is the weighted distance compared with
that limit (float32 addition of non-negative terms is monotone).  A class that only one of the two maps holds scores 0.0 there,
the formula's value and what MONAI's ``SurfaceDiceMetric`` and Dice give; the distance tables have NaN in that place.
"""
import math
from types import SimpleNamespace

import torch

from . import _native as nat
from .data import utils as DU
from .segloss import N_CLASSES

AXIS_X, AXIS_Y, AXIS_Z = 1, 2, 4
BYTES_PER_VOXEL = 1 + 4 + 4 + DU.WORKSPACE_BYTES_3D      # per voxel of each of the 2 * (C - 1) surface volumes of a sample
BYTES_PER_VOXEL_WEIGHTED = 1 + 4 + DU.WORKSPACE_BYTES_3D  # with spacing: float32 squared distances and no value map
SELECT_ROW_BYTES = 25096                                  # CTSEG_SURFACE_SELECT_ROW_BYTES of include/ctseg_hip.h
SELECT_F32_ROW_BYTES = 41480                              # CTSEG_SURFACE_SELECT_F32_ROW_BYTES
MIN_SPACING, MAX_SPACING = 1e-3, 1e3
MAX_CLASSES = 16
MAX_WORKING_SET = 2 << 30
SURFACE_DICE_MAX_RADIUS = 8                               # CTSEG_SURFACE_DICE_MAX_RADIUS: voxels searched along an axis


def _label_maps(pred, target, who="surface_distances"):
    if pred.shape != target.shape or pred.dim() not in (3, 4):
        raise ValueError(f"{who}: two label maps of one shape, (B, H, W, D) or (B, H, W); got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if pred.is_floating_point() or target.is_floating_point() or pred.dtype == torch.bool or target.dtype == torch.bool:
        raise ValueError(f"{who}: integer label maps, not {pred.dtype} / {target.dtype}")
    if pred.device != target.device:
        raise ValueError(f"{who}: the label maps are on {pred.device} and {target.device}")
    sides = tuple(int(s) for s in pred.shape[1:]) + ((1,) if pred.dim() == 3 else ())
    axes = AXIS_X | AXIS_Y | (AXIS_Z if pred.dim() == 4 else 0)
    if pred.shape[0] < 1 or min(sides) < 1 or max(sides) > DU.MAX_SIDE:
        raise nat.NativeError(f"{who}: at least one sample with sides in 1..{DU.MAX_SIDE} (got {tuple(pred.shape)})")
    return pred.to(torch.uint8).contiguous(), target.to(torch.uint8).contiguous(), sides, axes


def _squared_spacing(spacing, B, n_axes):
    """one ``n_axes``-tuple or ``(B, n_axes)`` voxel sizes -> (B, 3) float32 squared sizes on the host (planes: 1 on the third axis)"""
    s = torch.as_tensor(spacing).detach().to("cpu", torch.float64)
    if s.dim() == 1 and s.shape[0] == n_axes:
        s = s[None].expand(B, n_axes)
    if s.dim() != 2 or tuple(s.shape) != (B, n_axes):
        raise ValueError(f"surface_distances: spacing is {n_axes} voxel sizes or ({B}, {n_axes}) of them, not {tuple(s.shape)}")
    if not bool((torch.isfinite(s) & (s >= MIN_SPACING) & (s <= MAX_SPACING)).all()):
        raise ValueError(f"surface_distances: finite voxel sizes in [{MIN_SPACING:g}, {MAX_SPACING:g}], not {s.tolist()}")
    s = s.to(torch.float32)
    w = torch.ones((B, 3), dtype=torch.float32)
    w[:, :n_axes] = s * s
    return w


def surface_distances(pred, target, n_classes=N_CLASSES, percentile=95.0, samples_per_launch=None, spacing=None):
    """pred, target: integer label maps ``(B, H, W, D)`` or ``(B, H, W)`` on the device -> a namespace of device tensors, C =
    ``n_classes``, direction 0 = pred -> target, 1 = target -> pred:

    ``hd_directed`` (2, B, C-1) float64, ``hd`` (B, C-1), ``hd_max_directed`` (2, B, C-1) (the q = 100 values), ``assd`` (B, C-1),
    ``asd_directed`` (2, B, C-1), ``counts`` (2, B, C-1) int64 surface voxels, and the exact integers the float values come from:
    ``d2_lo``, ``d2_hi``, ``d2_max`` (2, B, C-1) int32, ``gamma`` and ``root_sum`` (2, B, C-1) float64, ``valid`` (2, B, C-1) bool.

    ``spacing``: the voxel sizes along the label map's axes, one triple (a pair for planes) or ``(B, 3)`` / ``(B, 2)`` per sample, as
    a sequence, an array or a tensor; every value finite and in [1e-3, 1e3], else ``ValueError``.  They are read on the host (a
    device tensor is copied back) and squared in float32.  The distances are then in the spacing's unit, and ``d2_lo``, ``d2_hi``,
    ``d2_max`` are float32: the squared physical distances as the weighted transform rounds them (see the module's docstring).
    """
    nat.require_gpu(pred, "surface_distances")
    nat.require_gpu(target, "surface_distances")
    C, q = int(n_classes), float(percentile)
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"surface_distances: 2 <= n_classes <= {MAX_CLASSES}, not {n_classes!r}")
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"surface_distances: a percentile in [0, 100], not {percentile!r}")
    p, t, (X, Y, Z), axes = _label_maps(pred, target)
    B, S, K, dev = p.shape[0], X * Y * Z, C - 1, p.device
    weighted = spacing is not None
    w2 = _squared_spacing(spacing, B, pred.dim() - 1).to(dev) if weighted else None
    row_bytes = SELECT_F32_ROW_BYTES if weighted else SELECT_ROW_BYTES
    if samples_per_launch is None:
        samples_per_launch = max(1, MAX_WORKING_SET // ((BYTES_PER_VOXEL_WEIGHTED if weighted else BYTES_PER_VOXEL) * 2 * K * S))
    G = max(1, min(int(samples_per_launch), B))
    P = 2 * G * K
    edges = torch.empty((P * S,), dtype=torch.uint8, device=dev)
    d2 = torch.empty((P * S,), dtype=torch.float32 if weighted else torch.int32, device=dev)
    dm_ws = torch.empty((DU.WORKSPACE_BYTES_3D * P * S,), dtype=torch.uint8, device=dev)
    sel_ws = torch.empty((P * row_bytes // 8,), dtype=torch.float64, device=dev)
    if not weighted:
        fmap = torch.empty((P * S,), dtype=torch.float32, device=dev)                # the transform's map: written, not read
        table = DU._byte_table(dev)
    counts, stats, fstats = [], [], []
    for b0 in range(0, B, G):
        g = min(G, B - b0)
        rows = 2 * g * K
        cnt = torch.zeros((2, g, K), dtype=torch.int32, device=dev)
        st = torch.empty((2, g, K, 4), dtype=torch.int32, device=dev)
        fs = torch.empty((2, g, K, 2), dtype=torch.float64, device=dev)
        nat.call("ctseg_surface_edges", nat.ptr(p[b0:b0 + g]), nat.ptr(t[b0:b0 + g]), g, X, Y, Z, C, axes, nat.ptr(edges), nat.ptr(cnt))
        if weighted:
            w = w2[b0:b0 + g].view(1, g, 1, 3).expand(2, g, K, 3).contiguous()       # a row of the table per surface volume
            nat.call("ctseg_distmap3d_weighted", nat.ptr(edges), rows, X, Y, Z, nat.ptr(w), nat.ptr(dm_ws),
                     DU.WORKSPACE_BYTES_3D * rows * S, nat.ptr(d2), None)
            nat.call("ctseg_surface_select_f32", nat.ptr(edges), nat.ptr(d2), nat.ptr(cnt), g, X, Y, Z, C, q, nat.ptr(sel_ws),
                     rows * row_bytes, nat.ptr(st), nat.ptr(fs))
        else:
            nat.call("ctseg_distmap3d_batch", nat.ptr(edges), rows, X, Y, Z, DU.REFERENCE, nat.ptr(table), nat.ptr(dm_ws),
                     DU.WORKSPACE_BYTES_3D * rows * S, nat.ptr(fmap), nat.ptr(d2), None)
            nat.call("ctseg_surface_select", nat.ptr(edges), nat.ptr(d2), nat.ptr(cnt), g, X, Y, Z, C, q, nat.ptr(sel_ws),
                     rows * row_bytes, nat.ptr(st), nat.ptr(fs))
        counts.append(cnt)
        stats.append(st)
        fstats.append(fs)
    cnt, st, fs = torch.cat(counts, 1), torch.cat(stats, 1), torch.cat(fstats, 1)
    return _tables(cnt, st[..., :3].contiguous().view(torch.float32) if weighted else st[..., :3], st[..., 3] != 0, fs)


def _tables(cnt, st, valid, fs):
    """the float64 tables from the select's {d2[lo], d2[hi], max} (int32, or float32 with spacing): a few small torch ops"""
    nan = torch.full((), float("nan"), dtype=torch.float64, device=cnt.device)
    n = cnt.to(torch.int64)
    lo, hi = st[..., 0].double().sqrt(), st[..., 1].double().sqrt()
    gamma, root_sum = fs[..., 1], fs[..., 0]
    hd_directed = torch.where(valid, lo + (hi - lo) * gamma, nan)
    both = n[0] + n[1]
    return SimpleNamespace(
        hd_directed=hd_directed, hd=torch.maximum(hd_directed[0], hd_directed[1]),
        hd_max_directed=torch.where(valid, st[..., 2].double().sqrt(), nan),
        asd_directed=torch.where(valid, root_sum / n.clamp(min=1), nan),
        assd=torch.where(valid[0], (root_sum[0] + root_sum[1]) / both.clamp(min=1), nan),
        counts=n, d2_lo=st[..., 0], d2_hi=st[..., 1], d2_max=st[..., 2], gamma=gamma, root_sum=root_sum, valid=valid)


def reduce_nan_mean(table):
    """(N, C-1) per-sample values -> (mean, per_class (C-1,)): per class the mean over the samples that have a value (NaN if
    none has), then the mean over the classes that have one (NaN if none has)"""
    per_class = torch.nanmean(table, dim=0)
    return torch.nanmean(per_class), per_class


def _dice_tables(tolerance, K, w, active, spacing):
    """the host tables of ``surface_dice``: tolerances (K,) float64, the limits (B, K) and the radii (B, K, 3) int32.  ``w``: the
    (B, 3) float32 squared voxel sizes, or None for voxel units with B = 1 row; ``active``: the number of leading active axes"""
    if not torch.is_tensor(tolerance):
        tolerance = torch.as_tensor(tolerance, dtype=torch.float64)                           # (Python floats are float64)
    tau = tolerance.detach().to("cpu", torch.float64)
    if tau.dim() == 0:
        tau = tau.expand(K)
    if tuple(tau.shape) != (K,):
        raise ValueError(f"surface_dice: one tolerance or one per class ({K},), not {tuple(tau.shape)}")
    if not bool((torch.isfinite(tau) & (tau >= 0)).all()):
        raise ValueError(f"surface_dice: finite tolerances >= 0, not {tau.tolist()}")
    sq = tau * tau
    over = SURFACE_DICE_MAX_RADIUS + 1
    if w is None:
        limit = sq.clamp(max=float(1 << 30)).floor().to(torch.int32)[None]                    # (1, K): T2
        radius = torch.tensor([[min(math.isqrt(int(v)), over)] * 3 for v in limit[0].tolist()], dtype=torch.int32)[None]
    else:
        limit = sq.to(torch.float32)[None].expand(w.shape[0], K)                              # (B, K): t2
        dd = torch.arange(over + 1, dtype=torch.float32) ** 2                                 # d^2, exact
        ok = (w[:, None, :, None] * dd) <= limit[:, :, None, None]                            # fl(w_a * d^2) <= t2: (B, K, 3, d)
        radius = (ok.sum(-1) - 1).to(torch.int32)                                             # monotone in d: the largest accepted
    radius = radius.clone()
    radius[..., active:] = 0
    if int(radius.max()) > SURFACE_DICE_MAX_RADIUS:
        b, k, a = (int(i) for i in (radius > SURFACE_DICE_MAX_RADIUS).nonzero()[0])
        unit = "voxel units" if spacing is None else f"spacing {torch.as_tensor(spacing).tolist()}"
        raise ValueError(f"surface_dice: class {k + 1} with tolerance {tau[k].item():g} in {unit} needs a search radius above "
                         f"{SURFACE_DICE_MAX_RADIUS} voxels along axis {a} (sample {b}); the limit is {SURFACE_DICE_MAX_RADIUS}")
    return tau, limit, radius


def surface_dice(pred, target, tolerance, n_classes=N_CLASSES, spacing=None):
    """The surface Dice at tolerance (normalised surface Dice) of integer label maps ``(B, H, W, D)`` or ``(B, H, W)`` on the
    device -> a namespace, C = ``n_classes``, direction 0 = pred -> target, 1 = target -> pred:

    ``nsd`` (B, C-1) float64 = (within[0] + within[1]) / (counts[0] + counts[1]), ``nsd_directed`` (2, B, C-1) = within / counts,
    ``within`` and ``counts`` (2, B, C-1) int64: the surface voxels with a voxel of the other map's surface of the same class
    within the tolerance, and all surface voxels; ``limit`` (B, C-1), the table the kernel compared with, and ``radius`` (B, C-1, 3)
    int32 on the host, the search radii per axis.

    ``tolerance``: one value or one per class ``(C-1,)``, finite and >= 0, in voxels or, with ``spacing``, in its unit; 0 counts
    coinciding surface voxels.  The rule is exact: squared voxel offsets against ``floor(tolerance^2)`` in integers, or the float32
    expression of the weighted distances against ``float32(tolerance^2)`` (module docstring).  ``spacing`` as in
    ``surface_distances``.  No radius may exceed ``SURFACE_DICE_MAX_RADIUS`` = 8 voxels (``ValueError``): clinical tolerances of
    1 to 3 mm on CT grids need at most 6.

    ``nsd`` is NaN only where both surfaces are empty.  A class that one map holds and the other lacks scores 0.0, as in MONAI's
    ``SurfaceDiceMetric`` and as Dice does; this differs from ``surface_distances``, where such a class is NaN.  ``nsd_directed``
    is NaN where that direction's surface is empty.  One launch for the whole batch; there is no CPU fallback."""
    nat.require_gpu(pred, "surface_dice")
    nat.require_gpu(target, "surface_dice")
    C = int(n_classes)
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"surface_dice: 2 <= n_classes <= {MAX_CLASSES}, not {n_classes!r}")
    p, t, (X, Y, Z), axes = _label_maps(pred, target, "surface_dice")
    B, K, dev = p.shape[0], C - 1, p.device
    w = None if spacing is None else _squared_spacing(spacing, B, pred.dim() - 1)
    _, limit, radius = _dice_tables(tolerance, K, w, pred.dim() - 1, spacing)
    limit = limit.expand(B, K).contiguous().to(dev)
    radius = radius.expand(B, K, 3).contiguous()
    w_dev = None if w is None else w.to(dev)
    tables = torch.zeros((2, 2, B, K), dtype=torch.int32, device=dev)                         # counts, within
    nat.call("ctseg_surface_dice", nat.ptr(p), nat.ptr(t), B, X, Y, Z, C, axes, nat.ptr(radius), nat.ptr(limit), nat.ptr(w_dev),
             nat.ptr(tables[0]), nat.ptr(tables[1]))
    counts, within = tables[0].to(torch.int64), tables[1].to(torch.int64)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    both = counts[0] + counts[1]
    return SimpleNamespace(
        nsd=torch.where(both > 0, (within[0] + within[1]).double() / both.clamp(min=1).double(), nan),
        nsd_directed=torch.where(counts > 0, within.double() / counts.clamp(min=1).double(), nan),
        within=within, counts=counts, limit=limit, radius=radius)
