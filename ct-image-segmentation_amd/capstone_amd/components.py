"""Connected components of label maps on the device, and the post-processing that the surface metrics call for: keep the largest
component of every class, drop components below a size.  The percentile Hausdorff distance is the metric that a stray island ruins
(a dozen false-positive voxels at the far end of a volume barely move Dice and push HD95 to hundreds of voxels), so pipelines on
the MICCAI 2015 head-and-neck data report it after this step; MONAI ships it as ``KeepLargestConnectedComponent``.  The reference
has neither.

Definitions, for a label map ``(B, H, W, D)`` (or planes ``(B, H, W)``, which are ``(H, W, 1)`` volumes whose third axis gives no
neighbours) and classes ``1..n_classes-1``:

* two voxels are neighbours when they differ by +-1 along at most ``connectivity`` axes: 1, 2, 3 mean 6, 18, 26 neighbours in a
  volume, and 1, 2 mean 4, 8 in a plane.  ``connectivity=None`` is the full one (3 for volumes, 2 for planes), the default of
  skimage and MONAI.
* a component is a maximal set of voxels of ONE label joined by neighbour steps inside its sample.  Classes never join, samples
  never join.  Label 0 and labels ``>= n_classes`` are in no component.
* ``ids[v]`` is the smallest linear index within the sample over the voxels of v's component (its representative), -1 off the
  components; ``sizes[v]`` is the component's voxel count at the representative and 0 elsewhere.  That form is unique.
* the largest component of a class in a sample: the most voxels; among equals the smallest representative, the one whose first
  voxel comes first in raster order, which is what ``argmax(bincount(labels))`` picks over scipy / skimage labels.

Two native calls per launch group, no host synchronisation: ``ctseg_components_label`` (three launches) and
``ctseg_components_keep`` (four).  Integers only: the same bits on every run.  The working set is 10 bytes per voxel (labels 1 +
ids 4 + sizes 4 + cleaned map 1); samples are processed in groups that keep it under ``MAX_WORKING_SET`` and under the 2^31 voxels
of one launch.  There is no CPU fallback.

``fill_holes`` repairs the opposite defect, a cavity inside a predicted organ (MONAI's ``FillHoles``): every cavity adds a closed
shell of surface voxels deep inside the true organ, which pull NSD, ASSD and the directed Hausdorff percentile the wrong way while
Dice barely moves.  With the neighbours above:

* a background component is a maximal set of voxels of label exactly 0 joined by neighbour steps inside its sample; it touches
  the boundary when one of its voxels has coordinate 0 or side - 1 along an active axis (a plane's third axis is not active);
* its border set holds the labels of all neighbours of its voxels that are not 0, a label ``>= n_classes`` counting as one foreign
  label; the same ``connectivity`` serves the component search and the border set, as in
  ``scipy.ndimage.binary_fill_holes(structure=generate_binary_structure(rank, connectivity))``;
* the component is a hole of class c when it does not touch the boundary, its border set is exactly ``{c}``, c is in
  ``applied_labels`` and, with ``max_size``, it has at most that many voxels.  A hole's voxels become c, everything else is copied.
  One pass: an island of class 2 in a cavity of class 1 leaves the ring between them, and a cavity inside the island takes 2.

One native call per launch group, ``ctseg_fill_holes`` (six launches: the background map, the three labelling launches on it, a
border pass, the rewrite), 15 bytes per voxel (labels 1 + workspace 13 + filled map 1).
"""
from types import SimpleNamespace

import torch

from . import _native as nat
from .data import utils as DU
from .segloss import N_CLASSES

AXIS_X, AXIS_Y, AXIS_Z = 1, 2, 4
BYTES_PER_VOXEL = 1 + 4 + 4 + 1                           # labels, ids, sizes, the cleaned map
FILL_BYTES_PER_VOXEL = 1 + 13 + 1                         # labels, the workspace of ctseg_fill_holes, the filled map
KEEP_ROW_BYTES = 16                                       # CTSEG_COMPONENTS_KEEP_ROW_BYTES of include/ctseg_hip.h
MAX_CLASSES = 16
MAX_WORKING_SET = 2 << 30
MAX_VOXELS = (1 << 31) - 1                                # of one launch


def _label_map(labels, what):
    if labels.dim() not in (3, 4):
        raise ValueError(f"{what}: a label map (B, H, W, D) or (B, H, W); got {tuple(labels.shape)}")
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError(f"{what}: an integer label map, not {labels.dtype}")
    sides = tuple(int(s) for s in labels.shape[1:]) + ((1,) if labels.dim() == 3 else ())
    if labels.shape[0] < 1 or min(sides) < 1 or max(sides) > DU.MAX_SIDE:
        raise ValueError(f"{what}: at least one sample with sides in 1..{DU.MAX_SIDE} (got {tuple(labels.shape)})")
    axes = AXIS_X | AXIS_Y | (AXIS_Z if labels.dim() == 4 else 0)
    return labels.to(torch.uint8).contiguous(), sides, axes


def _arguments(labels, n_classes, connectivity, what):
    nat.require_gpu(labels, what)
    C = int(n_classes)
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"{what}: 2 <= n_classes <= {MAX_CLASSES}, not {n_classes!r}")
    n_axes = labels.dim() - 1
    if connectivity is None:
        connectivity = n_axes
    if isinstance(connectivity, bool) or connectivity not in (1, 2, 3) or connectivity > max(n_axes, 1):
        raise ValueError(f"{what}: connectivity is None or 1..{n_axes} for {n_axes} axes, not {connectivity!r}")
    return C, int(connectivity)


def _class_mask(applied_labels, C, what):
    if applied_labels is None:
        return (1 << C) - 2
    mask = 0
    for c in applied_labels:
        if isinstance(c, bool) or int(c) != c or not 1 <= int(c) < C:
            raise ValueError(f"{what}: applied_labels are class indices in 1..{C - 1}, not {c!r}")
        mask |= 1 << int(c)
    return mask


def _group(B, S, bytes_per_voxel, samples_per_launch):
    """samples of S voxels per launch group: by request, else under ``MAX_WORKING_SET``; always under 2^31 voxels"""
    if samples_per_launch is None:
        samples_per_launch = max(1, MAX_WORKING_SET // (bytes_per_voxel * S))
    return max(1, min(int(samples_per_launch), B, MAX_VOXELS // S))


def _run(labels, C, connectivity, class_mask, keep_largest, min_size, samples_per_launch, what):
    """the two native calls per group of samples -> (ids, sizes, cleaned map, table (B, C-1, 4)), all as [B][X][Y][Z]"""
    p, (X, Y, Z), axes = _label_map(labels, what)
    B, S, dev = p.shape[0], X * Y * Z, p.device
    G = _group(B, S, BYTES_PER_VOXEL, samples_per_launch)
    ids = torch.empty((B, X, Y, Z), dtype=torch.int32, device=dev)
    sizes = torch.empty((B, X, Y, Z), dtype=torch.int32, device=dev)
    out = torch.empty((B, X, Y, Z), dtype=torch.uint8, device=dev)
    table = torch.empty((B, C - 1, 4), dtype=torch.int32, device=dev)
    ws = torch.empty((G * (C - 1) * KEEP_ROW_BYTES // 8,), dtype=torch.int64, device=dev)
    for b0 in range(0, B, G):
        g = min(G, B - b0)
        sl = slice(b0, b0 + g)
        nat.call("ctseg_components_label", nat.ptr(p[sl]), g, X, Y, Z, C, connectivity, axes, nat.ptr(ids[sl]), nat.ptr(sizes[sl]))
        nat.call("ctseg_components_keep", nat.ptr(p[sl]), nat.ptr(ids[sl]), nat.ptr(sizes[sl]), g, X, Y, Z, C, class_mask,
                 int(keep_largest), min_size, nat.ptr(ws), g * (C - 1) * KEEP_ROW_BYTES, nat.ptr(out[sl]), nat.ptr(table[sl]))
    return ids, sizes, out, table


def connected_components(labels, n_classes=N_CLASSES, connectivity=None, samples_per_launch=None):
    """labels: an integer label map ``(B, H, W, D)`` or ``(B, H, W)`` on the device -> a namespace of device tensors: ``ids`` and
    ``sizes`` (int32, the labels' shape; see the module's docstring) and ``count`` ``(B, n_classes - 1)`` int64, the number of
    components of every class"""
    what = "connected_components"
    C, connectivity = _arguments(labels, n_classes, connectivity, what)
    ids, sizes, _, table = _run(labels, C, connectivity, 0, False, 0, samples_per_launch, what)
    return SimpleNamespace(ids=ids.view(labels.shape), sizes=sizes.view(labels.shape), count=table[..., 0].to(torch.int64))


def keep_largest_component(labels, n_classes=N_CLASSES, applied_labels=None, connectivity=None, min_size=0, keep_largest=True,
                           samples_per_launch=None):
    """labels as for ``connected_components`` -> a namespace: ``labels``, the cleaned map in the input's dtype and shape, and four
    ``(B, n_classes - 1)`` int64 tables of the INPUT's components: ``count``, ``largest`` (voxels of the largest), ``representative``
    (its smallest linear index in the sample, -1 where the class is absent) and ``removed`` (voxels set to 0).

    A voxel of a class in ``applied_labels`` (``None``: every class ``1..n_classes-1``; otherwise an iterable of such indices) keeps
    its label when its component has at least ``min_size`` voxels and, with ``keep_largest``, is the largest of its class in its
    sample; otherwise it becomes 0.  Every other voxel is copied."""
    what = "keep_largest_component"
    C, connectivity = _arguments(labels, n_classes, connectivity, what)
    mask = _class_mask(applied_labels, C, what)
    if isinstance(min_size, bool) or int(min_size) != min_size or not 0 <= int(min_size) < 1 << 31:
        raise ValueError(f"{what}: min_size is an integer >= 0, not {min_size!r}")
    _, _, out, table = _run(labels, C, connectivity, mask, bool(keep_largest), int(min_size), samples_per_launch, what)
    t = table.to(torch.int64)
    return SimpleNamespace(labels=out.view(labels.shape).to(labels.dtype), count=t[..., 0], largest=t[..., 1], representative=t[..., 2],
                           removed=t[..., 3])


class KeepLargestConnectedComponent(object):
    """``KeepLargestConnectedComponent(applied_labels=None, connectivity=None, min_size=0)(label_map) -> cleaned label map``: the
    callable of MONAI's name on integer label maps ``(B, H, W, D)`` or ``(B, H, W)`` on the device.  ``last`` keeps the namespace of
    ``keep_largest_component`` of the call."""

    def __init__(self, applied_labels=None, connectivity=None, min_size=0, n_classes=N_CLASSES):
        self.applied_labels = None if applied_labels is None else tuple(applied_labels)
        self.connectivity, self.min_size, self.n_classes = connectivity, min_size, n_classes
        self.last = None

    def __call__(self, label_map):
        self.last = keep_largest_component(label_map, self.n_classes, self.applied_labels, self.connectivity, self.min_size)
        return self.last.labels


def fill_holes(labels, n_classes=N_CLASSES, applied_labels=None, connectivity=None, max_size=0, samples_per_launch=None):
    """labels as for ``connected_components`` -> a namespace: ``labels``, the filled map in the input's dtype and shape, and two
    ``(B, n_classes - 1)`` int64 tables: ``holes`` (holes filled per class) and ``filled`` (voxels filled per class).

    A component of label 0 that does not reach its sample's boundary and whose neighbours off the background all carry one class c
    of ``applied_labels`` (``None``: every class) takes c, unless ``max_size > 0`` and it has more voxels than that; every other
    voxel is copied (the module's docstring has the rule in full)."""
    what = "fill_holes"
    C, connectivity = _arguments(labels, n_classes, connectivity, what)
    mask = _class_mask(applied_labels, C, what)
    if isinstance(max_size, bool) or int(max_size) != max_size or not 0 <= int(max_size) < 1 << 31:
        raise ValueError(f"{what}: max_size is an integer >= 0 (0: no limit), not {max_size!r}")
    p, (X, Y, Z), axes = _label_map(labels, what)
    B, S, dev = p.shape[0], X * Y * Z, p.device
    G = _group(B, S, FILL_BYTES_PER_VOXEL, samples_per_launch)
    need = nat.lib().ctseg_fill_holes_workspace_bytes(G, X, Y, Z, C)
    if need < 0:
        nat.check(-1, "ctseg_fill_holes_workspace_bytes")
    out = torch.empty((B, X, Y, Z), dtype=torch.uint8, device=dev)
    table = torch.empty((B, C - 1, 2), dtype=torch.int32, device=dev)
    ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
    for b0 in range(0, B, G):
        g = min(G, B - b0)
        sl = slice(b0, b0 + g)
        nat.call("ctseg_fill_holes", nat.ptr(p[sl]), g, X, Y, Z, C, connectivity, axes, mask, int(max_size), nat.ptr(ws), need,
                 nat.ptr(out[sl]), nat.ptr(table[sl]))
    t = table.to(torch.int64)
    return SimpleNamespace(labels=out.view(labels.shape).to(labels.dtype), holes=t[..., 0], filled=t[..., 1])


class FillHoles(object):
    """``FillHoles(applied_labels=None, connectivity=None, max_size=0)(label_map) -> filled label map``: the callable of MONAI's
    name on integer label maps ``(B, H, W, D)`` or ``(B, H, W)`` on the device.  ``last`` keeps the namespace of ``fill_holes`` of the
    call."""

    def __init__(self, applied_labels=None, connectivity=None, max_size=0, n_classes=N_CLASSES):
        self.applied_labels = None if applied_labels is None else tuple(applied_labels)
        self.connectivity, self.max_size, self.n_classes = connectivity, max_size, n_classes
        self.last = None

    def __call__(self, label_map):
        self.last = fill_holes(label_map, self.n_classes, self.applied_labels, self.connectivity, self.max_size)
        return self.last.labels
