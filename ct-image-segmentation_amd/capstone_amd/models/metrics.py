"""Drop-in for reference capstone/models/metrics.py (+ capstone/volumetric/metrics.py:5-20).

``DiceMetricWrapper()(pred_labels, true_labels) -> (mean Dice, per-class Dice (9,))`` with the reference's
aggregation (per-sample per-class Dice, NaN where the class is absent from the truth; NaN-aware batch
mean per class; mean over the 9 classes — models/temp.py:173-214, :271-273; models/metrics.py:15-21).
The reference builds two (B,10,*sp) fp32 one-hots and their product; here exact integer counts come
from one pass over the two label maps (ctseg_dice_counts) — or for free from the fused loss pass.
"""
import torch

from .. import _native as nat
from .. import segloss, surface
from ..segloss import N_CLASSES


class DiceMetricWrapper(object):
    def __init__(self):
        self.n_classes = N_CLASSES

    def __call__(self, input, target):
        nat.require_gpu(input, "DiceMetricWrapper")
        B = input.shape[0]
        cnt = getattr(input, "_ctseg_counts", None)   # predictions that came out of the fused loss pass
        if cnt is None:
            p = input.reshape(B, -1).to(torch.uint8).contiguous()
            t = target.reshape(B, -1).to(torch.uint8).contiguous()
            cnt = segloss.dice_counts(p, t, self.n_classes)
        self.last_counts = cnt      # (B, 3, C) int64: what epoch_dice_across_ranks gathers at N > 1
        return segloss.dice_metric(cnt)


class SurfaceDistanceMetricWrapper(object):
    """``SurfaceDistanceMetricWrapper(percentile=95.0)(pred_labels, true_labels) -> (mean, per-class (9,))`` of the symmetric
    percentile Hausdorff distance in voxels (``capstone_amd.surface``): label maps ``(B, H, W, D)`` or planes ``(B, H, W)``, in the
    shape of ``DiceMetricWrapper``.  Not in the reference, which scores with Dice only.  A class absent from the prediction or the
    truth of a sample has no value there (NaN, never 0); the per-class value is the mean over the samples that have one, the mean
    that over the classes that have one.  ``last`` keeps the full tables of the call and ``assd()`` gives (mean, per-class) of the
    average symmetric surface distance from the same call.  ``spacing``: the voxel sizes of the label grid (a triple, a pair for
    planes, or one row per sample), fixed at construction or given per call, which takes precedence; the distances are then in
    that unit (``surface.surface_distances``)."""

    def __init__(self, percentile=95.0, spacing=None):
        self.n_classes = N_CLASSES
        self.percentile = float(percentile)
        self.spacing = spacing
        self.last = None

    def __call__(self, input, target, spacing=None):
        nat.require_gpu(input, "SurfaceDistanceMetricWrapper")
        self.last = surface.surface_distances(input, target, self.n_classes, self.percentile,
                                              spacing=self.spacing if spacing is None else spacing)
        return surface.reduce_nan_mean(self.last.hd)

    def assd(self):
        if self.last is None:
            raise RuntimeError("SurfaceDistanceMetricWrapper.assd(): call the wrapper on a batch first")
        return surface.reduce_nan_mean(self.last.assd)


class SurfaceDiceMetricWrapper(object):
    """``SurfaceDiceMetricWrapper(tolerance)(pred_labels, true_labels) -> (mean, per-class (9,))`` of the surface Dice at tolerance
    (normalised surface Dice, ``capstone_amd.surface.surface_dice``), called like ``SurfaceDistanceMetricWrapper``.  ``tolerance``:
    one value or one per class, in voxels or in the unit of ``spacing``.  A class in neither map of a sample has no value there
    (NaN) and is skipped by the means; a class in only one of them scores 0.  ``last`` keeps the full tables of the call."""

    def __init__(self, tolerance, spacing=None):
        self.n_classes = N_CLASSES
        self.tolerance = tolerance
        self.spacing = spacing
        self.last = None

    def __call__(self, input, target, spacing=None):
        nat.require_gpu(input, "SurfaceDiceMetricWrapper")
        self.last = surface.surface_dice(input, target, self.tolerance, self.n_classes,
                                         spacing=self.spacing if spacing is None else spacing)
        return surface.reduce_nan_mean(self.last.nsd)
