"""Drop-in for reference capstone/training/utils.py: ``_squash_masks`` / ``_squash_predictions`` (:13-20) and the mixup
helpers ``weighted_mixup`` / ``mixup_data`` / ``mixup_tensors`` (:23-56) with the reference's names, its module-level ``RNG``
and ``ANNOTATION_COUNT``.  lambda is a host float drawn from ``RNG``; the partner index is drawn on the device and stays there."""
import numpy as np
import torch

from .. import _native as nat
from .. import segloss

RNG = np.random.default_rng(seed=12342)
ANNOTATION_COUNT = torch.as_tensor([601, 44, 601, 94, 88, 535, 549, 280, 253])


def _squash_masks(masks, n_classes, device=None):
    """2-D variant (B, K, H, W) -> (B, H, W) int64; same kernel."""
    lab_u8, lab_i64, hist = segloss.squash_masks(masks, n_classes, want_i64=True)
    lab_i64._ctseg_labels = (lab_u8, hist)
    return lab_i64


def _squash_predictions(preds):
    """softmax(dim=1).argmax(dim=1) with the reference's tie behaviour (first maximal softmax value),
    fused into one pass over the logits: (B, C, *sp) fp32 -> (B, *sp) int64."""
    nat.require_gpu(preds, "_squash_predictions")
    from ..models.losses import _as_cl
    B, C = preds.shape[:2]
    ptr, ld, keep = _as_cl(preds.float() if preds.dtype != torch.float32 else preds)
    eng = segloss.SegLossEngine(preds.device, B, preds[0, 0].numel(), C)
    out = eng.predictions(ptr, ld)
    return out.reshape((B,) + tuple(preds.shape[2:])).long()


def mixup_tensors(tensor_1, tensor_2, lambda_):
    return lambda_ * tensor_1 + (1 - lambda_) * tensor_2


def _mixup_images(images, index, lambda_):
    """mixup_tensors(images, images[index], lambda_) in one pass, bit-equal to the torch expression; no gathered copy"""
    nat.require_gpu(images, "mixup")
    x = images.contiguous()
    if x.dtype != torch.float32:
        raise nat.NativeError(f"mixup: images are {x.dtype}; the mixing pass takes fp32 images")
    out = torch.empty_like(x)
    perm = index.to(device=x.device, dtype=torch.int32).contiguous()
    nat.call("ctseg_mixup_images", x.data_ptr(), perm.data_ptr(), x.shape[0], x[0].numel(), float(lambda_), out.data_ptr())
    return out


def mixup_probability(present):
    """reference :26-36 on the (B, 9) presence table: the chance of each sample to be drawn as a partner"""
    count = ANNOTATION_COUNT.to(device=present.device, dtype=torch.float32)
    ind = torch.einsum("ij,j->ij", present.float(), count)
    ind = ind + (ind.sum(dim=1, keepdim=True) == 0).float() * float(ANNOTATION_COUNT.sum())   # no NaNs for an empty sample
    probability = 1.0 / (ind.sum(dim=1) / (ind > 0).sum(dim=1))
    return probability / probability.sum()


def weighted_mixup(images, masks, alpha=0.2, device=None, *, index=None, lambda_=None):
    """reference :23-42 -> (mixed_images, index, lambda_).  ``index`` / ``lambda_`` force the draw (torch.multinomial's stream
    differs between devices).  The masks are read once: the pass that finds which structures each sample holds also squashes
    them, and the label maps are left on ``masks`` for the ``_squash_masks`` call that follows in the step."""
    nat.require_gpu(images, "weighted_mixup")
    batch_size = images.shape[0]
    present = getattr(masks, "_ctseg_present", None)
    if present is None or getattr(masks, "_ctseg_labels", None) is None:
        lab_u8, lab_i64, hist, present = segloss.squash_masks(masks, masks.shape[1] + 1, want_i64=True, want_present=True)
        masks._ctseg_labels = (lab_u8, hist, lab_i64)
    # (else: a batch of the device input pipeline, capstone_amd/transforms BatchPipeline2D — it squashed the masks and found the
    # structures of each sample in its own pass)
    if lambda_ is None:
        lambda_ = RNG.beta(alpha, alpha)
    if index is None:
        index = torch.multinomial(mixup_probability(present), batch_size, replacement=True)
    index = torch.as_tensor(index, device=images.device)
    return _mixup_images(images, index, lambda_), index, lambda_


def mixup_data(images, alpha=0.2, device=None):
    """reference :45-52: a uniformly random partner"""
    lambda_ = RNG.beta(alpha, alpha)
    index = torch.randperm(images.shape[0], device=images.device)
    return _mixup_images(images, index, lambda_), index, lambda_
