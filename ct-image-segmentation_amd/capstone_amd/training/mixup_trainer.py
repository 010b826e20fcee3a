"""Drop-in surface of reference capstone/training/mixup_trainer.py:22-128 (``MixupUNet2D``) on the MI355X engine.

A ``BaseUNet2D`` with one residual subunit per level (reference :26-42) whose training step mixes every image with a partner
drawn by ``weighted_mixup`` and takes the loss against both targets (:52-92).  The reference calls ``loss_func`` twice on one
prediction; here both terms come from ``MultipleLossWrapper.forward_mixed``: one statistics pass and one gradient pass over the
logits for the two targets, and the Dice counts of both sides from the same statistics pass.  Validation and test steps are
the base class's.  Distance maps (Boundary loss) need ``device_boundary=True`` as in the base class; side B then reads
``dist_maps[shuffle_index]`` (:74) in place.
"""
import torch

from .. import segloss
from .base_trainer import BaseUNet2D
from .utils import _squash_masks, _squash_predictions, mixup_tensors, weighted_mixup


class MixupUNet2D(BaseUNet2D):
    RES_UNITS = 1       # 1 residual unit works better for mixup (reference :27)

    def validation_step(self, batch, batch_idx=0):
        """Mixup is used only while training and not during validation/testing."""
        super()._shared_step(batch, prefix="val")

    def test_step(self, batch, batch_idx=0):
        super()._shared_step(batch, prefix="test")

    def _shared_step(self, batch, prefix: str):
        assert prefix == "train", "Mixup can be used only while training"
        images, masks, mask_indicator, dist_maps = self._split_batch(batch)
        mixed_images, shuffle_index, lambda_ = weighted_mixup(images, masks, alpha=0.2, device=self.device)
        masks = _squash_masks(masks, self._n_classes, self.device)      # weighted_mixup left the label maps on ``masks``
        mask_indicator = mask_indicator.type_as(images)
        prediction = self.forward(mixed_images)
        prediction._ctseg_plan = self.unet.engine().last_plan if prediction.requires_grad else None
        loss_dict = self.loss_func.forward_mixed(input=prediction, target=masks, index=shuffle_index, lambda_=lambda_,
                                                 mask_indicator=mask_indicator, dist_maps=dist_maps)
        total_loss = torch.stack(list(loss_dict.values())).sum()
        self._log_losses(prefix, loss_dict)
        self._log_mixed_dice_scores(prediction, masks, mask_indicator, shuffle_index, lambda_, prefix)
        return images, masks, mask_indicator, prediction, total_loss

    def _log_mixed_dice_scores(self, prediction, masks, mask_indicator, shuffle_index, lambda_, prefix):
        """reference :94-115.  A mixed score is no function of pooled counts, so training steps keep no Dice counts."""
        with torch.no_grad():
            if self.hparams.exclude_missing:
                # reference :121-125: each side masks the prediction with its own indicator before the argmax
                sides = [self._masked_dice(prediction.detach(), t, ind) for t, ind in
                         ((masks, mask_indicator), (masks[shuffle_index], mask_indicator[shuffle_index]))]
            else:
                cnt = self.loss_func.last_mixed_counts
                sides = [segloss.dice_metric(cnt[:, s]) for s in (0, 1)]
            (mean_a, per_a), (mean_b, per_b) = sides
            self._log_dice(prefix, mixup_tensors(mean_a, mean_b, lambda_), mixup_tensors(per_a, per_b, lambda_))

    def _masked_dice(self, pred, target, indicator):
        pred = pred.clone()
        pred[:, 1:] = pred[:, 1:] * indicator[:, :, None, None]
        return self.dice_score(_squash_predictions(pred), target)
