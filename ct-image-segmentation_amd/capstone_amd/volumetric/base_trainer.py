"""Drop-in for reference capstone/volumetric/base_trainer.py: ``BaseUNet3D`` with the same constructor,
``forward`` / ``training_step`` / ``validation_step`` / ``_shared_step`` / ``configure_optimizers`` /
``add_model_specific_args`` surface and hyper-parameter names, running on the MI355X engine.

Works as a ``pytorch_lightning.LightningModule`` when Lightning is importable and as a plain
``nn.Module`` otherwise (Lightning is not in this image); ``fit_step`` is the native step that
reproduces Lightning 1.0's per-batch order (zero_grad -> training_step -> backward -> [DDP mean of
gradients] -> Adam.step) without autograd, and is what bench.py times.
"""
import inspect
from typing import List

import torch

from .. import STRUCTURES, components, segloss, surface
from .. import _native as nat
from ..models import UNet
from ..models.losses import _as_cl
from ..training.module_base import _TrainerBase, _precision, pl
from ..training.utils import _squash_predictions  # noqa: F401  (same import the reference has)
from .losses import MultipleLossWrapper3D
from .metrics import DiceMetricWrapper3D, SurfaceDiceMetricWrapper3D, SurfaceDistanceMetricWrapper3D
from .utils import _squash_masks_3D

SEED = 12342


class BaseUNet3D(_TrainerBase):
    def __init__(self, filters: List = [16, 32, 64, 128, 256], use_res_units: bool = False, downsample: bool = False,
                 lr: float = 1e-3, loss_fx: list = ["CrossEntropy"], exclude_missing: bool = False, device_boundary: bool = False,
                 surface_metrics: bool = False, surface_percentile: float = 95.0, surface_spacing=None,
                 largest_component: bool = False, largest_component_connectivity=None, tta=None, val_inferer=None,
                 surface_dice=None, fill_holes: bool = False, fill_holes_connectivity=None, fill_holes_max_size: int = 0,
                 **kwargs) -> None:
        """``device_boundary``: opt in to the Boundary loss on volumes; the batch then carries the distance maps as its fourth
        element (``MiccaiDataset3D(dist_maps=True)``).  Without it a ``"Boundary"`` entry and a 4-tuple batch raise.
        ``surface_metrics``: ``validation_step`` also scores the batch with the percentile Hausdorff distance (``surface_percentile``,
        HD95 by default) and the average symmetric surface distance (``capstone_amd.surface``), in voxels of the label grid unless
        ``surface_spacing`` is given; the tables are kept per step, reduced by ``epoch_surface_metrics`` and logged by
        ``on_validation_epoch_end``.  Per rank: they are not gathered across data-parallel ranks.  Training steps never compute
        them.
        ``surface_spacing``: the voxel size (x, y, z) of the grid the network trains on, in millimetres, such as the cohort's mean
        after ``Resize3D``; one value for every sample, since the datasets carry no spacing.  The surface metrics are then physical
        distances and their log keys say so: ``"... HD95 mm (val)"``, ``"... ASSD mm (val)"``.
        ``largest_component``: ``validation_step`` also cleans the predicted label map, keeping the largest connected component of
        every class in every sample (``capstone_amd.components``; ``largest_component_connectivity``: 1, 2, 3 or ``None`` for the
        full 26 neighbours), and scores the cleaned map IN ADDITION to the raw one: its Dice under the prefix ``"val LCC"``
        (``"{structure} Dice (val LCC)"``, ``"Mean Dice Score (val LCC)"``) and, with ``surface_metrics``, its surface metrics, kept
        under ``"val LCC"`` and logged as ``"{structure} HD95 (val LCC)"`` and so on.  ``on_validation_epoch_end`` also logs
        ``"{structure} components (val)"``, the mean number of components of the raw prediction per class over the epoch's
        samples.  Per rank, and never in a training step, like the surface metrics.
        ``tta``: a ``volumetric.tta.TestTimeAugmenter3D`` whose ``size`` is the batch's grid.  ``validation_step`` then also predicts
        every sample once per view, merges the views (``predict_batch``) and scores the ensemble label map IN ADDITION to the plain
        one: its Dice under the prefix ``"val TTA"`` (``"{structure} Dice (val TTA)"``, ``"Mean Dice Score (val TTA)"``) and, with
        ``surface_metrics``, its surface metrics, kept under ``"val TTA"`` and logged as ``"{structure} HD95 (val TTA)"`` and so
        on.  ``predict_volume`` is the inference call.  Per rank, and never in a training step.
        ``val_inferer``: an ``inferers.SlidingWindowInferer``.  ``validation_step`` then gets its logits from
        ``val_inferer(images[i:i+1], self)`` per sample instead of one forward pass over the whole grid, so a model trained on
        patches (``MiccaiDataModule3D(patch_size=...)``) is validated on whole volumes; the losses and the Dice scores come from
        the same wrappers (``loss_func``, ``dice_score`` on the squashed logits) under the same keys.
        ``surface_dice``: a tolerance, or one per class, in voxels or, with ``surface_spacing``, in millimetres.
        ``validation_step`` then also scores the surface Dice at that tolerance (``capstone_amd.surface.surface_dice``) of the raw
        labels, of the cleaned ones with ``largest_component`` and of the merged ones with ``tta``; the tables are kept per step,
        reduced by ``epoch_surface_dice`` and logged by ``on_validation_epoch_end`` as ``"{structure} NSD (val)"`` and ``"Mean NSD
        (val)"``, and under ``(val LCC)`` / ``(val TTA)``.  Independent of ``surface_metrics``; per rank, and never in a training
        step.
        ``fill_holes``: ``validation_step`` also fills the enclosed holes of the predicted label map
        (``capstone_amd.components.fill_holes``; ``fill_holes_connectivity``: 1, 2, 3 or ``None`` for the full 26 neighbours;
        ``fill_holes_max_size``: the largest hole filled, 0 for no limit) and scores the filled map IN ADDITION: its Dice under the
        prefix ``"val filled"`` and, with ``surface_metrics`` / ``surface_dice``, its surface metrics and NSD under ``"(val
        filled)"``.  With ``largest_component`` it fills the keep-largest result, the order of a MONAI post-processing chain.
        ``on_validation_epoch_end`` also logs ``"{structure} holes (val)"``, the mean number of holes filled per class over the
        epoch's samples.  Per rank, and never in a training step."""
        super().__init__()
        assert isinstance(loss_fx, list), "This module expects a list of loss functions"
        loss_fx.sort()  # consistent order of loss functions (reference :35)
        self.save_hyperparameters(*self.HPARAMS, frame=inspect.currentframe())
        self._precision = _precision(kwargs)
        self.unet = self._construct_model()
        self.device_boundary = device_boundary      # (a switch of this port, not a reference hyperparameter: kept out of hparams)
        self.loss_func = MultipleLossWrapper3D(losses=loss_fx, exclude_missing=exclude_missing, device_boundary=device_boundary)
        self.dice_score = DiceMetricWrapper3D()
        self.surface_metrics = surface_metrics      # (as device_boundary: a switch of this port, kept out of hparams)
        self.surface_spacing = surface_spacing      # (kept out of hparams too)
        self.surface_score = SurfaceDistanceMetricWrapper3D(surface_percentile, surface_spacing) if surface_metrics else None
        self._surface_kept = {}
        self.largest_component = largest_component                  # (kept out of hparams, like the switches above)
        self.largest_component_connectivity = largest_component_connectivity
        self.lcc_dice_score = DiceMetricWrapper3D() if largest_component else None
        self._components_kept = []
        self.tta = tta                                              # (kept out of hparams too)
        self.tta_dice_score = DiceMetricWrapper3D() if tta is not None else None
        self.val_inferer = val_inferer                              # (kept out of hparams too)
        self.surface_dice = surface_dice                            # (kept out of hparams too)
        self.surface_dice_score = SurfaceDiceMetricWrapper3D(surface_dice, surface_spacing) if surface_dice is not None else None
        self._surface_dice_kept = {}
        self.fill_holes = fill_holes                                # (kept out of hparams too)
        self.fill_holes_connectivity = fill_holes_connectivity
        self.fill_holes_max_size = fill_holes_max_size
        self.filled_dice_score = DiceMetricWrapper3D() if fill_holes else None
        self._holes_kept = []

    def _construct_model(self):
        # reference :58-72 — in_channels=1, strides for a 5-entry filter list, num_res_units hard-wired to 2
        return UNet(dimensions=3, in_channels=1, out_channels=self._n_classes, channels=self.hparams.filters,
                    strides=[2, 2, 2, 2], num_res_units=2, precision=self._precision)

    def forward(self, x):
        return self.unet(x)

    def training_step(self, batch, batch_idx=0):
        """reference :80-82.  Only the loss leaves this function, so when the step is cross-entropy-only (the reference's working
        3-D default, :28) the loss runs fused with the logits convolution (bf16: ``ctseg_conv_logits_ce``; otherwise the one-pass
        cross-entropy over the materialised logits) and the returned scalar carries an autograd node (plan._StepLossFn) whose
        backward is the recorded backward program: ``training_step -> loss.backward() -> optimizer.step()`` then does the GPU
        work of ``fit_step``.  ``_shared_step`` (which must return the prediction) keeps the two-pass route;
        ``CTSEG_DROPIN_FUSED=0`` forces it here too."""
        if self._fused_training_ok(batch):
            return self._fused_training_step(batch)
        _, _, _, _, loss = self._shared_step(batch, is_training=True)
        return loss

    def _ce_only(self):
        names = list(self.loss_func.names)
        return len(names) == 1 and names[0] in ("CrossEntropy", "WeightedCrossEntropy")

    def _fused_training_ok(self, batch):
        import os
        return (torch.is_grad_enabled() and self._ce_only() and os.environ.get("CTSEG_DROPIN_FUSED", "1") != "0"
                and any(p.requires_grad for p in self.unet.parameters()))

    def _labels_then_forward(self, plan, images, masks, side_work=None, skip_head=False):
        """The plan's loss engine, found or built, with this batch's labels, and the forward pass: (loss engine, logits).  The
        label map is not needed before the loss: where the plan has a side stream the masks are squashed there — and
        ``side_work(loss engine)``, work that needs only the labels, runs behind them — while the forward pass starts."""
        le = getattr(plan, "_ctseg_loss", None)
        if le is None:
            le = plan._ctseg_loss = segloss.SegLossEngine(images.device, images.shape[0], plan.logits.S, self._n_classes)
        side = plan.side_stream()
        if side is None:
            lab_u8, _, hist = segloss.squash_masks(masks, self._n_classes, want_i64=False)
            le.set_labels(lab_u8, hist)
            return le, plan.forward(images, skip_head=skip_head)
        main = torch.cuda.current_stream(images.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            lab_u8, _, hist = segloss.squash_masks(masks, self._n_classes, want_i64=False)
            le.set_labels(lab_u8, hist)
            if side_work is not None:
                side_work(le)
        for t in (lab_u8, hist):
            t.record_stream(main)
        logits = plan.forward(images, skip_head=skip_head)
        main.wait_stream(side)
        return le, logits

    def _forward_and_ce(self, batch, keep_logits):
        """squash masks (side stream) -> forward -> cross-entropy + Dice counts + d loss / d logits for an upstream gradient of 1.
        Returns (engine, plan, loss engine, weighted)."""
        images, masks, mask_indicator, _ = self._split_batch(batch)     # (cross-entropy only: the maps are not read)
        eng = self.unet.engine()
        plan = eng.plan_for(images)
        weighted = self.loss_func.names[0] != "CrossEntropy"
        head_slots = 0 if keep_logits else plan.head_ce_slots(self._n_classes)
        # (side stream: also the loss tables that need only the label histogram)
        le, logits = self._labels_then_forward(plan, images, masks, side_work=lambda le: le.prepare_fused_ce(weighted=weighted),
                                               skip_head=head_slots > 0)
        dl = plan.dlogits
        if head_slots > 0:
            le.head_ce(plan._head_ce[2], head_slots, dl.ptr(), dl.ld, weighted=weighted)
        else:
            le.fused_ce(logits.ptr(), logits.ld, dl.ptr(), dl.ld, plan.dt, weighted=weighted)
        return eng, plan, le, weighted

    def _log_ce_summary(self, le, weighted, prefix="train"):
        """loss, mean Dice and the nine per-structure Dice scores of the fused pass: ONE launch, logged under the reference's names"""
        name = self.loss_func.names[0]
        loss, dm, dpc = le.ce_summary(weighted=weighted)
        if pl is None:
            self.log_packed(le.last_summary, self._summary_layout(name, prefix))
        else:   # Lightning logs scalars
            self._log_losses(prefix, {name: loss})
            self._log_dice(prefix, dm, dpc)
        return loss

    def _fused_training_step(self, batch):
        from ..plan import _StepLossFn
        import os
        nat.require_gpu(batch[0], "training_step")
        eng, plan, le, weighted = self._forward_and_ce(batch, keep_logits=os.environ.get("CTSEG_DROPIN_KEEP_LOGITS", "0") == "1")
        plan.dlogits_is_current = True
        loss = self._log_ce_summary(le, weighted)
        self._keep_dice_counts(le.cnt, "train")
        return _StepLossFn.apply(loss, eng, plan, self, *eng.store.params)

    def validation_step(self, batch, batch_idx=0):
        if self.val_inferer is not None:
            images, masks, prediction = self._inferer_step(batch)
        else:
            images, masks, _, prediction, _ = self._shared_step(batch, is_training=False)
        nsd = self.surface_dice_score is not None
        if not (self.surface_metrics or self.largest_component or self.tta is not None or nsd or self.fill_holes):
            return
        with torch.no_grad():
            if self.surface_metrics or self.largest_component or nsd or self.fill_holes:
                labels = _squash_predictions(prediction)
            if self.surface_metrics:
                self._score_surfaces(labels, masks, "val")
            if nsd:
                self._score_surface_dice(labels, masks, "val")
            if self.largest_component:
                kept = components.keep_largest_component(labels, self._n_classes,
                                                         connectivity=self.largest_component_connectivity)
                self._components_kept.append(kept.count)
                self._log_dice("val LCC", *self.lcc_dice_score(kept.labels, masks))
                if self.surface_metrics:
                    self._score_surfaces(kept.labels, masks, "val LCC")
                if nsd:
                    self._score_surface_dice(kept.labels, masks, "val LCC")
            if self.fill_holes:
                filled = components.fill_holes(kept.labels if self.largest_component else labels, self._n_classes,
                                               connectivity=self.fill_holes_connectivity, max_size=self.fill_holes_max_size)
                self._holes_kept.append(filled.holes)
                self._log_dice("val filled", *self.filled_dice_score(filled.labels, masks))
                if self.surface_metrics:
                    self._score_surfaces(filled.labels, masks, "val filled")
                if nsd:
                    self._score_surface_dice(filled.labels, masks, "val filled")
            if self.tta is not None:        # last: the views' forward passes overwrite the storage behind ``prediction``
                merged = self.tta.predict_batch(self, images).labels
                self._log_dice("val TTA", *self.tta_dice_score(merged, masks))
                if self.surface_metrics:
                    self._score_surfaces(merged, masks, "val TTA")
                if nsd:
                    self._score_surface_dice(merged, masks, "val TTA")

    def _inferer_step(self, batch):
        """``_shared_step`` for validation with ``val_inferer``: the logits of every sample come from the sliding-window inferer
        (whose result is a view of its own storage, so each is copied into the batch's block), then the same wrappers score them"""
        images, masks, mask_indicator, dist_maps = self._split_batch(batch)
        masks = _squash_masks_3D(masks, self._n_classes, self.device)
        mask_indicator = mask_indicator.type_as(images)
        with torch.no_grad():
            prediction = torch.cat([self.val_inferer(images[i:i + 1], self) for i in range(images.shape[0])])
            loss_dict = self.loss_func(input=prediction, target=masks, mask_indicator=mask_indicator, dist_maps=dist_maps)
            self._log_losses("val", loss_dict)
            dice_mean, dice_per_class = self.dice_score(_squash_predictions(prediction), masks)
            self._keep_dice_counts(self.dice_score.last_counts, "val")
            self._log_dice("val", dice_mean, dice_per_class)
        return images, masks, prediction

    def predict_volume(self, image, native: bool = True, want_probs: bool = False):
        """the inference call: a raw (D, H, W) scan on the device -> ``TestTimeAugmenter3D.predict``'s namespace, whose ``labels``
        are uint8 on the scan's own grid (``native``) or on the model's (H', W', D').  Needs ``tta``; one identity view
        (``TestTimeAugmenter3D([Augment3D.identity_params()])``) is the plain prediction carried back to the scan."""
        if self.tta is None:
            raise ValueError("predict_volume: construct the module with tta=TestTimeAugmenter3D(...)")
        return self.tta.predict(self, image, native=native, want_probs=want_probs)

    def _score_surfaces(self, labels, masks, prefix):
        self.surface_score(labels, masks)
        last = self.surface_score.last
        self._surface_kept.setdefault(prefix, []).append((last.hd, last.assd))

    def _score_surface_dice(self, labels, masks, prefix):
        self.surface_dice_score(labels, masks)
        self._surface_dice_kept.setdefault(prefix, []).append(self.surface_dice_score.last.nsd)

    def epoch_surface_dice(self, prefix="val", reset=True):
        """(NSD mean, NSD per class (9,)) over all samples scored since the last reset: per class the mean over the samples where
        the class is in the prediction or in the truth, then the mean over the classes that have a value; NaN where nothing has.
        None without ``surface_dice`` or when nothing was kept.  The values of this rank."""
        kept = self._surface_dice_kept.get(prefix)
        if self.surface_dice_score is None or not kept:
            return None
        if reset:
            self._surface_dice_kept[prefix] = []
        return surface.reduce_nan_mean(torch.cat(kept))

    def epoch_surface_metrics(self, prefix="val", reset=True):
        """(HD mean, HD per class (9,), ASSD mean, ASSD per class (9,)) over all samples scored since the last reset: per class the
        mean over the samples where the class is in both the prediction and the truth, then the mean over the classes that have a
        value; NaN where nothing has.  None with ``surface_metrics`` off or when nothing was kept.  The values of this rank."""
        kept = self._surface_kept.get(prefix)
        if not self.surface_metrics or not kept:
            return None
        hd, assd = (torch.cat([k[i] for k in kept]) for i in (0, 1))
        if reset:
            self._surface_kept[prefix] = []
        return surface.reduce_nan_mean(hd) + surface.reduce_nan_mean(assd)

    def on_validation_epoch_end(self, *args, **kwargs):
        """logs the epoch's surface metrics that have a value: "{structure} HD95 (val)", "Mean HD95 (val)", "{structure} ASSD
        (val)", "Mean ASSD (val)" (``HD`` and the percentile); with ``surface_spacing`` the unit follows the name, as in "{structure}
        HD95 mm (val)" and "Mean ASSD mm (val)", and the keys without it are not logged.  With ``largest_component`` the same
        keys under "(val LCC)" for the cleaned predictions, and "{structure} components (val)" besides.  With ``surface_dice``:
        "{structure} NSD (val)" and "Mean NSD (val)" for the classes that have a value, and the same under "(val LCC)" / "(val TTA)"
        (the tolerance's unit is that of ``surface_spacing``; the score has none).  With ``fill_holes`` the same keys under "(val
        filled)" for the filled predictions, and "{structure} holes (val)" besides"""
        if self.surface_metrics:
            for prefix, on in self._scored_prefixes():
                if on:
                    self._log_surface_epoch(prefix)
        if self.surface_dice_score is not None:
            for prefix, on in self._scored_prefixes():
                res = self.epoch_surface_dice(prefix) if on else None
                if res is not None:
                    self._log_per_structure("NSD", prefix, *res)
        if self.largest_component and self._components_kept:
            mean = torch.cat(self._components_kept).double().mean(dim=0)
            self._components_kept = []
            for structure, value in zip(STRUCTURES, mean):
                self.log(f"{structure} components (val)", value, on_step=False, on_epoch=True)
        if self.fill_holes and self._holes_kept:
            mean = torch.cat(self._holes_kept).double().mean(dim=0)
            self._holes_kept = []
            for structure, value in zip(STRUCTURES, mean):
                self.log(f"{structure} holes (val)", value, on_step=False, on_epoch=True)

    def _scored_prefixes(self):
        return (("val", True), ("val LCC", self.largest_component), ("val TTA", self.tta is not None),
                ("val filled", self.fill_holes))

    def _log_surface_epoch(self, prefix):
        res = self.epoch_surface_metrics(prefix)
        if res is None:
            return
        unit = "" if self.surface_spacing is None else " mm"
        hd = f"HD{self.surface_score.percentile:g}"
        for name, mean, per_class in ((hd + unit, res[0], res[1]), ("ASSD" + unit, res[2], res[3])):
            self._log_per_structure(name, prefix, mean, per_class)

    def _log_per_structure(self, name, prefix, mean, per_class):
        finite = torch.isfinite(per_class).tolist()
        for structure, value, ok in zip(STRUCTURES, per_class, finite):
            if ok:
                self.log(f"{structure} {name} ({prefix})", value, on_step=False, on_epoch=True)
        if any(finite):
            self.log(f"Mean {name} ({prefix})", mean, on_step=False, on_epoch=True)

    def _shared_step(self, batch, is_training: bool):
        images, masks, mask_indicator, dist_maps = self._split_batch(batch)
        masks = _squash_masks_3D(masks, self._n_classes, self.device)
        mask_indicator = mask_indicator.type_as(images)
        prefix = "train" if is_training else "val"
        prediction = self.forward(images)
        prediction._ctseg_plan = self.unet.engine().last_plan
        loss_dict = self.loss_func(input=prediction, target=masks, mask_indicator=mask_indicator, dist_maps=dist_maps)
        total_loss = torch.stack(list(loss_dict.values())).sum()
        self._log_losses(prefix, loss_dict)
        self._log_dice_scores(prediction, masks, mask_indicator, prefix)
        return images, masks, mask_indicator, prediction, total_loss

    def configure_optimizers(self):
        # reference :113-114 ``optim.Adam(self.parameters(), lr=self.hparams.lr)``: the same optimizer class and arguments; its
        # step() is one ctseg_adam_step launch over the flat parameter buffer (capstone_amd.optim.Adam IS a torch.optim.Adam)
        from ..optim import Adam
        return Adam(self.parameters(), lr=self.hparams.lr, unet=self.unet)

    def _log_dice_scores(self, prediction, masks, mask_indicator, prefix):
        # reference :116-132 clones 1 GB of logits, softmaxes, argmaxes and one-hots twice; the fused loss pass
        # already counted |pred==c & true==c|, |pred==c|, |true==c| with the same softmax->argmax tie rule.
        with torch.no_grad():
            eng = getattr(prediction._ctseg_plan, "_ctseg_loss", None)
            if all(n == "Boundary" for n in self.loss_func.names):      # no label loss ran: count now, on the labels the wrapper set
                ptr, ld, _keep = _as_cl(prediction)
                eng.stats(ptr, ld)
            dice_mean, dice_per_class = eng.dice_metric()
            self._keep_dice_counts(eng.cnt, prefix)
            self._log_dice(prefix, dice_mean, dice_per_class)

    # ---- native step: what Lightning's loop does per batch, without autograd -------------------------
    def fit_step(self, batch, betas=(0.9, 0.999), eps=1e-8, keep_logits=True):
        """keep_logits=False lets a cross-entropy-only step run the logits convolution with the loss fused into its epilogue
        (ctseg_conv_logits_ce): the fp32 logits are then never materialised and ``engine.logits_view()`` raises after the step;
        loss, Dice metric, gradients and the update are the same (gradient of the loss w.r.t. the logits bit-identical)."""
        images, masks, mask_indicator, dist_maps = self._split_batch(batch)
        nat.require_gpu(images, "fit_step")
        names = list(self.loss_func.names)
        ce_only = self._ce_only()
        assert "Boundary" not in names or dist_maps is not None, "Distance maps are required for using boundary loss"
        vals = None
        if ce_only:
            eng, plan, le, weighted = self._forward_and_ce(batch, keep_logits)
        else:
            eng = self.unet.engine()
            plan = eng.plan_for(images)
            le, logits = self._labels_then_forward(plan, images, masks)
            dl = plan.dlogits
            if "Boundary" in names:
                le.set_dist_maps(dist_maps)
            # (count_dice: the step's Dice counts come from the label pass, as in _SegLossPairFn)
            vals = le.loss_forward(logits.ptr(), logits.ld, names, self.loss_func.exclude_missing, mask_indicator.float(),
                                   count_dice=True)
            le.build_coef({n: 1.0 for n in names})
            le.grad_passes(logits.ptr(), logits.ld, names, dl.ptr(), dl.ld, plan.dt)
        book = {}

        def bookkeeping():     # scalar-sized work: queued behind the backward pass, beside the side stream's tail
            if ce_only:        # one launch for loss + Dice
                loss, dm, dpc = le.ce_summary(weighted=names[0] != "CrossEntropy")
                book["vals"], book["total"], book["dice"], book["packed"] = {names[0]: loss}, loss, (dm, dpc), le.last_summary
                return
            book["vals"] = vals
            book["total"] = torch.stack([vals[n] for n in names]).sum()
            book["dice"] = le.dice_metric()

        self._keep_dice_counts(le.cnt, "train")        # (queued before the next step overwrites the counters)

        reducer = eng.reducer
        if reducer is not None:
            plan.backward(reducer.hooks(plan), before_join=bookkeeping)
            scale = reducer.finish()
        else:
            eng.warn_if_unattached()
            plan.backward(before_join=bookkeeping)
            scale = 1.0
        eng.store.adam_step(self.hparams.lr, betas, eps, grad_scale=scale)
        plan.repack_after_update()
        vals, total = book["vals"], book["total"]
        dice_mean, dice_per_class = book["dice"]
        if "packed" in book and pl is None:
            self.log_packed(book["packed"], self._summary_layout(names[0], "train"))
        else:
            self._log_losses("train", vals)
            self._log_dice("train", dice_mean, dice_per_class, native=True)
        return total

    # ---- optimizer state of the native step, in torch.optim.Adam's own state_dict layout ------------------------------
    # The reference checkpoints through Lightning's ModelCheckpoint (volumetric/base_trainer.py:224-225), which stores
    # ``optimizer.state_dict()`` next to the module's ``state_dict``.  fit_step keeps Adam's moments in the flat store, outside any
    # torch optimizer, so the module exports / imports them in exactly that layout: a checkpoint written after native steps
    # resumes under ``configure_optimizers()``'s torch Adam and vice versa, and ``state_dict()`` keeps the reference's keys only.
    def optimizer_state_dict(self, betas=(0.9, 0.999), eps=1e-8):
        st = self.unet.engine().store
        params = list(self.parameters())
        state = {}
        if st is not None and st.step > 0:
            for i, p in enumerate(params):
                o, n = st.off(p), p.numel()
                state[i] = {"step": torch.tensor(float(st.step)), "exp_avg": st.adam_m[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": st.adam_v[o:o + n].view(p.shape).clone()}
        group = {"lr": self.hparams.lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0, "amsgrad": False,
                 "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        eng = self.unet.engine()
        st = eng.ensure(self.device)
        params = list(self.parameters())
        state = sd["state"]
        if not state:
            st.adam_m = st.adam_v = None
            st.step = 0
            return
        steps = {int(float(v["step"])) for v in state.values()}
        if len(state) != len(params) or len(steps) != 1:
            raise ValueError("optimizer state does not cover every parameter with one common step count")
        st.ensure_adam_state()
        with torch.no_grad():
            for i, p in enumerate(params):
                o, n = st.off(p), p.numel()
                e = state[i] if i in state else state[str(i)]
                st.adam_m[o:o + n].copy_(e["exp_avg"].reshape(-1))
                st.adam_v[o:o + n].copy_(e["exp_avg_sq"].reshape(-1))
        st.step = steps.pop()

    def on_save_checkpoint(self, checkpoint):
        """Lightning hook: the native step's Adam state rides in the checkpoint under its own key"""
        checkpoint["ctseg_native_adam"] = self.optimizer_state_dict()

    def on_load_checkpoint(self, checkpoint):
        if checkpoint.get("ctseg_native_adam", {}).get("state"):
            self.load_optimizer_state_dict(checkpoint["ctseg_native_adam"])

    def checkpoint(self):
        """what Lightning's ModelCheckpoint would write for this module (weights + optimizer state + hparams)"""
        ck = {"state_dict": self.state_dict(), "hyper_parameters": dict(self.hparams),
              "optimizer_states": [self.optimizer_state_dict()]}
        return ck

    def load_checkpoint(self, ck):
        self.load_state_dict(ck["state_dict"])
        if ck.get("optimizer_states"):
            self.load_optimizer_state_dict(ck["optimizer_states"][0])

    @staticmethod
    def add_model_specific_args(parent_parser):
        """Same flags and defaults as reference :134-182 (the ``--loss_fx`` default a string, as there)."""
        return _TrainerBase._model_args(parent_parser, batch_size=1, batch_size_help="Volumes per optimizer step",
                                        loss_fx="CrossEntropy")
