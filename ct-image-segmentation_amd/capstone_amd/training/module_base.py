"""What the drop-in trainer modules share (``BaseUNet3D``, ``BaseUNet2D`` and its ``MixupUNet2D``): the module base — a
``pytorch_lightning.LightningModule`` when Lightning is importable, a plain ``nn.Module`` with the slice of it the reference uses
otherwise (Lightning is not in this image) — the data-parallel surface, the ``precision`` flag, and ``_TrainerBase``: batch
splitting, hyper-parameter saving, the logging of losses and Dice scores under the reference's names, and the argparse flags.
"""
from argparse import ArgumentParser

import torch
import torch.nn as nn

from .. import STRUCTURES, segloss
from .. import _native as nat

try:  # pragma: no cover - Lightning is absent from the build image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    pl = None

    class _HParams(dict):
        __getattr__ = dict.__getitem__

    class _Base(nn.Module):
        """The slice of LightningModule the reference's module uses."""

        def __init__(self):
            super().__init__()
            self.hparams = _HParams()
            self.logged = {}
            self._epoch = {}

        def save_hyperparameters(self, *names, frame=None):
            """Lightning's signature: the arguments are read from ``frame``, the ``__init__`` frame, its ``**kwargs`` included"""
            frame_locals = frame.f_locals
            for n in names:
                self.hparams[n] = frame_locals.get(n, frame_locals.get("kwargs", {}).get(n))

        def log(self, name, value, on_step=False, on_epoch=True, **kw):
            """``logged[name]`` = the value of the last step; with ``on_epoch=True`` (what the reference passes everywhere,
            volumetric/base_trainer.py:106-109,125-131) the value also enters a running sum whose mean over the steps of the
            epoch is what Lightning 1.0 reports (``epoch_means``)."""
            v = value.detach() if torch.is_tensor(value) else value
            self.logged[name] = v
            if on_epoch:
                acc = self._epoch.get(name)
                if acc is None:
                    self._epoch[name] = [v.clone() if torch.is_tensor(v) else v, 1]
                else:
                    acc[0] = acc[0] + v
                    acc[1] += 1

        def log_packed(self, packed, layout):
            """several logged values that are slices of ONE small device tensor (the native step's loss / Dice summary):
            one accumulate for all of them instead of one tiny launch per name.  layout: [(name, index or slice)]"""
            packed = packed.detach()
            for name, sl in layout:
                self.logged[name] = packed[sl]
            key = ("packed",) + tuple(n for n, _ in layout)
            acc = self._epoch.get(key)
            if acc is None:
                self._epoch[key] = [packed.clone(), 1, layout]
            else:
                acc[0] += packed
                acc[1] += 1

        def epoch_means(self, reset=True):
            """{name: mean over the steps logged since the last reset} — Lightning's ``on_epoch=True`` reduction"""
            out = {}
            for k, acc in self._epoch.items():
                if isinstance(k, tuple):
                    mean = acc[0] / acc[1]
                    out.update({name: mean[sl] for name, sl in acc[2]})
                else:
                    out[k] = acc[0] / acc[1]
            if reset:
                self._epoch = {}
            return out

        @property
        def device(self):
            return next(self.parameters()).device


class _DataParallelSurface:
    """What the drop-in modules need so that the reference's ONLY way into multi-GPU training —
    ``Trainer.from_argparse_args(args)`` with ``--gpus N --distributed_backend ddp`` (capstone/volumetric/base_trainer.py:196,217;
    capstone/training/base_trainer.py: the same Trainer flags) — lands on the engine's own gradient exchange."""

    # ---- the gradient reducer lives on the engine (plan.Engine.reducer): one object for every route into the backward ----
    @property
    def reducer(self):
        return self.unet.engine().reducer

    @reducer.setter
    def reducer(self, value):
        self.unet.engine().reducer = value

    def configure_ddp(self, model, device_ids):
        """Lightning 1.0 hook (``LightningModule.configure_ddp(model, device_ids)``, called by the DDP accelerator once the process
        group exists and the module sits on its GPU; stock: ``LightningDistributedDataParallel(model, device_ids, ...)``).  Here:
        build the flat parameter store on the module's device, make the replicas identical and install the flat-buffer gradient
        exchange (``distributed.attach``), and return a pass-through wrapper with DDP's ``.module`` / per-mode ``forward``."""
        from .. import distributed as cdist
        dev = next(model.unet.parameters()).device
        model.unet.engine().ensure(dev)
        cdist.attach(model)
        return cdist.NativeDataParallel(model, device_ids)

    @property
    def _ddp_params_and_buffers_to_ignore(self):
        """torch's ``DistributedDataParallel.__init__`` probes the wrapped module for this attribute: the probe is the tripwire.
        A stock DDP wrap would train on rank-local gradients without any error (its reducer waits for AccumulateGrad hooks that
        never fire: the HIP kernels write the flat gradient buffer and the autograd nodes return None for the parameters)."""
        raise nat.NativeError(
            "torch.nn.parallel.DistributedDataParallel cannot wrap this module: its gradients are written into one flat buffer by "
            "the HIP backward kernels and averaged by capstone_amd.distributed.attach(module). Under Lightning the module's own "
            "configure_ddp() does that; in a hand-written loop call attach(module) after init_process_group and skip the DDP wrap.")

    # ---- Dice across ranks (the integer counts, one small all-gather at epoch end) -------------------------
    def _keep_dice_counts(self, cnt, prefix):
        """remember this step's per-sample integer Dice counts (B, 3, C) when the module is data-parallel (or on request,
        ``CTSEG_KEEP_DICE_COUNTS=1``): 30 int64 per sample and step"""
        import os
        red = self.unet.engine().reducer
        if (red is not None and red.world > 1) or os.environ.get("CTSEG_KEEP_DICE_COUNTS") == "1":
            self.__dict__.setdefault("_dice_counts", {}).setdefault(prefix, []).append(cnt.detach().clone())

    def epoch_dice_across_ranks(self, prefix="train", reset=True, group=None):
        """(mean Dice, per-class Dice (9,)) of the epoch as the reference computes it on the GLOBAL batch: per step, the
        per-sample counts of all ranks are one batch for ``compute_meandice`` + ``do_metric_reduction("mean_batch")``
        (capstone/models/temp.py:173-292, capstone/models/metrics.py:15-21); the epoch value is the mean over the steps
        (Lightning's ``on_epoch=True``).  The reference itself logs per rank (no ``sync_dist``, :106-109,125-131); this is the
        figure "Dice vs ref" is read from at N > 1.  One all-gather of (steps, B, 3, C) int64.  None when nothing was kept."""
        from .. import distributed as cdist
        kept = self.__dict__.get("_dice_counts", {}).get(prefix)
        if not kept:
            return None
        if len({tuple(k.shape) for k in kept}) == 1:
            cnt = list(cdist.gather_dice_counts(torch.stack(kept), group))  # ONE collective: (steps, world * B, 3, C)
        else:                                                               # a short last batch: one small collective per step
            cnt = [cdist.gather_dice_counts(k, group) for k in kept]
        if reset:
            self._dice_counts[prefix] = []
        per_step = [segloss.dice_metric(c) for c in cnt]
        mean = torch.stack([m for m, _ in per_step]).mean()
        per_class = torch.stack([p for _, p in per_step]).mean(dim=0)
        return mean, per_class


def _precision(kwargs):
    """Lightning's Trainer flag arrives through **vars(args) too.  ``--precision 16`` is IEEE half, as in the reference's stack
    (Lightning 1.0 native AMP): fp16 STORAGE for the inference passes (validation / test / sliding window), and bf16 storage
    for the training plans after a one-time RuntimeWarning (plan.Engine.train_dt: no fp16 backward kernels, no loss scaling;
    bf16 has fp32's range).  "bf16" by name uses bf16 throughout.  Nothing is remapped silently."""
    p = kwargs.get("precision", "fp32")
    if p in (16, "16", "fp16", "16-mixed", "16-true"):
        return "fp16"
    if p in ("bf16", "bf16-mixed", "bf16-true"):
        return "bf16"
    if p in (32, "32", "fp32", "32-true", None):
        return "fp32"
    raise ValueError(f"unsupported precision {p!r}")


class _TrainerBase(_DataParallelSurface, _Base):
    """What ``BaseUNet3D`` and ``BaseUNet2D`` do alike around their own steps."""

    # each ``__init__`` saves these with ``save_hyperparameters(*self.HPARAMS, frame=inspect.currentframe())``: the arguments are
    # read from that frame (Lightning needs its zero-argument ``super()`` there), ``batch_size`` and ``transform_degree`` out of
    # its ``**kwargs``
    HPARAMS = ("batch_size", "transform_degree", "filters", "use_res_units", "downsample", "lr", "loss_fx", "exclude_missing")

    @property
    def _n_classes(self):
        return len(STRUCTURES) + 1

    def _split_batch(self, batch):
        """(images, masks, mask_indicator, dist_maps or None), reference training/base_trainer.py:98-101; a fourth element
        needs ``device_boundary``"""
        images, masks, mask_indicator, *dist_maps = batch
        if dist_maps and not self.device_boundary:
            raise NotImplementedError("distance maps (Boundary loss) are outside the MI355X hot path unless device_boundary=True")
        return images, masks, mask_indicator, (dist_maps[0] if dist_maps else None)

    # ---- logging under the reference's names ----
    def _log_losses(self, prefix, loss_dict):
        for name, loss_value in loss_dict.items():
            self.log(f"{name} Loss ({prefix})", loss_value, on_step=False, on_epoch=True)

    def _log_dice(self, prefix, mean, per_class, native=False):
        """one entry per structure and then the mean, as the reference's ``_log_dice_scores`` does (volumetric/base_trainer.py:
        125-131).  ``native``: the order of ``fit_step``, which logs the mean first and, outside Lightning (whose ``log`` takes
        scalars only), the nine scores as one vector"""
        if native:
            self.log(f"Mean Dice Score ({prefix})", mean, on_step=False, on_epoch=True)
        if native and pl is None:
            self.log(f"Dice per class ({prefix})", per_class, on_step=False, on_epoch=True)
        else:
            for structure, score in zip(STRUCTURES, per_class):
                self.log(f"{structure} Dice ({prefix})", score, on_step=False, on_epoch=True)
        if not native:
            self.log(f"Mean Dice Score ({prefix})", mean, on_step=False, on_epoch=True)

    @staticmethod
    def _summary_layout(name, prefix):
        """``log_packed`` layout of ``SegLossEngine.ce_summary``'s tensor: [loss, mean Dice, Dice per class (9)]"""
        return ([(f"{name} Loss ({prefix})", 0), (f"Mean Dice Score ({prefix})", 1), (f"Dice per class ({prefix})", slice(2, None))] +
                [(f"{s_} Dice ({prefix})", 2 + i) for i, s_ in enumerate(STRUCTURES)])

    @staticmethod
    def _model_args(parent_parser, batch_size, batch_size_help, loss_fx):
        """the flags of the reference's two ``add_model_specific_args``, which differ in these defaults only"""
        parser = ArgumentParser(parents=[parent_parser], add_help=False)
        parser.add_argument("--batch_size", type=int, default=batch_size, help=batch_size_help)
        parser.add_argument("--transform_degree", type=int, default=0,
                            help="Augmentation preset index (0 = none)")
        parser.add_argument("--filters", nargs=5, type=int, default=[64, 128, 256, 512, 1024],
                            help="Channel widths of the five encoder levels")
        parser.add_argument("--use_res_units", action="store_true", default=False, help="Build the U-Net from residual units")
        parser.add_argument("--downsample", action="store_true", default=False,
                            help="Reduce a 3-channel input to 1 channel with a 1x1 convolution before the U-Net")
        parser.add_argument("--lr", type=float, default=1e-3, help="Adam step size")
        parser.add_argument("--loss_fx", nargs="+", type=str, default=loss_fx, help="One or more loss names, summed")
        parser.add_argument("--exclude_missing", action="store_true", default=False,
                            help="Weight per-class loss terms by annotation availability (AnatomyNet)")
        return parser
