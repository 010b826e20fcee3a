"""Loss / metric engine: host side of ctseg_squash_masks / ctseg_seg_loss / ctseg_dice_counts / ctseg_boundary_*.

One pass over the fp32 channels-last logits produces every sum the reference's losses and its Dice
metric need (capstone/models/losses.py, capstone/models/temp.py, capstone/models/metrics.py); the
per-(sample, class) closed forms are then a handful of ops on (B, 10) device tensors, and one more
pass writes d(loss)/d(logits).  CE-only (the reference's 3-D default, base_trainer.py:28) is a single
fused pass.  The Boundary loss (models/losses.py:127-157) has a statistics and a gradient pass of its own over the same logits
and the batch's distance maps; its gradient pass can add to the row the other losses' pass wrote.
"""
import contextlib
import math

import torch

from . import _native as nat
from ._native import BF16, F32
from .engine import SCRATCH, STATE, declare, plan_buf

N_CLASSES = 10
CLASS_WEIGHT = (1e-10, 0.007, 0.3296, 0.0046, 0.2619, 0.3035, 0.0068, 0.0065, 0.0374, 0.0426)  # models/losses.py:10-21
SMOOTH = 1e-5
LOSS_NAMES = ("CrossEntropy", "WeightedCrossEntropy", "Focal", "Dice", "GeneralizedDice")


def cl_logits(t):
    """(B,C,*sp) fp32 tensor -> (channels-last storage tensor [B,S,ld] sharing memory, ld) or None"""
    if t.dtype != torch.float32 or not t.is_cuda or t.ndim < 3:
        return None
    perm = (0,) + tuple(range(2, t.ndim)) + (1,)
    v = t.permute(perm)
    st, sh = v.stride(), v.shape
    if st[-1] != 1:
        return None
    ld = st[-2] if v.ndim > 2 else sh[-1]
    exp = ld
    for d in range(v.ndim - 2, -1, -1):   # every outer dim must be dense over ld-strided voxels
        if st[d] != exp and sh[d] != 1:
            return None
        exp *= sh[d]
    if ld % 4 or ld < sh[-1] or ld > 16 or t.data_ptr() % 16:
        return None
    return ld


def squash_masks(masks, n_classes=N_CLASSES, want_i64=True, want_present=False):
    """_squash_masks_3D / _squash_masks on device: (B,K,*sp) uint8 -> labels u8 (B,S), int64 (B,*sp), hist (B,K+1);
    want_present: a fourth result, present (B,K) int32 = any(masks[b,k] == 1), from the same read of the masks."""
    nat.require_gpu(masks, "_squash_masks")
    pre = getattr(masks, "_ctseg_labels", None)
    if pre is not None and not want_present and (masks.dtype == torch.uint8 or len(pre) == 3):
        # label maps squashed by the device input pipeline (volumetric/datasets.collate_3d), or raw masks that weighted_mixup
        # squashed already (it stashes the int64 map as a third entry): nothing left to do
        lab64 = pre[2] if len(pre) == 3 else (masks.long() if want_i64 else None)
        return pre[0], lab64, pre[1]
    if masks.dtype != torch.uint8:
        masks = masks.to(torch.uint8)
    masks = masks.contiguous()
    B, K = masks.shape[:2]
    S = masks[0, 0].numel()
    assert K == n_classes - 1
    lab = torch.empty((B, S), dtype=torch.uint8, device=masks.device)
    lab64 = torch.empty((B,) + tuple(masks.shape[2:]), dtype=torch.int64, device=masks.device) if want_i64 else None
    hist = torch.zeros((B, K + 1), dtype=torch.int64, device=masks.device)
    if want_present:
        present = torch.zeros((B, K), dtype=torch.int32, device=masks.device)
        nat.call("ctseg_squash_masks_present", masks.data_ptr(), B, K, S, lab.data_ptr(), nat.ptr(lab64), hist.data_ptr(),
                 present.data_ptr())
        return lab, lab64, hist, present
    nat.call("ctseg_squash_masks", masks.data_ptr(), B, K, S, lab.data_ptr(), nat.ptr(lab64), hist.data_ptr())
    return lab, lab64, hist


class SegLossEngine:
    def __init__(self, device, B, S, C=N_CLASSES):
        self.device, self.B, self.S, self.C = device, B, S, C
        self.P = max(1, min(2048, math.ceil(S / 2048)))
        self.R = 2 + 3 * C
        # BufferRole of every device buffer of the engine, by name: the tensors the caller hands in every step (labels, histogram,
        # maps) replace their entry (Plan.all_buffers reaches this registry through the plan the engine is cached on)
        self.buffers = {}
        self.part = plan_buf(self, "loss/part", (B, self.P, self.R), torch.float64)
        self.red = plan_buf(self, "loss/red", (B, self.R), torch.float64)
        self.red_w = plan_buf(self, "loss/red_w", (B, self.R), torch.float64)
        # (cnt and coef are accumulated into / partly written by the kernels: every pass that uses them re-zeroes them first, so
        # within a step they are written before they are read)
        self.cnt = plan_buf(self, "loss/cnt", (B, 3, C), torch.int64)
        self.coef = plan_buf(self, "loss/coef", (B, 1 + 3 * C), torch.float32)
        self.cw = declare(self, "loss/class weights", torch.tensor(CLASS_WEIGHT[:C], dtype=torch.float32, device=device), STATE,
                          "constant: the reference's class-weight table")
        self.cw_eff = plan_buf(self, "loss/cw_eff", C, torch.float32, fill=1.0)
        self.labels = self.hist = None
        self._ce_ready = None        # the `weighted` that prepare_fused_ce last set the tables up for, until a pass uses them
        self._part_head = None       # head_ce's partial records (B, slots, R)
        self.maps = None             # Boundary loss: fp32 distance maps (B, C-1, S) and, once they are set, its tables
        self._b_side = 0             # the side whose Boundary tables the closed forms below read and fill

    # ---- Boundary loss: maps, statistics, gradient (ctseg_boundary_stats / ctseg_boundary_grad) ----
    NS = 1                           # sides per sample; SegLossPairEngine has 2

    def _boundary_perm(self):
        return None

    def set_dist_maps(self, maps):
        """(B, C-1, *spatial) floating-point device tensor (no background plane); another float dtype is converted on the device"""
        nat.require_gpu(maps, "Boundary loss distance maps")
        if not maps.is_floating_point():
            raise TypeError(f"Boundary loss: distance maps must be floating point, got {maps.dtype}")
        if maps.ndim < 3 or tuple(maps.shape[:2]) != (self.B, self.C - 1) or maps[0, 0].numel() != self.S:
            raise ValueError(f"Boundary loss: distance maps of shape {tuple(maps.shape)}, expected ({self.B}, {self.C - 1}, ...) with "
                             f"{self.S} voxels per plane")
        self.maps = declare(self, "loss/distance maps", maps.detach().to(torch.float32).reshape(self.B, self.C - 1, self.S).contiguous(),
                            STATE, "input: the batch's distance maps, given by the caller")
        if getattr(self, "b_red", None) is None:
            self.b_part = plan_buf(self, "loss/b_part", (self.B, self.P, self.NS, self.C - 1), torch.float64)
            self.b_red = plan_buf(self, "loss/b_red", (self.B, self.NS, self.C - 1), torch.float64)
            self.bw = plan_buf(self, "loss/bw", (self.B, self.NS, self.C - 1), torch.float32)

    def boundary_stats(self, logits_ptr, ld):
        """b_red (B, NS, C-1) = sum over voxels of softmax(x)[c+1] * D_s[c]"""
        nat.call("ctseg_boundary_stats", logits_ptr, ld, self.maps.data_ptr(), nat.ptr(self._boundary_perm()), self.B, self.S, self.C,
                 self.b_part.data_ptr(), self.P)
        nat.call("ctseg_reduce_partials_f64", self.b_part.data_ptr(), self.B, self.P, self.NS * (self.C - 1), self.b_red.data_ptr())

    def boundary_grad(self, logits_ptr, ld, dl_ptr, g_ld, gdt, accumulate):
        """d(sum of bw-weighted table entries)/d(logits) from bw, which build_coef filled: stored, or added to the rows ``grad`` wrote"""
        nat.call("ctseg_boundary_grad", logits_ptr, ld, self.maps.data_ptr(), nat.ptr(self._boundary_perm()), self.B, self.S, self.C,
                 self.bw.data_ptr(), self.P, dl_ptr, g_ld, gdt, int(bool(accumulate)))

    # ---- targets ----
    def set_labels(self, labels_u8, hist):
        self.labels = declare(self, "loss/labels", labels_u8, STATE, "input: the batch's label map, given by the caller")
        self.hist = declare(self, "loss/hist", hist, STATE, "input: the batch's label histogram, given by the caller")

    def set_labels_from_i64(self, target):
        t = target.reshape(self.B, self.S)
        self.labels = declare(self, "loss/labels", t.to(torch.uint8).contiguous(), STATE, "input: the label map of the caller's target")
        self.hist = declare(self, "loss/hist", torch.zeros((self.B, self.C), dtype=torch.int64, device=self.device), STATE,
                            "input: the label histogram of the caller's target")
        self.hist.scatter_add_(1, t.long(), torch.ones_like(t, dtype=torch.int64))

    def set_target(self, target):
        """labels of a loss call's ``target``: the (labels u8, hist) the device squash left on it, or built from its int64 map"""
        stash = getattr(target, "_ctseg_labels", None)
        if stash is not None:
            self.set_labels(stash[0], stash[1])
        else:
            self.set_labels_from_i64(target)

    # ---- passes ----
    def _pass(self, logits_ptr, ld, cw, do_stats, do_grad, coef=None, dl_ptr=None, g_ld=0, gdt=F32, pred=None, part=None):
        """do_stats / do_grad: False, True, or 2 = cross-entropy-only fast path of the kernel"""
        nat.call("ctseg_seg_loss", logits_ptr, ld, self.labels.data_ptr(), self.B, self.S, self.C, nat.ptr(cw),
                 int(do_stats), nat.ptr(part if part is not None else self.part), self.P, self.cnt.data_ptr(),
                 int(do_grad), nat.ptr(coef), dl_ptr, g_ld, gdt, nat.ptr(pred))

    def stats(self, logits_ptr, ld, weighted_too=False):
        self.cnt.zero_()
        self._pass(logits_ptr, ld, None, True, False)
        nat.call("ctseg_reduce_partials_f64", self.part.data_ptr(), self.B, self.P, self.R, self.red.data_ptr())
        if weighted_too:
            keep = self.cnt.clone()
            self._pass(logits_ptr, ld, self.cw, True, False)
            nat.call("ctseg_reduce_partials_f64", self.part.data_ptr(), self.B, self.P, self.R, self.red_w.data_ptr())
            self.cnt.copy_(keep)

    def prepare_fused_ce(self, weighted=False):
        """the part of fused_ce that needs only the label histogram (counters zeroed, 1/denominator table): the training step
        issues it on the side stream right behind the mask squash, off the forward -> loss critical path"""
        self.cnt.zero_()
        w = self.cw.double() if weighted else torch.ones(self.C, dtype=torch.float64, device=self.device)
        denom = (self.hist.double() * w[None, :]).sum()
        self.coef.zero_()
        self.coef[:, 0] = (1.0 / denom).float()
        self._ce_ready = weighted

    def _take_ce_tables(self, weighted):
        """the tables of prepare_fused_ce for this ``weighted``, prepared now unless the side stream did; one pass uses them up"""
        if self._ce_ready is not weighted:
            self.prepare_fused_ce(weighted)
        self._ce_ready = None

    def fused_ce(self, logits_ptr, ld, dl_ptr, g_ld, gdt, weighted=False):
        """CrossEntropy (or WeightedCrossEntropy) alone: stats + gradient in ONE pass (upstream gradient 1)."""
        self._take_ce_tables(weighted)
        self._pass(logits_ptr, ld, self.cw if weighted else None, 2, 2, self.coef, dl_ptr, g_ld, gdt)
        nat.call("ctseg_reduce_partials_f64", self.part.data_ptr(), self.B, self.P, self.R,
                 (self.red_w if weighted else self.red).data_ptr())

    def head_ce(self, desc, slots, dl_ptr, g_ld, weighted=False):
        """the logits convolution and the cross-entropy (loss sums, Dice counts, d loss / d logits) in ONE launch: ``desc`` is the
        recorded descriptor of the plan's last forward op, ``slots`` = plan.head_ce_slots().  Same tables as fused_ce."""
        self._take_ce_tables(weighted)
        part = self._part_head
        if part is None or part.shape[1] != slots:
            part = self._part_head = plan_buf(self, "loss/head partial records", (self.B, slots, self.R), torch.float64)
        nat.call("ctseg_conv_logits_ce", desc, self.labels.data_ptr(), self.C, nat.ptr(self.cw if weighted else None),
                 self.coef.data_ptr(), self.coef.shape[1], dl_ptr, g_ld, part.data_ptr(), slots, self.R, self.cnt.data_ptr())
        nat.call("ctseg_reduce_partials_f64", part.data_ptr(), self.B, slots, self.R, (self.red_w if weighted else self.red).data_ptr())

    def ce_summary(self, weighted=False):
        """(loss, mean Dice, Dice per class) of the last fused_ce pass as views of one small tensor: one launch instead of the
        ~20 scalar-sized torch kernels of loss_values() + dice_metric()"""
        out = torch.empty(1 + self.C, dtype=torch.float32, device=self.device)
        nat.call("ctseg_loss_dice_summary", (self.red_w if weighted else self.red).data_ptr(), self.B, self.R, self.cnt.data_ptr(),
                 self.C, out.data_ptr())
        self.last_summary = declare(self, "loss/summary", out, SCRATCH)
        return out[0], out[1], out[2:]

    def predictions(self, logits_ptr, ld):
        pred = torch.empty((self.B, self.S), dtype=torch.uint8, device=self.device)
        if self.labels is None:
            self.labels = declare(self, "loss/labels", torch.zeros((self.B, self.S), dtype=torch.uint8, device=self.device), STATE,
                                  "input: a stand-in label map for a pass that only predicts")
        self._pass(logits_ptr, ld, None, False, False, pred=pred)
        return pred

    # ---- closed forms on (B, C) tables ----
    def _tables_for(self, names):
        """``_tables()`` when a loss other than Boundary asks for them (Boundary alone needs no labels)"""
        return self._tables() if any(n != "Boundary" for n in names) else (None,) * 4

    def _tables(self):
        C = self.C
        r = self.red
        return r[:, 2:2 + C], r[:, 2 + C:2 + 2 * C], r[:, 2 + 2 * C:2 + 3 * C], self.hist.double()

    def loss_values(self, names, exclude_missing=False, indicator=None):
        """dict name -> 0-dim fp32 tensor, plus per-loss (B,C) weights used for the gradient tables."""
        tables = self._tables_for(names)
        out, self._w = {}, {}
        for name in names:
            if name == "CrossEntropy":
                out[name] = (self.red[:, 0].sum() / self.red[:, 1].sum()).float()
            elif name == "WeightedCrossEntropy":
                out[name] = (self.red_w[:, 0].sum() / self.red_w[:, 1].sum()).float()
            else:       # a table loss (KeyError for an unknown name): its entries under the plain mean or the missing-mask weights
                f = self.loss_table(name, tables)
                wt = self._mask_weights(name, indicator, exclude_missing, f.shape[1])       # Boundary: the weights Dice gets
                out[name] = (f * wt).sum()
                # the two Dice tables leave the background out: their gradient weights get a zero column for it
                self._w[name] = torch.cat([torch.zeros_like(wt[:, :1]), wt], 1) if name in ("Dice", "GeneralizedDice") else wt
        return out

    def loss_table(self, name, tables=None):
        """the unreduced per-(sample, class) table of one loss after ``stats()`` — what the reference's wrapper returns with
        ``reduction="none"`` (capstone/models/losses.py:177-180 builds every entry that way under ``exclude_missing``):
        Dice / GeneralizedDice (B, C-1) (background excluded), Focal (B, C); Boundary (B, C-1) after ``boundary_stats()``.
        ``tables``: what ``_tables()`` returned, when the caller holds it already"""
        if name == "Boundary":
            return (self.b_red[:, self._b_side] / self.S).float()           # models/losses.py:146: the mean over (H, W)
        P, I, FO, Y = tables or self._tables()
        if name == "Dice":
            return (1.0 - (2.0 * I + SMOOTH) / (P + Y + SMOOTH))[:, 1:].float()
        if name == "GeneralizedDice":
            w = self._gdl_w(Y)
            return (1.0 - (2.0 * I * w + SMOOTH) / ((P + Y) * w + SMOOTH))[:, 1:].float()
        if name == "Focal":
            return (FO / self.S).float()
        raise KeyError(name)

    def _table_weight(self, name, g):
        """weight of table entry (b, c) in the scalar being differentiated: ``_w[name] * g`` for the reduced losses, or the
        upstream gradient itself when the caller took the unreduced table (``g`` is then (B, C-1) or (B, C))"""
        g = torch.as_tensor(g, dtype=torch.float64, device=self.device)
        if g.ndim == 2:
            if g.shape[1] == self.C - 1:
                g = torch.cat([torch.zeros_like(g[:, :1]), g], 1)
            return g
        return self._w[name].double() * g

    def _gdl_w(self, Y):
        y = Y.float()
        w = torch.reciprocal(y * y)                      # models/temp.py:90-94 (Weight.SQUARE)
        w = w[:, 1:]
        inf = torch.isinf(w)
        w = torch.where(inf, torch.zeros_like(w), w)
        w = torch.where(inf, w.max(dim=1, keepdim=True).values.expand_as(w), w)  # temp.py:150-153
        return torch.cat([torch.ones_like(y[:, :1]), w], 1).double()

    def _mask_weights(self, name, indicator, exclude_missing, ncol):
        """weight of table entry (b,c) in the scalar loss: plain mean, or models/losses.py:206-221"""
        B = self.B
        if not exclude_missing:
            return torch.full((B, ncol), 1.0 / (B * ncol), dtype=torch.float32, device=self.device)
        ind = indicator.float()
        if name == "Focal":
            bg = (ind.sum(dim=1, keepdim=True) == (self.C - 1)).float()
            ind = torch.cat([bg, ind], dim=1)
        w = 1.0 / ind.sum(dim=0)
        w = torch.where(torch.isinf(w).any(), torch.ones_like(w), w)
        w = w / w.sum()
        return w[None, :] * ind / B

    def build_coef(self, scales):
        """scales: dict name -> upstream gradient (0-dim tensor or float). Fills coef (B,1+3C) and cw_eff (C)."""
        B, C, S = self.B, self.C, self.S
        P, I, FO, Y = self._tables_for(scales)
        dev = self.device
        a = torch.zeros((B, C), dtype=torch.float64, device=dev)
        b = torch.zeros((B, C), dtype=torch.float64, device=dev)
        fcoef = torch.zeros((B, C), dtype=torch.float64, device=dev)
        cw = torch.zeros(C, dtype=torch.float64, device=dev)
        for name, g in scales.items():
            g = torch.as_tensor(g, dtype=torch.float64, device=dev)     # 0-dim, or the (B, C[-1]) gradient of an unreduced table
            if name == "CrossEntropy":
                cw = cw + g / float(B * S)
            elif name == "WeightedCrossEntropy":
                cw = cw + g * self.cw.double() / (self.hist.double() * self.cw.double()[None, :]).sum()
            elif name == "Dice":
                D = P + Y + SMOOTH
                wt = self._table_weight(name, g)
                a = a - 2.0 * wt / D
                b = b + wt * (2.0 * I + SMOOTH) / (D * D)
            elif name == "GeneralizedDice":
                w = self._gdl_w(Y)
                D = (P + Y) * w + SMOOTH
                wt = self._table_weight(name, g)
                a = a - 2.0 * w * wt / D
                b = b + wt * w * (2.0 * I * w + SMOOTH) / (D * D)
            elif name == "Focal":
                fcoef = fcoef + self._table_weight(name, g) / float(S)
            elif name == "Boundary":        # bw (B, NS, C-1): weight of the table entry, times the upstream gradient, times 1 / S
                wt = g if g.ndim == 2 else self._w[name].double() * g
                self.bw[:, self._b_side] = (wt / float(S)).float()
        self.cw_eff.copy_(cw.float())
        self.coef[:, 0] = 1.0
        self.coef[:, 1:1 + C] = a.float()
        self.coef[:, 1 + C:1 + 2 * C] = b.float()
        self.coef[:, 1 + 2 * C:] = fcoef.float()

    def grad(self, logits_ptr, ld, dl_ptr, g_ld, gdt):
        self._pass(logits_ptr, ld, self.cw_eff, False, True, self.coef, dl_ptr, g_ld, gdt)

    # ---- the loss sequence: stat_passes -> loss_values -> build_coef -> grad_passes ----
    _label_stats, _label_grad = stats, grad      # the label losses' pass of each half (SegLossPairEngine: its two-target pass)

    def stat_passes(self, logits_ptr, ld, names, count_dice=False):
        """the statistics passes ``names`` need.  ``count_dice``: the label pass runs for a Boundary-only recipe too (a training
        step takes its Dice counts from it)"""
        if count_dice or any(n != "Boundary" for n in names):
            self._label_stats(logits_ptr, ld, weighted_too="WeightedCrossEntropy" in names)
        if "Boundary" in names:
            self.boundary_stats(logits_ptr, ld)

    def loss_forward(self, logits_ptr, ld, names, exclude_missing=False, indicator=None, count_dice=False):
        """``stat_passes`` and then ``loss_values``"""
        self.stat_passes(logits_ptr, ld, names, count_dice)
        return self.loss_values(names, exclude_missing, indicator)

    def grad_passes(self, logits_ptr, ld, names, dl_ptr, g_ld, gdt):
        """one gradient row per voxel from the tables ``build_coef`` filled: the label losses' pass stores it and the Boundary
        pass adds to it, or the Boundary pass stores when it is the only name"""
        others = any(n != "Boundary" for n in names)
        if others:
            self._label_grad(logits_ptr, ld, dl_ptr, g_ld, gdt)
        if "Boundary" in names:
            self.boundary_grad(logits_ptr, ld, dl_ptr, g_ld, gdt, accumulate=others)

    def dice_metric(self):
        return dice_metric(self.cnt)


class SegLossPairEngine(SegLossEngine):
    """One prediction, two targets (the mixup step, capstone/training/mixup_trainer.py:63-81): side 0 of sample b is
    ``labels[b]``, side 1 is ``labels[perm[b]]``.  ctseg_seg_loss_pair takes one softmax per voxel for both sides' sums and
    writes the summed gradient once; the closed forms of the base class run once per side on views of the pair tables."""

    def __init__(self, device, B, S, C=N_CLASSES):
        super().__init__(device, B, S, C)
        if 2 * self.R > 64:
            raise nat.NativeError(f"pair loss pass: {C} classes need reduced records of {2 * self.R} > 64 doubles")
        self.part2 = plan_buf(self, "loss/part2", (B, self.P, 2, self.R), torch.float64)
        self.red2 = plan_buf(self, "loss/red2", (B, 2, self.R), torch.float64)
        self.red2_w = plan_buf(self, "loss/red2_w", (B, 2, self.R), torch.float64)
        self.cnt2 = plan_buf(self, "loss/cnt2", (B, 2, 3, C), torch.int64)          # (re-zeroed by every pass that uses it, as cnt)
        self.coef2 = plan_buf(self, "loss/coef2", (B, 2, 1 + 3 * C), torch.float32)
        self.cw2 = plan_buf(self, "loss/cw2", (2, C), torch.float32, fill=1.0)
        self.cw2_stats = declare(self, "loss/class weights of both sides", self.cw[None, :].repeat(2, 1), STATE,
                                 "constant: the class-weight table, one row per side")
        self.perm = self.hist2 = None

    NS = 2                           # Boundary loss: side 1 of sample b reads the maps of sample perm[b]

    def _boundary_perm(self):
        return self.perm

    def set_pair(self, labels_u8, hist, index):
        """index: (B,) integer device tensor; it never visits the host"""
        self.labels = declare(self, "loss/labels", labels_u8, STATE, "input: the batch's label map, given by the caller")
        self.perm = declare(self, "loss/perm", index.to(torch.int32).contiguous(), STATE, "input: the mixup partner of every sample")
        self.hist2 = (declare(self, "loss/hist", hist, STATE, "input: the batch's label histogram, given by the caller"),
                      declare(self, "loss/hist of the partners", hist[index.long()], STATE, "input: the partners' label histograms"))

    @contextlib.contextmanager
    def side(self, s):
        """the base class's tables (red, red_w, hist, cnt, coef, cw_eff) stand for side ``s`` inside the block"""
        keep = (self.red, self.red_w, self.hist, self.cnt, self.coef, self.cw_eff, self._b_side)
        self.red, self.red_w, self.hist = self.red2[:, s], self.red2_w[:, s], self.hist2[s]
        self.cnt, self.coef, self.cw_eff, self._b_side = self.cnt2[:, s], self.coef2[:, s], self.cw2[s], s
        try:
            yield self
        finally:
            self.red, self.red_w, self.hist, self.cnt, self.coef, self.cw_eff, self._b_side = keep

    def _pass_pair(self, logits_ptr, ld, cw, do_grad, dl_ptr=None, g_ld=0, gdt=F32):
        nat.call("ctseg_seg_loss_pair", logits_ptr, ld, self.labels.data_ptr(), self.perm.data_ptr(), self.B, self.S, self.C,
                 nat.ptr(cw), int(do_grad), self.part2.data_ptr(), self.P, self.cnt2.data_ptr(), self.coef2.data_ptr(), dl_ptr,
                 g_ld, gdt)

    def stats_pair(self, logits_ptr, ld, weighted_too=False):
        self.cnt2.zero_()
        self._pass_pair(logits_ptr, ld, None, False)
        nat.call("ctseg_reduce_partials_f64", self.part2.data_ptr(), self.B, self.P, 2 * self.R, self.red2.data_ptr())
        if weighted_too:
            keep = self.cnt2.clone()
            self._pass_pair(logits_ptr, ld, self.cw2_stats, False)
            nat.call("ctseg_reduce_partials_f64", self.part2.data_ptr(), self.B, self.P, 2 * self.R, self.red2_w.data_ptr())
            self.cnt2.copy_(keep)

    def grad_pair(self, logits_ptr, ld, dl_ptr, g_ld, gdt):
        """d(sum over both sides)/d(logits) from coef2 / cw2, which build_coef filled inside ``side(0)`` and ``side(1)``"""
        self._pass_pair(logits_ptr, ld, self.cw2, True, dl_ptr, g_ld, gdt)

    _label_stats, _label_grad = stats_pair, grad_pair


def dice_metric(cnt):
    """(mean Dice, Dice per class (C-1,)) from exact integer counts (B, 3, C) = |pred == c & true == c|, |pred == c|, |true == c|
    (models/metrics.py:15-21, temp.py:173-292)"""
    inter, pred, true = (cnt[:, i, 1:].float() for i in range(3))
    nan = torch.full_like(inter, float("nan"))
    score = torch.where(true > 0, 2.0 * inter / (true + pred), nan)      # (B, 9), NaN where truth empty
    ok = (~torch.isnan(score)).float()
    score = torch.nan_to_num(score, nan=0.0)
    n_ok = ok.sum(dim=0)
    per_class = torch.where(n_ok > 0, score.sum(dim=0) / n_ok, torch.zeros_like(n_ok))   # "mean_batch"
    return per_class.mean(), per_class


def dice_counts(pred_u8, true_u8, C=N_CLASSES):
    B, S = pred_u8.shape
    cnt = torch.zeros((B, 3, C), dtype=torch.int64, device=pred_u8.device)
    nat.call("ctseg_dice_counts", pred_u8.data_ptr(), true_u8.data_ptr(), B, S, C, cnt.data_ptr())
    return cnt
