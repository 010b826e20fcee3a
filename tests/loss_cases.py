"""Inputs of the loss / metric op tests (tests/test_gpu_loss_ops.py), generated from seeds on the CPU.  Nothing here needs a GPU:
tests/test_reference_ops.py asserts what the cases promise (exact logits, the four regions of the fused-head case, margins, label
coverage, the sum bound inside its cap), the GPU tests only consume them.

seg_loss_case: logits are randn * 2 rounded to multiples of 2^-10, so two logits of a voxel are equal or at least 2^-10 apart: the
float32 softmax of the kernel and the float64 softmax of the reference then order every pair of classes alike, and the expected
prediction needs no voxel left out.  A few rows hold exact ties of the top two / top three classes.
That draw (regime "initial") is the first step of training: a voxel's classes lie a few units around zero.  The other regimes are
the states a trained network is in, where softmax / log-sum-exp code loses digits, underflows or divides by a sum rounded to 1;
they keep the labels, the tie rows, PAD_LOGIT and the multiples of 2^-10 of the initial draw:
  * "confident": on about 97 % of the voxels the label's logit is the largest other logit of the row + 6 + U(0, 4) (per-voxel
    cross-entropy 1e-3 and below); on the rest another class gets that lead (confidently wrong, cross-entropy about 8).  Leads of 10
    and more on every voxel would not do: float32 cannot resolve log(1 + 1e-5), the float32 evaluation itself is then 6.8e-4 off and
    no bound derived from it is inside its cap.
  * "shifted+64", "shifted+250", "shifted-64": the initial draw plus a common offset on the columns < C (a head bias that has moved
    off zero); every logit stays an exact float32 number.
  * "saturated": as confident with leads of 30, 60, 90 and 120 + U(0, 4): exp(x - m) is below the float32 epsilon (9e-14), 9e-27
    (its square underflows), a float32 subnormal (8e-40) and 0 in float32; the label's probability is exactly 1.0 in float32 on the
    right voxels.  Rows 5 to 7 of every sample have a wrong class at 30000 (cross-entropy 3e4, every other probability exactly 0
    in float64 as well), row 8 the label's class at 30000 (cross-entropy exactly 0), and row 4 of sample 1 has all C logits at
    -30000 (a tie of everything: prediction 0, cross-entropy log C).
In the confident and the saturated regime every class of a sample's labels has at least one wrong voxel in that sample, whatever
the 3 % draw gave (at S = 100 and 13 classes that raises the wrong share to about 15 %): the focal sum of a class without one
consists of terms (1 - p_t)^2 (-log p_t) of the right voxels alone, which float32 evaluates with a relative error of 1e-3
(confident) or as exactly 0 against 1e-39 (saturated), and sum_bound's condition 0 < 16 x float32 < 1 / (4 S) would not hold.

HeadCase (ctseg_conv_logits_ce): operands with which every logit is an exact float32 number.  One unit is U = 2^-11.
  * activations: integers in [-4, 4] (exact in bf16 and fp16);
  * weights: integers in [-127, 127] times U, all 27 taps; biases: integers times U;
  * a logit is at most 16 * 27 * 4 * 127 units + bias + residual < 2^18 units (2^19 with the shifted biases), far below the 2^24
    units up to which every integer is a float32 number: every partial sum of the fp32 accumulators is exact in any order, and the
    float32 and the float64 convolution agree bit for bit.
Distinct logits differ by >= U = 4.9e-4 while the logits of a voxel spread over a few units of 1: a margin of U moves the fp32
softmax by 5e-4 relative, four orders above an ulp, so the expected prediction is the first maximal index of the float64 logits.

The regions, by construction (input channel 0 is the "background" channel, G1 and G2 two groups of input channels):
  * class 1 has the weights of class 0 except on G1, class 2 (C >= 3) those of class 0 except on G2; the three biases are equal.
    Where the G1 inputs of a voxel's 27 neighbours are zero, logits 0 and 1 are EQUAL; where G2 is zero as well, 0, 1 and 2 are:
    region (a), exact ties, expected prediction the first index.  The identity residual adds input channels 0, 1 / 2: zero there.
  * on the first channel of G1 the weights of class 1 differ from those of class 0 by +-1 or +-2 units in every tap.  A single
    input of 1 on that channel inside the zeroed band makes the 27 voxels around it differ by exactly those units between class 0
    and class 1: region (b), margins of U or 2 U < 1e-3, in both directions (the later index may be the larger one).
  * the block x < 5, y < 9, z < 9 of every sample holds 2 on channel 0 and zeros elsewhere; only class 0 has weights on channel 0,
    all positive: the first tile (4 x 8 x 8 voxels at the origin) predicts class 0 everywhere, its labels are 0: region (c).
  * everything else: region (d).
Two variants of it (``variant``), the state of a trained head:
  * "shifted": every bias raised by 64 (64 / U units);
  * "confident": a second constant block (y < 5, 10 <= z < 15, every x) outside the first tile, where channel 0 holds 12 and the
    other channels 0.  Class 0's channel-0 weights of 20 .. 60 units over 27 taps (18 or 12 at the faces of the volume) give it a
    lead of about 6 (4 and 3 there) on the voxels whose neighbours all lie in the block (y < 4, 11 <= z < 14); their label is 0 but
    for two voxels per sample.  No identity residual: it would add the 12 to logit 0, a lead of 18.  regions() counts them."""
import torch
import torch.nn.functional as F

from reference_ops import first_max_index

U = 2.0 ** -11


# ---- ctseg_seg_loss ---------------------------------------------------------------------------------------------------------------
SEG_SHAPES = [(2, 4), (8, 8), (10, 12), (10, 16), (12, 12), (13, 16), (16, 16)]       # (C, ld)
SEG_S = [100, 4221]
SEG_B = 3
PAD_LOGIT = 64.0          # what the columns >= C of a logits row hold: the kernels must not read them into any result
SEG_SHIFT = {"shifted+64": 64.0, "shifted+250": 250.0, "shifted-64": -64.0}
SEG_REGIMES = ["confident", "shifted+64", "shifted+250", "shifted-64", "saturated"]      # besides "initial"
SEG_REGIME_SHAPES = [(10, 12), (13, 16), (2, 4)]                                          # the (C, ld) the regimes are tested at
SAT_LEADS = (30.0, 60.0, 90.0, 120.0)
SAT_BIG = 30000.0
SAT_WRONG_ROWS, SAT_RIGHT_ROW, SAT_EQUAL_ROW = (5, 6, 7), 8, (1, 4)     # rows at SAT_BIG; (sample, row) of the all-equal row
_SEG = {}


def seg_class_weight(C):
    """class weights of mixed size, the first tiny as the project's own table has it"""
    w = 0.05 + torch.rand(C, generator=torch.Generator().manual_seed(900 + C))
    w[0] = 1e-3
    return w


def _lead_regime(x, labels, C, regime, tie_rows, seed):
    """the confident / saturated regime, written into x[..., :C] (see the module's docstring) -> mask (B, S) of the voxels on which
    the label's class leads"""
    B, S = labels.shape
    g = torch.Generator().manual_seed(seed)
    sat = regime == "saturated"
    free = torch.ones(S, dtype=torch.bool)
    free[[r for r, _ in tie_rows]] = False                  # the tie rows keep their ties
    if sat:
        free[4:9] = False
    wrong = torch.rand(B, S, generator=g) < 0.03
    for b in range(B):                                      # every class of the sample's labels: at least one wrong voxel
        for c in range(C):
            idx = ((labels[b] == c) & free).nonzero()[:, 0]
            if len(idx) and not bool(wrong[b, idx].any()):
                wrong[b, idx[len(idx) // 2]] = True
    leader = torch.where(wrong, (labels + 1 + torch.randint(0, C - 1, (B, S), generator=g)) % C, labels)
    lead = torch.round(torch.rand(B, S, generator=g) * 4.0 * 1024.0) / 1024.0
    lead += torch.tensor(SAT_LEADS)[torch.randint(0, len(SAT_LEADS), (B, S), generator=g)] if sat else 6.0
    xc = x[..., :C]
    others = xc.scatter(-1, leader[..., None], float("-inf")).max(-1).values
    new = xc.scatter(-1, leader[..., None], (others + lead)[..., None])
    xc[:, free] = new[:, free]
    right = ~wrong
    if sat:
        right[:, 4:9] = False                               # (row 4 of the other samples keeps the initial draw)
        for r in SAT_WRONG_ROWS + (SAT_RIGHT_ROW,):
            c = labels[:, r] if r == SAT_RIGHT_ROW else (labels[:, r] + 1) % C
            xc[torch.arange(B), r, c] = SAT_BIG
            right[:, r] = r == SAT_RIGHT_ROW
        xc[SAT_EQUAL_ROW[0], SAT_EQUAL_ROW[1]] = -SAT_BIG
        right[SAT_EQUAL_ROW[0], SAT_EQUAL_ROW[1]] = False
    right[:, ~free & (torch.arange(S) < 4)] = False
    return right


def seg_loss_case(C, ld, S, B=SEG_B, regime="initial"):
    """-> dict(x (B, S, ld) fp32, labels (B, S) uint8, coef (B, 1 + 3 C), cw (C,), tie_rows; regimes with a lead: label_leads (B, S)
    bool): computed once per key, never written to.  ``regime``: see the module's docstring; labels, coef and cw do not depend on it"""
    assert regime == "initial" or regime in SEG_REGIMES
    key = (C, ld, S, B) if regime == "initial" else (C, ld, S, B, regime)
    if key in _SEG:
        return _SEG[key]
    g = torch.Generator().manual_seed(1000 * C + 10 * ld + S % 7)
    x = torch.full((B, S, ld), PAD_LOGIT)
    x[..., :C] = torch.round(torch.randn(B, S, C, generator=g) * 2.0 * 1024.0) / 1024.0
    # exact ties at the top: rows 0 .. 3 of every sample, two or three classes, a later pair as well as one that includes class 0
    tie_rows = []
    for r, cls in enumerate(((0, 1), (C - 2, C - 1), (0, 1, 2), (1, C // 2, C - 1))):
        cls = sorted(set(c for c in cls if 0 <= c < C))
        if len(cls) < 2 or r >= S:
            continue
        for b in range(B):
            x[b, r, cls] = x[b, r, :C].max() + 0.5
        tie_rows.append((r, cls))
    labels = torch.randint(0, C, (B, S), generator=g)
    for b in range(1, B):                                   # every class, whatever the draw (sample 0: all but the last)
        n = min(C, S)
        labels[b, S - n:] = (torch.arange(n) + b) % C
    labels[0][labels[0] == C - 1] = 0                       # one class absent from one sample
    extra = {}
    if regime in SEG_SHIFT:
        x[..., :C] += SEG_SHIFT[regime]
    elif regime != "initial":
        extra["label_leads"] = _lead_regime(x, labels, C, regime, tie_rows, 77000 + 1000 * C + 10 * ld + S % 7 + (50 if regime == "saturated" else 0))
    coef = torch.zeros(B, 1 + 3 * C)
    coef[:, 0] = 1.0
    coef[:, 1:] = (torch.rand(B, 3 * C, generator=g) - 0.5) * 2e-3
    cw = torch.rand(C, generator=g) * 1e-3
    _SEG[key] = dict(x=x, labels=labels.to(torch.uint8), coef=coef, cw=cw, tie_rows=tie_rows, **extra)
    return _SEG[key]


def top_margin(x):
    """difference of the two largest entries along the last axis"""
    top = x.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


# ---- ctseg_conv_logits_ce ---------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(2, 7, 11, 13), (3, 4, 8, 16)]        # ragged tiles on every axis / whole tiles, three samples
_HEAD = {}


class HeadCase:
    """operands (x (N, cin, X, Y, Z), w (C, cin, 3, 3, 3), b (C,): float32 tensors holding the exact values), labels (N, X, Y, Z) and
    the masks of the regions; ``logits(dtype)``: conv + bias (+ the identity residual) in that precision"""

    def __init__(self, C, cin, shape, residual, seed=0, variant="base"):
        assert variant in ("base", "shifted", "confident")
        N, X, Y, Z = shape
        g = torch.Generator().manual_seed(7000 + 100 * C + cin + 7 * X + seed)
        self.C, self.cin, self.shape, self.residual, self.variant = C, cin, shape, residual, variant
        G1, G2 = [1, 2, 3], ([4, 5, 6] if cin == 16 else [4, 5])

        def ints(lo, hi, size):
            return torch.randint(lo, hi + 1, size, generator=g).float()
        # weights, in units
        w = ints(-40, 40, (C, cin, 3, 3, 3))
        w[:, 0] = 0.0
        w[0, 0] = ints(20, 60, (3, 3, 3))                   # the background channel: class 0 only, positive
        w[0, G1] = ints(-27, 27, (len(G1), 3, 3, 3))
        w[1] = w[0]
        w[1, 0] = 0.0
        small = ints(1, 2, (3, 3, 3)) * (ints(0, 1, (3, 3, 3)) * 2 - 1)                     # +-1, +-2
        large = ints(30, 100, (len(G1) - 1, 3, 3, 3)) * (ints(0, 1, (len(G1) - 1, 3, 3, 3)) * 2 - 1)
        w[1, G1] = w[0, G1] + torch.cat([small[None], large])
        if C >= 3:
            w[2] = w[0]
            w[2, 0] = 0.0
            w[2, G2] = w[0, G2] + ints(30, 80, (len(G2), 3, 3, 3)) * (ints(0, 1, (len(G2), 3, 3, 3)) * 2 - 1)
        assert float(w.abs().max()) <= 127
        b = ints(-1024, 1024, (C,))
        b[:min(C, 3)] = 2048.0                              # the classes that tie start ahead of the others (whose biases are <= 0.5)
        # activations
        x = ints(-4, 4, (N, cin, X, Y, Z))
        x[:, 0] = 0.0                                       # (channel 0 is zero outside the background block: class 0 alone reads it)
        xs, ys, zs = torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij")
        m1 = (ys >= Y - 3) | (zs >= Z - 3)                  # G1 zeroed: outputs two voxels deep tie in classes 0, 1
        m2 = zs >= Z - 3                                    # G2 zeroed as well: classes 0, 1, 2
        bg = (xs < 5) & (ys < 9) & (zs < 9)
        x[:, G1] = torch.where(m1, torch.zeros(()), x[:, G1])
        x[:, G2] = torch.where(m2, torch.zeros(()), x[:, G2])
        # single inputs of 1 on the first G1 channel, 3 apart, in the middle planes of the two zeroed bands
        imp = (xs % 3 == 1) & ~bg & (((ys == Y - 2) & (zs % 3 == 1) & (zs < Z - 4)) | ((zs == Z - 2) & (ys % 3 == 1) & (ys < Y - 4)))
        x[:, G1[0]] = torch.where(imp, torch.ones(()), x[:, G1[0]])
        x[:] = torch.where(bg, torch.zeros(()), x)
        x[:, 0] = torch.where(bg, torch.full((), 2.0), x[:, 0])
        block2 = (ys < 5) & (zs >= 10) & (zs < 15)          # the confident variant's block; its core sees no input outside it
        self.core2 = (ys < 4) & (zs >= 11) & (zs < 14)
        if variant == "confident":
            assert Z >= 19 and Y >= 8 and not residual and not bool((block2 & (bg | imp)).any())
            x[:] = torch.where(block2, torch.zeros(()), x)
            x[:, 0] = torch.where(block2, torch.full((), 12.0), x[:, 0])
        if variant == "shifted":
            b = b + 64.0 / U
        self.x, self.w, self.b = x, w * U, b * U
        assert Z >= 12 and Y >= 3
        labels = torch.randint(0, C, (N, X, Y, Z), generator=g)
        labels[:, :4, :8, :8] = 0                            # the first tile of every sample: background in truth
        for c in range(C):                                  # every class in every sample, outside the first tile (Z - 4 >= 8)
            labels[:, -1, Y - 1 - c // 4, Z - 1 - c % 4] = c
        if variant == "confident":                          # (the rows above lie at y >= Y - 4 >= 4: outside the core)
            labels[:, self.core2] = 0
            labels[:, 1, 1, 12] = 1                         # second to class 0 there, a lead of 6 against it
            labels[:, 2, 2, 11] = C - 1
        self.labels = labels.to(torch.uint8)
        self.masks = dict(m1=m1, m2=m2, bg=bg, imp=imp)
        self._logits = {}

    def logits(self, dtype):
        """(N, X, Y, Z, C): never written to"""
        if dtype not in self._logits:
            y = F.conv3d(self.x.to(dtype), self.w.to(dtype), self.b.to(dtype), padding=1)
            if self.residual:
                r = self.x[:, :self.C].to(dtype)
                y[:, :r.shape[1]] += r
            self._logits[dtype] = y.permute(0, 2, 3, 4, 1).contiguous()
        return self._logits[dtype]

    def regions(self):
        """voxel counts of the four regions, from the float64 logits: (a) exact ties of the top two / the top three, (b) top margins
        in (0, 1e-3), split by which index wins, (c) voxels of the first tile with label and prediction 0, (d) the rest; the
        confident variant: voxels of the second block's core that predict class 0 with a margin of 2.5 and more, by label 0 / other"""
        y = self.logits(torch.float64)
        top = y.topk(min(3, self.C), dim=-1).values
        margin = top[..., 0] - top[..., 1]
        tie2 = margin == 0
        tie3 = tie2 & (top[..., 0] == top[..., -1]) if self.C >= 3 else torch.zeros_like(tie2)
        near = (margin > 0) & (margin < 1e-3)
        pred = first_max_index(y)
        second = torch.where(y == top[..., 1:2], torch.arange(self.C), torch.full((), self.C)).min(-1).values
        tile0 = torch.zeros_like(tie2)
        tile0[:, :4, :8, :8] = True
        bgv = tile0 & (pred == 0) & (self.labels == 0)
        conf = self.core2 & (pred == 0) & (margin >= 2.5) if self.variant == "confident" else torch.zeros_like(tie2)
        return dict(confident=int((conf & (self.labels == 0)).sum()), confident_wrong=int((conf & (self.labels != 0)).sum()),
                    confident_lead=float(margin[conf].max()) if bool(conf.any()) else 0.0,
                    tie2=int((tie2 & ~tie3).sum()), tie3=int(tie3.sum()), near_first=int((near & (pred < second)).sum()),
                    near_later=int((near & (pred > second)).sum()), background=int(bgv.sum()), tile0=int(tile0.sum()),
                    ordinary=int((~tie2 & ~near & ~tile0).sum()), min_margin=float(margin[margin > 0].min()))


def head_case(C, cin, shape, residual, variant="base"):
    key = (C, cin, tuple(shape), bool(residual), variant)
    if key not in _HEAD:
        _HEAD[key] = HeadCase(C, cin, tuple(shape), bool(residual), variant=variant)
    return _HEAD[key]


# (C, input channels, identity residual, dlogits row width, storage type name, class-weighted, shape)
HEAD_CASES = [
    (10, 16, True, 12, "bf16", False, HEAD_SHAPES[0]),
    (10, 10, True, 12, "bf16", True, HEAD_SHAPES[0]),        # 10 of 16 gathered channels, 12-wide input rows
    (10, 16, False, 16, "bf16", False, HEAD_SHAPES[1]),
    (2, 16, False, 12, "bf16", True, HEAD_SHAPES[1]),
    (7, 10, False, 16, "bf16", False, HEAD_SHAPES[0]),
    (12, 16, True, 16, "bf16", True, HEAD_SHAPES[0]),
    (12, 10, False, 12, "bf16", False, HEAD_SHAPES[1]),
    (10, 16, True, 12, "fp16", False, HEAD_SHAPES[0]),
]
HEAD_IDS = [f"C{c[0]}-cin{c[1]}-{'res' if c[2] else 'nores'}-g{c[3]}-{c[4]}-{'weighted' if c[5] else 'plain'}-N{c[6][0]}" for c in HEAD_CASES]
# 9 tiles under CTSEG_MAX_WG = 8: eight workgroups walk the tiles in eight chunks of two, the chunks of workgroups 5, 6, 7 are empty
HEAD_EMPTY_WG_CASE = (10, 16, True, 12, "bf16", False, (3, 4, 8, 20))
# the same tuples + the variant: bf16 with 12- and 16-wide gradient rows and one fp16 run each.  Shifted: the smaller shape;
# confident: the second block needs z up to 15 outside the zeroed bands, the shape of HEAD_EMPTY_WG_CASE
HEAD_VARIANT_CASES = [
    (10, 16, True, 12, "bf16", False, HEAD_SHAPES[1], "shifted"),
    (10, 10, False, 16, "bf16", True, HEAD_SHAPES[1], "shifted"),
    (10, 16, True, 12, "fp16", False, HEAD_SHAPES[1], "shifted"),
    (10, 16, False, 12, "bf16", True, (3, 4, 8, 20), "confident"),
    (12, 10, False, 16, "bf16", False, (3, 4, 8, 20), "confident"),
    (10, 16, False, 12, "fp16", False, (3, 4, 8, 20), "confident"),
]
HEAD_VARIANT_IDS = [f"{c[7]}-C{c[0]}-cin{c[1]}-{'res' if c[2] else 'nores'}-g{c[3]}-{c[4]}-{'weighted' if c[5] else 'plain'}"
                    for c in HEAD_VARIANT_CASES]
HEAD_LOSS_SCALE = {"bf16": 1.0, "fp16": 2.0 ** 16}
_HEAD_REF = {}


def head_reference(C, cin, residual, weighted, shape, scale=1.0, variant="base"):
    """the float64 specification of ctseg_conv_logits_ce on head_case(...): per-sample (ce, weight) sums with their bound
    (helpers.sum_bound, rows = voxels of a sample), the gradient for a scale of coef[b] = scale (b + 1) / (N S) per sample in float64
    and in float32, predictions and Dice counts.  Computed once, never written to.  (``scale``: the loss scale of an fp16 run, so
    that no gradient element is a subnormal of the storage type.)"""
    from helpers import sum_bound
    from reference_ops import seg_loss_terms
    key = (C, cin, bool(residual), bool(weighted), tuple(shape), scale, variant)
    if key in _HEAD_REF:
        return _HEAD_REF[key]
    hc = head_case(C, cin, shape, residual, variant)
    N = shape[0]
    S = shape[1] * shape[2] * shape[3]
    cw = seg_class_weight(C) if weighted else None
    lab = hc.labels.reshape(N, S)
    y64, y32 = hc.logits(torch.float64).reshape(N, S, C), hc.logits(torch.float32).reshape(N, S, C)
    t64 = seg_loss_terms(y64, lab, C, None if cw is None else cw.double())
    t32 = seg_loss_terms(y32, lab, C, cw)
    rec64, rec32 = torch.stack([t64["ce"], t64["w"]], -1), torch.stack([t32["ce"], t32["w"]], -1)
    s64, norm, live, bound = sum_bound(f"head C={C} cin={cin} {shape} {variant}", rec64, rec32, (1,), rows=S)
    coef = scale * (torch.arange(N) + 1.0) / float(N * S)     # one scale per sample, all different
    oh = F.one_hot(lab.long(), C)
    g64 = coef.double()[:, None, None] * t64["w"][..., None] * (t64["p"] - oh.double())
    g32 = coef[:, None, None] * t32["w"][..., None] * (t32["p"] - oh.float())
    _HEAD_REF[key] = dict(case=hc, cw=cw, coef=coef, sums=s64, norm=norm, live=live, bound=bound, g64=g64, g32=g32,
                          pred=first_max_index(y64), pred_softmax=t64["pred"], cnt=t64["cnt"], y64=y64)
    return _HEAD_REF[key]


_SEG_REF = {}


def seg_stats_reference(C, ld, S, weighted, ce_only, B=SEG_B, regime="initial"):
    """float64 record sums (B, R) of seg_loss_case with their bound (helpers.sum_bound over the whole record, rows = S), predictions
    and Dice counts"""
    from helpers import sum_bound
    from reference_ops import seg_loss_records, seg_loss_terms
    key = (C, ld, S, bool(weighted), bool(ce_only), B, regime)
    if key in _SEG_REF:
        return _SEG_REF[key]
    case = seg_loss_case(C, ld, S, B, regime)
    cw = seg_class_weight(C) if weighted else None
    t64 = seg_loss_terms(case["x"].double(), case["labels"], C, None if cw is None else cw.double())
    t32 = seg_loss_terms(case["x"], case["labels"], C, cw)
    n = 2 if ce_only else 2 + 3 * C
    s64, norm, live, bound = sum_bound(f"seg_loss C={C} ld={ld} S={S} {regime}", seg_loss_records(t64)[..., :n], seg_loss_records(t32)[..., :n],
                                       (1,), rows=S)
    if ce_only:
        pad = torch.zeros(B, 3 * C, dtype=torch.float64)
        s64, norm, live = torch.cat([s64, pad], 1), torch.cat([norm, pad + 1], 1), torch.cat([live, pad.bool()], 1)
    _SEG_REF[key] = dict(case=case, cw=cw, sums=s64, norm=norm, live=live, bound=bound, pred=t64["pred"], pred32=t32["pred"],
                         cnt=t64["cnt"])
    return _SEG_REF[key]


# ---- ctseg_reduce_partials_f64 ------------------------------------------------------------------------------------------------------
def partials_case(P, R, B=2):
    """(B, P, R) float64 of mixed magnitude (2^-30 .. 2^30) and sign"""
    g = torch.Generator().manual_seed(40000 + 64 * P + R)
    mant = torch.randn(B, P, R, generator=g, dtype=torch.float64)
    expo = torch.randint(-30, 31, (B, P, R), generator=g).double()
    return mant * torch.pow(2.0, expo)


def partials_reference(part):
    """(B, P, R) float64 -> (exact sums over P (math.fsum) (B, R), sums of |entries| (B, R), bound on |error| / sum |entries|:
    16 x the worst error of numpy's own float64 pairwise sum of the same columns; 0 where numpy is exact everywhere, as for P = 1)"""
    import math
    import numpy as np
    cols = np.ascontiguousarray(part.numpy().transpose(0, 2, 1))          # (B, R, P): numpy adds a contiguous axis pairwise
    exact = np.array([[math.fsum(c) for c in row] for row in cols])
    mag = np.abs(cols).sum(-1)
    err = np.abs(cols.sum(-1) - exact) / mag
    return torch.from_numpy(exact), torch.from_numpy(mag), 16.0 * float(err.max())
