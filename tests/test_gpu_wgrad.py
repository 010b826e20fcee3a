"""GPU: the weight-gradient passes (ctseg_conv_wgrad, every kernel family) and the slab reduces at op level.

Every case names the instantiation it is written for; helpers.WgradPassDriver asserts ctseg_wgrad_pass_name of the recorded
descriptor before anything runs.

Oracle A (default): x and dy are integers in [-4, 4] (seeded, no symmetry).  Every product is an integer of magnitude <= 16 and a
sum of N * rows of them stays below 2^24 (asserted), so the gradient is exact in fp32 in any summation order: the kernel must equal
the float64 autograd reference (conv_wgrad of reference_ops.py) bit for bit (torch.equal), bias gradient included.  Every such case runs over slabs poisoned with
NaN, checks that nothing of the flat gradient outside the layer's views changed, and replays the recorded program with other
operands over its own stale slabs: `ws` need not be initialised (include/ctseg_hip.h).

Oracle B (one case per family): normal-valued operands rounded to the storage type, float64 autograd reference, error per entry
|got - ref| / S with S the float64 gradient of (|x|, |dy|); bound 16 x the same error of torch's plain float32 evaluation, measured
in the test, which asserts 0 < bound < 1 / (4 * N * rows); the weight and the bias gradient each have their own bound.  Every test
prints its figures and bounds before asserting.  float32 adds a few hundred bf16 values without any rounding often enough: where
torch's float32 column sums of dy are all exact (the 16 lower columns x 192 rows of the "stem 32 dyn" case always are) the measured
bias bound would be 0, and the kernel, which adds the same values in another order, is allowed ONE float32 rounding of a partial sum
instead, 2^-24 of sum |dy|.  The weight bound is never replaced.  (The element-wise case is 33 x 45 pixels for the same reason.)
Measured on an MI355X (weight / bias error, bound of the case in brackets):
  x-column head 12/12  2.3e-08 / 1.0e-09 (3.3e-07);  on load, N = 2 / 16: 2.1e-08 / 1.7e-08 (4.0e-07 / 2.9e-07)
  halo 64x64 / 32x64 / 64x32  3.3e-08 / 3.1e-08 / 3.0e-08 (9.0e-07 / 5.4e-07 / 5.0e-07), bias <= 3.9e-09
  up 12                4.8e-08 (4.7e-07)
  stem 32              3.2e-08 / 6.8e-09 (5.2e-07);  dyn 32 / 64 columns, N = 2 / 8: 2.0e-08 .. 6.5e-08 (3.3e-07 .. 7.8e-07)
  ring 512x64 / 256x128 / 256x256  3.5e-08 / 6.8e-08 / 7.4e-08 (2.7e-06 / 1.9e-06 / 2.4e-06), bias <= 5.9e-09
  generic 64 bf16 / fp32  3.4e-08 / 9.7e-08 (2.4e-06 / 4.2e-06), bias 2.6e-09 / 3.5e-08;  element-wise 2.9e-08 (4.2e-07)
No family needed the L * 2^-24 fallback bound.

Shapes that differ from the plain list, and why:
  * 32 -> 24 "halo 64x64" takes dY rows 32 wide: with the default 24-wide rows wgrad_halo_eligible turns the layer down (a dY row
    narrower than its two 16-channel planes) and the generic kernel runs; that case is kept by its name "generic 32";
  * 96 -> 160 in bf16 is the ring's ("ring 256x256", a case of its own); the bf16 "generic 128" case is 24 -> 160;
  * the flat-grid cases use (2, 8, 14, 14): GemmLayer._wgrad_splits never cuts below 512 rows per split, so four splits need more
    than 1536 rows;
  * an empty last split cannot come out of GemmLayer._wgrad_splits (at least 512 rows per split, 32-row rounding); the C ABI takes
    any split count, so the case forces splits = 12 over 585 rows (64-row ranges: range 9 holds 9 rows, ranges 10 and 11 none).

The 2-D U-Net at its real widths (UNET2D_CASES, UNET2D_FUSED: every weight-gradient row of tests/unet2d_passes.py): up to 1536 columns
(six column blocks of "ring 256x256"), K up to 9 * 1024, the fused down units' single pass held to the gradients of its two layers.
Oracle A on every row; Oracle B on one row per distinct pass name, the long-K ConvTranspose2d 1536 -> 256 and 1024 -> 1024 and two
fused units (each half with its own layer's bound).  Measured on an MI355X (weight / bias error, bounds in brackets):
  generic 16 (10 -> 10)  3.5e-08 (6.0e-07), bias 0 (torch's float32 column sums came out exact: the one-rounding bound 6.0e-08 applied)
  generic 128 (convT 128 -> 10)  5.1e-08 / 1.3e-09 (2.7e-06 / 2.0e-08);  ring 512x64 (64 -> 64)  5.6e-08 / 2.3e-09 (1.6e-06 / 3.6e-08)
  ring 256x128 (128 -> 128)  6.3e-08 / 1.2e-09 (2.4e-06 / 7.9e-08)
  ring 256x256: convT 1536 -> 256  7.7e-08 / 2.5e-09 (3.1e-06 / 7.8e-08);  1024 -> 1024  1.4e-07 / 6.9e-09 (3.1e-06 / 1.6e-07)
  fused 1 -> 2 x 64 (generic 128 element-wise), residual / unit0:  2.9e-08 / 3.2e-08 (7.3e-07 / 5.7e-07), bias <= 3.0e-09 (>= 2.3e-08)
  fused 256 -> 2 x 512 (ring 256x256), residual / unit0:  6.7e-08 / 7.6e-08 (3.0e-06 / 2.9e-06), bias <= 1.2e-08 (>= 1.1e-07)
  caps 1 / (4 * N * rows): 5.1e-04 .. 1.0e-03, far above every bound

Not covered, with the reason the library gives:
  * "head 12/16" and "head 16/12" (conv_wgrad_head_kernel, the head kernel without the x-column reuse): wgrad_halo_variant picks
    that kernel only for taps out of canonical order, which GemmLayer never records; "head 16/16" and "head 12/12" run below from
    a recorded descriptor with its taps reversed, the mixed widths are the same staging template with one operand of each and are
    named on the CPU from a hand-made descriptor (tests/test_abi_exports.py);
  * "halo 32x32": 16 -> <= 16 channels with rows neither 12 nor 16 wide (g_ld = 24, ...), which no activation of the host mirror
    has; named on the CPU likewise;
  * "generic 32/64 element-wise": named on the CPU; the element-wise staging code is the same template branch as the 16-column
    tile's, which the three first-layer cases run, and the 128-column tile's, which the 2-D U-Net's fused first layer runs;
  * in_mean_rstd on anything but the x-column head kernel and dyn_* on anything but the stem kernel: the launch refuses
    ("... is not implemented for this pass"), asserted below;
  * CTSEG_WGRAD_ADDR64: its own bit-equality test (test_gpu_round3.py).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd._native import BF16, F32  # noqa: E402
from capstone_amd.engine import Act, new_act  # noqa: E402
from helpers import CAP_IDS, CAPS, GRAD_SENTINEL, WgradPassDriver, cap_env, norm_for, to_cl  # noqa: E402
from reference_ops import conv_module, conv_out_shape, conv_wgrad, norm_prelu_dy  # noqa: E402

DEV = "cuda:0"


def _ints(shape, gen):
    return torch.randint(-4, 5, shape, generator=gen).float()


class _Case:
    """kind: conv / conv_s2 / convT (3-D), conv2d / conv2d_s2 / convT2d (shape (N, X, Y, 1)); op, dims: the same for reference_ops"""

    def __init__(self, name, kind, cin, cout, shape, dt=BF16, k=3, cg=None, x_ld=None, dy_ld=None, env=None, splits=None, target=None):
        self.name, self.kind, self.cin, self.cout, self.shape, self.dt, self.k = name, kind, cin, cout, shape, dt, k
        self.op, self.dims = kind.replace("2d", ""), 2 if "2d" in kind else 3
        self.cg, self.x_ld, self.dy_ld, self.env, self.splits, self.target = cg, x_ld, dy_ld, env or {}, splits, target

    @property
    def seed(self):
        """of the layer alone (kind, channels, shape): cases that differ in row widths, caps or switches get the same operands"""
        return len(self.kind) + 1009 * self.cin + 1000003 * self.cout + sum(v * 31 ** i for i, v in enumerate(self.shape))

    @property
    def bias_done(self):
        return self.kind == "convT" and self.dy_ld == 12

    @property
    def id(self):
        e = "".join(f" {k[6:]}={v}" for k, v in self.env.items())
        w = "".join(f" {n}{v}" for n, v in (("x", self.x_ld), ("dy", self.dy_ld), ("splits", self.splits), ("wgs", self.target)) if v)
        return f"{self.name} | {self.kind} {self.cin}->{self.cout} {self.shape}{' fp32' if self.dt == F32 else ''}{w}{e}".replace(" ", "_")

    def sizes(self):
        N, sp = self.shape[0], tuple(self.shape[1:1 + self.dims])
        xs = (N, self.cin) + sp
        ys = (N, self.cout) + conv_out_shape(self.op, self.k, sp)
        mod_w = ((self.cin, self.cout) + (3,) * self.dims) if self.op == "convT" else ((self.cout, self.cin) + (self.k,) * self.dims)
        return xs, ys, mod_w

    def setenv(self, monkeypatch, cap=None):
        for k in ("CTSEG_MAX_WG", "CTSEG_NO_WGRAD_UP", "CTSEG_WGRAD_RING", "CTSEG_WGRAD_TARGET_WGS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        if self.target:
            monkeypatch.setenv("CTSEG_WGRAD_TARGET_WGS", str(self.target))
        cap_env(monkeypatch, cap)

    def driver(self):
        torch.manual_seed(1)
        return WgradPassDriver(conv_module(self.op, self.cin, self.cout, self.k, self.dims), self.dt, DEV, cg=self.cg)

    def acts(self, drv, x, dy):
        # a transposed layer's 12 / 16 wide rows are those of dOut (the gathered operand)
        e = nat.epc(self.dt)
        x_ld = self.x_ld if self.x_ld else (self.cin if self.cg is None and self.cin % e else None)    # (as run_conv_module lays x out)
        return drv.act(x, ld=x_ld), drv.act(dy, ld=self.dy_ld)


def _exact_run(case, monkeypatch, cap=None):
    """Oracle A over poisoned slabs, then a replay with other operands over the stale ones -> (gw, gb) of the first run"""
    case.setenv(monkeypatch, cap)
    xs, ys, wshape = case.sizes()
    rows = 1
    for v in (xs if case.kind.startswith("convT") else ys)[2:]:
        rows *= v
    assert 16 * xs[0] * rows < 2 ** 24, "the integer oracle is exact only below 2^24"
    gen = torch.Generator().manual_seed(case.seed)
    drv = case.driver()
    first = None
    for rnd in range(2):
        x, dy = _ints(xs, gen), _ints(ys, gen)
        rw, rb = conv_wgrad(case.op, case.k, x, dy, wshape, torch.float64)
        assert bool((rw.abs().flatten(1).sum(1) > 0).all()) and bool((rw.abs().transpose(0, 1).flatten(1).sum(1) > 0).all()), \
            "an all-zero channel slice of the reference: a skipped column block would pass"
        assert bool((rb != 0).any())
        if rnd == 0:
            xa, ga = case.acts(drv, x, dy)
            d = drv.record(case.name, xa, ga, splits=case.splits, bias_done=case.bias_done)
            gw, gb, _, flat = drv.go(poison=float("nan"))
        else:       # the same recorded program, new operands in the same tensors, its own stale slabs
            xa.t[..., :xs[1]].copy_((x if x.ndim == 5 else x.unsqueeze(-1)).permute(0, 2, 3, 4, 1))
            ga.t[..., :ys[1]].copy_((dy if dy.ndim == 5 else dy.unsqueeze(-1)).permute(0, 2, 3, 4, 1))
            gw, gb, _, flat = drv.go()
        tag = "poisoned slabs" if rnd == 0 else "replay over stale slabs"
        assert torch.equal(gw, rw.float()), (case.id, tag, "weight gradient", int((gw != rw.float()).sum()), float((gw - rw.float()).abs().max()))
        # (bias_done: 12-wide dOut has no column-sum pass; in the network that bias gradient comes out of the norm's backward)
        assert torch.equal(gb, torch.full_like(gb, GRAD_SENTINEL) if case.bias_done else rb.float()), (case.id, tag, "bias gradient")
        assert drv.outside_untouched(flat), (case.id, tag, "flat gradient outside the layer's views")
        if first is None:
            first = (gw, gb, d)
    return first


# ---- the families ------------------------------------------------------------------------------------------------------------
S1 = (2, 5, 9, 13)
HEAD_CASES = [
    _Case("x-column head 16/16", "conv", 16, 16, S1),
    _Case("x-column head 16/16", "conv", 16, 10, S1),
    _Case("x-column head 16/12", "conv", 16, 10, S1, dy_ld=12),
    _Case("x-column head 16/16", "conv", 10, 10, S1, cg=16, x_ld=16, dy_ld=16),
    _Case("x-column head 16/12", "conv", 10, 10, S1, cg=16, x_ld=16, dy_ld=12),
    _Case("x-column head 12/16", "conv", 10, 10, S1, cg=16, x_ld=12, dy_ld=16),
    _Case("x-column head 12/12", "conv", 10, 10, S1, cg=16, x_ld=12, dy_ld=12),
    _Case("x-column head 12/12", "conv", 10, 10, (2, 5, 9, 4), cg=16, x_ld=12, dy_ld=12),        # Z = 4: the eligibility edge
]
HALO_CASES = [_Case(n, "conv", ci, co, sh, dy_ld=32 if co == 24 else None)
              for sh in (S1, (1, 4, 8, 8))
              for n, ci, co in (("halo 32x64", 16, 32), ("halo 64x32", 32, 16), ("halo 64x32", 32, 10), ("halo 64x64", 32, 32), ("halo 64x64", 32, 24))]
UP_CASES = [_Case(f"up {w}", "convT", 64, c, sh, dy_ld=w) for sh in ((2, 5, 6, 9), (3, 1, 2, 3)) for c in (10, 12, 16) for w in (16, 12) if not (c == 16 and w == 12)]
STEM_CASES = [_Case(f"stem {c}", "conv_s2", 1, c, sh) for sh in ((2, 8, 12, 8), (1, 10, 20, 24)) for c in (16, 32, 48, 64)]
PERSISTENT = HEAD_CASES + HALO_CASES + UP_CASES + STEM_CASES


@pytest.mark.parametrize("cap", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("case", PERSISTENT, ids=[c.id for c in PERSISTENT])
def test_persistent_kernels_are_exact_on_integers_capped_or_not(case, cap, monkeypatch):
    """x-column head, halo, up, stem: Oracle A, also with one and three workgroups for all tiles (several tiles per workgroup, a
    sample change inside a workgroup)"""
    _exact_run(case, monkeypatch, cap)


def test_twelve_wide_rows_give_the_sixteen_wide_result(monkeypatch):
    res = [_exact_run(c, monkeypatch)[:2] for c in HEAD_CASES[3:7]]
    for gw, gb in res[1:]:
        assert torch.equal(gw, res[0][0]) and torch.equal(gb, res[0][1])


def test_default_rows_of_32_to_24_run_the_generic_kernel(monkeypatch):
    _exact_run(_Case("generic 32", "conv", 32, 24, (1, 4, 8, 8)), monkeypatch)


RING_SHAPES = [("conv", 64, 64, (2, 7, 10, 6), "ring 512x64", "generic 64"), ("conv_s2", 32, 128, (2, 12, 16, 8), "ring 256x128", "generic 128"),
               ("conv", 64, 256, (2, 6, 6, 6), "ring 256x256", "generic 128")]
RING_CASES = [_Case(r, k, ci, co, sh) for k, ci, co, sh, r, _ in RING_SHAPES] + [
    _Case("ring 256x128", "convT", 128, 32, (2, 6, 6, 4)),          # roles swapped: gathered = dOut (32 channels), columns = 128
    _Case("ring 256x256", "conv", 96, 160, (2, 4, 5, 7)),
]
S2 = (2, 4, 5, 7)
BIG = (2, 8, 14, 14)
GENERIC_CASES = [
    _Case("generic 16", "conv", 8, 8, S1), _Case("generic 32", "conv", 24, 24, S1), _Case("generic 64", "conv", 48, 48, S1),
    _Case("generic 64", "conv", 96, 40, S2), _Case("generic 128", "conv", 24, 160, S2),
    _Case("generic 16", "conv", 8, 8, S1, dt=F32), _Case("generic 32", "conv", 24, 24, S1, dt=F32), _Case("generic 64", "conv", 48, 48, S1, dt=F32),
    _Case("generic 64", "conv", 96, 40, S2, dt=F32), _Case("generic 128", "conv", 96, 160, S2, dt=F32),
    _Case("generic 16 element-wise", "conv2d", 3, 16, (2, 9, 13, 1)), _Case("generic 16 element-wise", "conv2d_s2", 3, 16, (2, 10, 14, 1)),
    _Case("generic 16 element-wise", "conv_s2", 1, 16, (2, 8, 12, 8), dt=F32), _Case("generic 16 element-wise", "conv", 6, 8, S1, dt=F32),
    _Case("generic 32", "conv2d_s2", 16, 32, (2, 10, 14, 1)), _Case("generic 32", "convT2d", 32, 16, (2, 5, 7, 1)),
    _Case("generic 32", "conv", 48, 24, S1, k=1), _Case("generic 128", "convT", 96, 24, (2, 4, 5, 3)),
] + [_Case(g, k, ci, co, sh, env={"CTSEG_WGRAD_RING": "0"}) for k, ci, co, sh, _, g in RING_SHAPES] + [
    _Case("generic 64", "convT", 64, c, (2, 5, 6, 9), env={"CTSEG_NO_WGRAD_UP": "1"}) for c in (10, 16)]


@pytest.mark.parametrize("case", RING_CASES + GENERIC_CASES, ids=[c.id for c in RING_CASES + GENERIC_CASES])
def test_split_k_kernels_are_exact_on_integers(case, monkeypatch):
    _exact_run(case, monkeypatch)


# ---- the 2-D U-Net at its real widths ----------------------------------------------------------------------------------------
# The weight-gradient rows of tests/unet2d_passes.py (BaseUNet2D, filters 64 .. 1024, residual units; the CPU test of
# tests/test_abi_exports.py holds the names against the plan recorder): up to 1536 columns (6 column blocks of "ring 256x256"), K up
# to 9 * 1024, the transposed layers with their roles swapped (gathered = dOut).  (2, 13, 19) stride-1 / transposed input, (2, 28, 30)
# stride-2 input; the bottom unit gathers the lower 512 columns of the 1536-wide skip concat.
P1, P2 = (2, 13, 19, 1), (2, 28, 30, 1)
UNET2D_CASES = [
    _Case("generic 16", "conv2d", 10, 10, P1, cg=16, x_ld=16, dy_ld=16), _Case("generic 128", "convT2d", 128, 10, P1),
    _Case("ring 512x64", "conv2d", 64, 64, P1), _Case("ring 256x256", "convT2d", 256, 64, P1),
    _Case("ring 256x128", "conv2d", 128, 128, P1), _Case("ring 256x256", "convT2d", 512, 128, P1),
    _Case("ring 256x256", "conv2d", 256, 256, P1), _Case("ring 256x256", "convT2d", 1536, 256, P1),
    _Case("ring 256x256", "conv2d", 1024, 1024, (1, 13, 19, 1)), _Case("ring 256x256", "conv2d", 512, 1024, P1, x_ld=1536),
    _Case("ring 256x256", "conv2d", 512, 1024, P1, k=1, x_ld=1536), _Case("ring 256x256", "conv2d", 512, 512, P1),
]
# the fused [residual | unit0] GEMM of the strided residual units: (name, cin, C of each half)
UNET2D_FUSED = [("generic 128 element-wise", 1, 64), ("ring 256x256", 64, 128), ("ring 256x256", 128, 256), ("ring 256x256", 256, 512)]


def test_unet2d_cases_are_the_recorded_weight_gradient_passes():
    from unet2d_passes import UNET2D_PASSES
    table = {(kind, cin, cout, k, fused): (name, Cg, Cn) for pas, _, kind, cin, cout, k, fused, Cg, Cn, _, name in UNET2D_PASSES if pas == "wgrad"}
    cases = {(c.op, c.cin, c.cout, c.k, False): (c.name, c.cg or (c.cout if c.op == "convT" else c.cin), c.cin if c.op == "convT" else c.cout)
             for c in UNET2D_CASES}
    cases.update({("conv_s2", cin, 2 * C, 3, True): (name, cin, 2 * C) for name, cin, C in UNET2D_FUSED})
    # (a transposed layer gathers dOut in 16-byte chunked rows: 16 channels for the 10 classes)
    cases[("convT", 128, 10, 3, False)] = ("generic 128", 16, 128)
    assert cases == table


@pytest.mark.parametrize("case", UNET2D_CASES, ids=[c.id for c in UNET2D_CASES])
def test_unet2d_layers_are_exact_on_integers(case, monkeypatch):
    _exact_run(case, monkeypatch)


@pytest.mark.parametrize("name,cin,C", UNET2D_FUSED, ids=[f"{n}_{ci}->2x{c}".replace(" ", "_") for n, ci, c in UNET2D_FUSED])
def test_unet2d_fused_down_unit_equals_the_two_layers(name, cin, C, monkeypatch):
    """ONE weight-gradient pass over the 2 * C columns of [d_res | d_y0], two slab reduces at col0 = 0 and C: each half must equal
    the float64 gradient of its own layer (residual, unit0) bit for bit, bias gradient included; Oracle A as in _exact_run (NaN slabs,
    untouched guards, replay over stale slabs with other operands)"""
    case = _Case(name, "conv2d_s2", cin, 2 * C, P2)
    case.setenv(monkeypatch)
    xs, ys, _ = case.sizes()
    assert 16 * xs[0] * ys[2] * ys[3] < 2 ** 24, "the integer oracle is exact only below 2^24"
    gen = torch.Generator().manual_seed(case.seed)
    torch.manual_seed(1)
    mods = [conv_module("conv_s2", cin, C, 3, 2) for _ in range(2)]
    drv = WgradPassDriver(mods, BF16, DEV)
    for rnd in range(2):
        x, dy = _ints(xs, gen), _ints(ys, gen)
        refs = [conv_wgrad("conv_s2", 3, x, dy[:, h * C:(h + 1) * C], tuple(mods[h].weight.shape), torch.float64) for h in (0, 1)]
        if rnd == 0:
            xa, ga = case.acts(drv, x, dy)
            d = drv.record(name, xa, ga)
            assert d.Cn == 2 * C and sum(1 for p in drv.prog or drv.plan.prog if p[0] == "ctseg_conv_wgrad_reduce") == 2
            flat = drv.go(poison=float("nan"))[3]
        else:
            xa.t[..., :cin].copy_(x.unsqueeze(-1).permute(0, 2, 3, 4, 1))
            ga.t[..., :2 * C].copy_(dy.unsqueeze(-1).permute(0, 2, 3, 4, 1))
            flat = drv.go()[3]
        tag = "poisoned slabs" if rnd == 0 else "replay over stale slabs"
        for (gw, gb), (rw, rb), half in zip(drv.part_grads(flat), refs, ("residual", "unit0")):
            assert bool((rw.abs().flatten(1).sum(1) > 0).all()) and bool((rw.abs().transpose(0, 1).flatten(1).sum(1) > 0).all()), \
                "an all-zero channel slice of the reference: a skipped column or K block would pass"
            assert bool((rb != 0).any())
            assert torch.equal(gw, rw.float()), (name, tag, half, "weight gradient", int((gw != rw.float()).sum()))
            assert torch.equal(gb, rb.float()), (name, tag, half, "bias gradient")
        assert drv.outside_untouched(flat), (name, tag, "flat gradient outside the two layers' views")


# (case, expected splits, flat XCD-ordered grid?)
GRID_CASES = [
    (_Case("generic 64", "conv", 48, 48, BIG, target=88), 4, True),          # N * splits = 8, 11 K blocks per slab
    (_Case("generic 64", "conv", 48, 48, BIG, target=66), 3, False),         # 6 slabs: the 3-D grid; 1568 rows in 544 + 544 + 480
    (_Case("ring 512x64", "conv", 64, 64, BIG, target=112), 4, True),
    (_Case("ring 512x64", "conv", 64, 64, BIG, target=84), 3, False),
    (_Case("generic 64", "conv", 48, 48, S1, splits=12), 12, True),          # 585 rows in 64-row ranges: 9 rows in range 9, none in 10, 11
    (_Case("ring 512x64", "conv", 64, 64, S1, splits=12), 12, True),
    (_Case("generic 16", "conv", 8, 8, S1, splits=5), 5, False),             # 585 rows in 128-row ranges, the last one 73 rows
]


@pytest.mark.parametrize("case,splits,flat", GRID_CASES, ids=[c[0].id for c in GRID_CASES])
def test_split_counts_and_grid_forms(case, splits, flat, monkeypatch):
    _, _, d = _exact_run(case, monkeypatch)
    assert d.splits == splits
    wps = nat.lib().ctseg_conv_wgrad_wgs_per_slab(ctypes.byref(d), None, None)
    assert ((d.N * d.splits) % 8 == 0 and wps > 1) == flat, (d.N, d.splits, wps)
    rows = d.Xr * d.Yr * d.Zr
    rps = -(-(-(-rows // d.splits)) // 32) * 32
    if case.splits == 12:
        assert rps * (d.splits - 1) >= rows, "the last split is empty"
    else:
        assert rps * (d.splits - 1) < rows < rps * d.splits, "the last split is short"


def test_up_kernel_writes_the_bias_row_of_the_tightest_slab(monkeypatch):
    """kpad_w = 27 * 16 + 1, the smallest the C ABI takes for the stride-2 transposed kernel (the mirror rounds it up to 512): the
    bias row is then the LAST row of the slab, the one its `row < kpad_w` guard decides.  Every other guarded store of the library
    decides a pad row only: the halo kernels are refused below kpad_w = K + 16, the ring and generic kernels take multiples of 128
    and K + 1 = ntaps * Cg + 1 with Cg % 8 == 0 is odd; the reduce reads rows [0, K] alone.  The slabs are summed here."""
    case = _Case("up 16", "convT", 64, 10, (2, 5, 6, 9), dy_ld=16)
    case.setenv(monkeypatch)
    xs, ys, wshape = case.sizes()
    gen = torch.Generator().manual_seed(case.seed)
    x, dy = _ints(xs, gen), _ints(ys, gen)
    drv = case.driver()
    xa, ga = case.acts(drv, x, dy)
    d = type(drv.record(case.name, xa, ga)).from_buffer_copy(drv.desc)
    d.kpad_w = 27 * 16 + 1
    assert nat.lib().ctseg_wgrad_pass_name(ctypes.byref(d)) == b"up 16"
    nslabs = nat.lib().ctseg_conv_wgrad_slabs(ctypes.byref(d))
    assert nslabs > 0
    ws = torch.full((nslabs, d.kpad_w, d.cn_pad), float("nan"), device=DEV)
    d.ws = ws.data_ptr()
    nat.call("ctseg_conv_wgrad", d)
    torch.cuda.synchronize()
    tot = ws.sum(0).cpu()
    rw, _ = conv_wgrad(case.op, case.k, x, dy, wshape, torch.float64)              # [ci][co][tap]
    assert torch.equal(tot[:432].view(27, 16, d.cn_pad)[:, :10, :64], rw.reshape(64, 10, 27).permute(2, 1, 0).float())
    assert torch.equal(tot[432, :64], x.sum((0, 2, 3, 4)))


# ---- conv_wgrad_head_kernel: taps out of canonical order, called directly ----------------------------------------------------
# 16 input channels do not fit a 12-wide row: "head 12/12" is the 10 -> 10 layer of HEAD_CASES (Cg = 16) with both rows 12 wide
HEAD_REVERSED = [("head 16/16", _Case("x-column head 16/16", "conv", 16, 10, S1)),
                 ("head 12/12", _Case("x-column head 12/12", "conv", 10, 10, S1, cg=16, x_ld=12, dy_ld=12))]


@pytest.mark.parametrize("cap", [None, "3"], ids=["uncapped", "max_wg3"])
@pytest.mark.parametrize("name,case", HEAD_REVERSED, ids=[c[0].replace(" ", "_") for c in HEAD_REVERSED])
def test_head_kernel_on_reversed_taps_equals_the_x_column_kernel(name, case, cap, monkeypatch):
    """The recorded descriptor of the canonical-order case with its 27 taps in reverse order runs conv_wgrad_head_kernel (taps in
    any order); its reduced gradient over NaN-poisoned slabs is the x-column kernel's with the tap axis reversed, bit for bit (the
    operands are integers: exact in any order), and the bias gradient is the same.  CTSEG_MAX_WG=3: several tiles per workgroup."""
    case.setenv(monkeypatch, cap)
    xs, ys, _ = case.sizes()
    gen = torch.Generator().manual_seed(case.seed)
    drv = case.driver()
    xa, ga = case.acts(drv, _ints(xs, gen), _ints(ys, gen))          # (stay alive: the reversed descriptor reads them too)
    d0 = drv.record(case.name, xa, ga)
    gw, gb, _, _ = drv.go(poison=float("nan"))
    assert bool((gw != 0).any()) and bool((gb != 0).any())
    L = nat.lib()
    d = type(d0).from_buffer_copy(d0)
    assert d.ntaps == 27
    for j in range(27):
        d.taps[j] = d0.taps[26 - j]
    assert L.ctseg_wgrad_pass_name(ctypes.byref(d)) == name.encode()
    nslabs = L.ctseg_conv_wgrad_slabs(ctypes.byref(d))
    assert nslabs > 0
    ws = torch.full((nslabs, d.kpad_w, d.cn_pad), float("nan"), device=DEV)
    d.ws = ws.data_ptr()
    co, ci = gw.shape[:2]
    dw = torch.full((co * ci * 27 + 8,), GRAD_SENTINEL, device=DEV)
    db = torch.full((co + 8,), GRAD_SENTINEL, device=DEV)
    nat.call("ctseg_conv_wgrad", d)
    nat.call("ctseg_conv_wgrad_reduce", ws.data_ptr(), nslabs, d.kpad_w, d.cn_pad, ci, d.Cg, 27, 0, co, dw.data_ptr(), db.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(dw[:co * ci * 27].cpu().view(co, ci, 27), gw.reshape(co, ci, 27).flip(-1)), (name, cap, "weight gradient")
    assert torch.equal(db[:co].cpu(), gb), (name, cap, "bias gradient")
    assert bool((dw[co * ci * 27:] == GRAD_SENTINEL).all()) and bool((db[co:] == GRAD_SENTINEL).all())


# ---- Oracle B ----------------------------------------------------------------------------------------------------------------
NORMAL_CASES = [
    _Case("x-column head 12/12", "conv", 10, 10, S1, cg=16, x_ld=12, dy_ld=12), _Case("halo 64x64", "conv", 32, 32, S1),
    _Case("halo 32x64", "conv", 16, 32, S1), _Case("halo 64x32", "conv", 32, 16, S1),
    _Case("up 12", "convT", 64, 10, (2, 5, 6, 9), dy_ld=12), _Case("stem 32", "conv_s2", 1, 32, (2, 8, 12, 8)),
    _Case("ring 512x64", "conv", 64, 64, (2, 7, 10, 6)), _Case("ring 256x128", "conv_s2", 32, 128, (2, 12, 16, 8)),
    _Case("ring 256x256", "conv", 64, 256, (2, 6, 6, 6)),
    _Case("generic 64", "conv", 48, 48, S1), _Case("generic 64", "conv", 48, 48, S1, dt=F32),
    _Case("generic 16 element-wise", "conv2d", 3, 16, (2, 33, 45, 1)),
    # the 2-D U-Net at its real widths: one row per distinct weight-gradient pass name of tests/unet2d_passes.py, the six column blocks
    # of ConvTranspose2d 1536 -> 256 and K = 9 * 1024 ("generic 128 element-wise": the fused first layer, below)
    _Case("generic 16", "conv2d", 10, 10, (2, 13, 19, 1), cg=16, x_ld=16, dy_ld=16), _Case("generic 128", "convT2d", 128, 10, (2, 13, 19, 1)),
    _Case("ring 512x64", "conv2d", 64, 64, (2, 13, 19, 1)), _Case("ring 256x128", "conv2d", 128, 128, (2, 13, 19, 1)),
    _Case("ring 256x256", "convT2d", 1536, 256, (2, 13, 19, 1)), _Case("ring 256x256", "conv2d", 1024, 1024, (1, 13, 19, 1)),
]


def _normalised_check(tag, gw, gb, x, dy, kind, k, wshape, n_rows):
    """|got - ref| / S against 16 x the float32 evaluation's, S = gradient of (|x|, |dy|)"""
    rw, rb = conv_wgrad(kind, k, x, dy, wshape, torch.float64)
    sw, sb = conv_wgrad(kind, k, x.abs(), dy.abs(), wshape, torch.float64)
    fw, fb = conv_wgrad(kind, k, x, dy, wshape, torch.float32)
    assert bool((sw > 0).all()) and bool((sb > 0).all())
    bound_w, bound_b = 16.0 * float(((fw.double() - rw).abs() / sw).max()), 16.0 * float(((fb.double() - rb).abs() / sb).max())
    if bound_b == 0.0:      # torch's float32 column sums of dy came out exact (few hundred bf16 values): one float32 rounding, see above
        bound_b = 2.0 ** -24
    err_w, err_b = float(((gw.double() - rw).abs() / sw).max()), float(((gb.double() - rb).abs() / sb).max())
    cap = 1.0 / (4 * n_rows)
    print(f"{tag}: weight {err_w:.3e} (bound {bound_w:.3e}), bias {err_b:.3e} (bound {bound_b:.3e}), cap {cap:.3e}")
    assert 0.0 < bound_w < cap, ("float32 reference error x 16 of the weight gradient is not inside (0, 1 / (4 * N * rows))", bound_w, n_rows)
    assert 0.0 < bound_b < cap, ("float32 reference error x 16 of the bias gradient is not inside (0, 1 / (4 * N * rows))", bound_b, n_rows)
    assert err_w <= bound_w, (tag, "weight gradient", err_w, bound_w)
    assert err_b <= bound_b, (tag, "bias gradient", err_b, bound_b)


@pytest.mark.parametrize("case", NORMAL_CASES, ids=[c.id for c in NORMAL_CASES])
def test_normal_valued_operands_within_the_float32_bound(case, monkeypatch):
    case.setenv(monkeypatch)
    xs, ys, wshape = case.sizes()
    torch.manual_seed(case.seed)
    tdt = nat.torch_dtype(case.dt)
    x, dy = torch.randn(xs).to(tdt).float(), torch.randn(ys).to(tdt).float()
    drv = case.driver()
    xa, ga = case.acts(drv, x, dy)
    drv.record(case.name, xa, ga, bias_done=case.bias_done)
    gw, gb, d, flat = drv.go(poison=float("nan"))
    assert drv.outside_untouched(flat)
    if case.bias_done:
        gb = conv_wgrad(case.op, case.k, x, dy, wshape, torch.float64)[1].float()       # (not computed by this pass)
    _normalised_check(case.id, gw, gb, x, dy, case.op, case.k, wshape, d.N * d.Xr * d.Yr * d.Zr)


@pytest.mark.parametrize("name,cin,C", [UNET2D_FUSED[0], UNET2D_FUSED[3]], ids=["generic_128_element-wise_1->2x64", "ring_256x256_256->2x512"])
def test_unet2d_fused_down_unit_normal_valued_within_the_float32_bound_of_each_layer(name, cin, C, monkeypatch):
    """Oracle B on the single pass of a fused [residual | unit0] unit: each half against the float64 gradient of its own layer, with
    that layer's own bound (_normalised_check, unchanged)"""
    case = _Case(name, "conv2d_s2", cin, 2 * C, P2)
    case.setenv(monkeypatch)
    xs, ys, _ = case.sizes()
    torch.manual_seed(case.seed)
    x, dy = torch.randn(xs).bfloat16().float(), torch.randn(ys).bfloat16().float()
    mods = [conv_module("conv_s2", cin, C, 3, 2) for _ in range(2)]
    drv = WgradPassDriver(mods, BF16, DEV)
    xa, ga = case.acts(drv, x, dy)
    d = drv.record(name, xa, ga)
    flat = drv.go(poison=float("nan"))[3]
    assert drv.outside_untouched(flat)
    for h, ((gw, gb), half) in enumerate(zip(drv.part_grads(flat), ("residual", "unit0"))):
        _normalised_check(f"{case.id} {half}", gw, gb, x, dy[:, h * C:(h + 1) * C], "conv_s2", 3, tuple(mods[h].weight.shape), d.N * d.Xr * d.Yr * d.Zr)


# ---- operand normalised on load (in_mean_rstd): the x-column head kernel -----------------------------------------------------
@pytest.mark.parametrize("N", [2, 16])
def test_operand_normalised_on_load_equals_the_materialised_activation(N, monkeypatch):
    case = _Case("x-column head 12/12", "conv", 10, 10, (N, 5, 9, 13), cg=16, x_ld=12, dy_ld=12)
    case.setenv(monkeypatch)
    xs, ys, wshape = case.sizes()
    C, dims = 10, case.shape[1:]
    alpha = torch.nn.Parameter(torch.tensor([0.2]))
    torch.manual_seed(1)
    drv = WgradPassDriver(conv_module("conv", 10, 10), BF16, DEV, cg=16, extra_params=[alpha])
    drv.plan.narrow_rows = True
    na, y, m, r = norm_for(drv, alpha, N, C, dims, seed=5)
    ya = to_cl(y, BF16, DEV, ld=12)
    na.y = ya
    dy = torch.randn(ys, generator=torch.Generator().manual_seed(9)).bfloat16().float()
    ga = drv.act(dy, ld=12)
    xm = na._apply(ya, None, None)                       # the materialised activation, 12-wide rows as well
    drv.plan.run()
    torch.cuda.synchronize()
    d0 = drv.record(case.name, xm, ga)
    assert not d0.in_mean_rstd
    gw0, gb0, _, _ = drv.go(poison=float("nan"))
    plain = (drv.prog, drv.ws)
    ya.pending_norm = na
    d1 = drv.record(case.name, ya, ga)
    assert d1.in_mean_rstd and d1.in_norm_C == C and d1.in_ == ya.ptr(), "the pass normalises on load"
    assert nat.lib().ctseg_wgrad_in_norm_ok(ctypes.byref(d1)) == 1
    gw1, gb1, _, flat = drv.go(poison=float("nan"))
    assert torch.equal(gw1, gw0) and torch.equal(gb1, gb0)
    # float64 conv(prelu((y - m) * r)): padding voxels contribute zero, not prelu(-mean * rstd).  The activation the kernel
    # multiplies is rounded to bf16: the references take the stored activation (checked against float64 to bf16 rounding) as operand.
    xh = (y.double() - m) * r
    act64 = torch.where(xh > 0, xh, 0.2 * xh)
    act = xm.valid().float().cpu()
    assert float(((act.double() - act64).abs() / act64.abs().clamp(min=2.0 ** -6)).max()) < 2.0 ** -7, "the materialised activation against float64"
    _normalised_check(case.id + " on load", gw1, gb1, act, dy, "conv", 3, wshape, N * d1.Xr * d1.Yr * d1.Zr)
    # both recorded programs again over their own stale slabs, with another dY in the same tensor
    on_load = (drv.prog, drv.ws)
    dy2 = torch.randn(ys, generator=torch.Generator().manual_seed(11)).bfloat16().float()
    ga.t[..., :C].copy_(dy2.permute(0, 2, 3, 4, 1))
    gw2, gb2, _, _ = _replay(drv, plain)
    gw3, gb3, _, flat = _replay(drv, on_load)
    assert torch.equal(gw3, gw2) and torch.equal(gb3, gb2) and not torch.equal(gw3, gw1) and drv.outside_untouched_but(flat, alpha)
    _normalised_check(case.id + " on load, replay", gw3, gb3, act, dy2, "conv", 3, wshape, N * d1.Xr * d1.Yr * d1.Zr)
    # what the query turns down
    for n, c in ((17, 10), (2, 13)):
        bad = type(d1).from_buffer_copy(d1)
        bad.N, bad.in_norm_C = n, c
        assert nat.lib().ctseg_wgrad_in_norm_ok(ctypes.byref(bad)) == 0


def _replay(drv, saved):
    """a recorded (program, slab buffer) of the driver once more, slabs as the last run left them"""
    drv.prog, drv.ws = saved
    return drv.go()


def test_operand_normalisation_is_refused_off_the_head_kernel(monkeypatch):
    case = _Case("halo 64x64", "conv", 32, 32, (1, 4, 8, 8))
    case.setenv(monkeypatch)
    xs, ys, _ = case.sizes()
    drv = case.driver()
    xa, ga = case.acts(drv, torch.zeros(xs), torch.zeros(ys))
    d = drv.record(case.name, xa, ga)
    mr = torch.zeros(1, 32, 2, device=DEV)
    al = torch.zeros(1, device=DEV)
    d.in_mean_rstd, d.in_alpha, d.in_norm_C = mr.data_ptr(), al.data_ptr(), 10
    assert nat.lib().ctseg_wgrad_in_norm_ok(ctypes.byref(d)) == 0
    assert nat.lib().ctseg_wgrad_pass_name(ctypes.byref(d)) is None
    assert nat.lib().ctseg_conv_wgrad(ctypes.byref(d), None) != 0
    assert b"in_mean_rstd (normalise the operand on load) is not implemented for this pass" in nat.lib().ctseg_last_error()


# ---- dY formed on load (dyn_*): the stem kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,N", [(32, 2), (64, 2), (32, 8), (64, 8)])
def test_dy_formed_on_load_equals_the_apply_pass(Cn, N, monkeypatch):
    C = Cn // 2
    case = _Case(f"stem {Cn}", "conv_s2", 1, Cn, (N, 8, 12, 8))
    case.setenv(monkeypatch)
    xs, ys, wshape = case.sizes()
    rdims = ys[2:]
    alpha = torch.nn.Parameter(torch.tensor([0.2]))
    torch.manual_seed(1)
    drv = WgradPassDriver(conv_module("conv_s2", 1, Cn), BF16, DEV, extra_params=[alpha])
    gen = torch.Generator().manual_seed(Cn + N)
    x = torch.randn(xs, generator=gen).bfloat16().float()
    dy_lo = torch.randn((N, C) + rdims, generator=gen).bfloat16().float()
    g = torch.randn((N, C) + rdims, generator=gen).bfloat16().float()
    na, y, m, r = norm_for(drv, alpha, N, C, rdims, seed=Cn)
    xa, lo, ga = drv.act(x, ld=1), to_cl(dy_lo, BF16, DEV), to_cl(g, BF16, DEV)
    # plain: the apply pass writes the upper half of a fused [d_res | dy0] tensor
    fused = new_act(N, *rdims, Cn, BF16, DEV)
    fused.t[..., :C].copy_(lo.t[..., :C])
    na.emit_bwd(ga, dy_out=fused.slice(C, C))
    drv.plan.run()
    torch.cuda.synchronize()
    drv.record(f"stem {Cn}", xa, fused)
    gw0, gb0, _, _ = drv.go(poison=float("nan"))
    plain = (drv.prog, drv.ws)
    # on load: statistics only, then the pass forms the upper half itself
    sums = na.emit_bwd(ga, apply=False)
    drv.plan.run()
    torch.cuda.synchronize()
    d = drv.record(f"stem {Cn} dyn", xa, lo, dyn=(ga, na, sums))
    assert d.dyn_col0 == C and d.dyn_g and nat.lib().ctseg_wgrad_dy_norm_ok(ctypes.byref(d)) == 1
    gw1, gb1, _, flat = drv.go(poison=float("nan"))
    assert torch.equal(gw1, gw0) and torch.equal(gb1, gb0)
    # float64 through InstanceNorm + PReLU + the convolution (the norm's float32 (mean, rstd) table); the formed dy0 is rounded to
    # bf16 by the kernel as the apply pass rounds it, which the references take as their operand
    dy0 = norm_prelu_dy(g.double(), y.double(), m, r, 0.2)
    stored = fused.valid().float().cpu()
    assert float((stored[:, C:].double() - dy0).abs().max() / dy0.abs().max()) < 2.0 ** -7, "the apply pass against float64"
    _normalised_check(case.id + " dyn", gw1, gb1, x, stored, "conv_s2", 3, wshape, N * d.Xr * d.Yr * d.Zr)
    # both recorded programs again over their own stale slabs, with another x and lower half of dY in the same tensors (g, y and
    # with them the sums and the formed upper half stay)
    on_load = (drv.prog, drv.ws)
    x2 = torch.randn(xs, generator=gen).bfloat16().float()
    lo2 = torch.randn((N, C) + rdims, generator=gen).bfloat16().float()
    xa.t[..., :1].copy_(x2.permute(0, 2, 3, 4, 1))
    for t in (lo.t, fused.t):
        t[..., :C].copy_(lo2.permute(0, 2, 3, 4, 1))
    gw2, gb2, _, _ = _replay(drv, plain)
    gw3, gb3, _, _ = _replay(drv, on_load)
    assert torch.equal(gw3, gw2) and torch.equal(gb3, gb2) and not torch.equal(gw3, gw1)
    _normalised_check(case.id + " dyn, replay", gw3, gb3, x2, fused.valid().float().cpu(), "conv_s2", 3, wshape, N * d.Xr * d.Yr * d.Zr)
    # what the query and the launch turn down
    for field, val in (("N", 9), ("dyn_col0", C - 8)):
        bad = type(d).from_buffer_copy(d)
        setattr(bad, field, val)
        assert nat.lib().ctseg_wgrad_dy_norm_ok(ctypes.byref(bad)) == 0
        assert nat.lib().ctseg_conv_wgrad(ctypes.byref(bad), None) != 0
        assert b"dyn_* (dY formed on load) is not implemented for this pass" in nat.lib().ctseg_last_error()


def test_dy_on_load_is_refused_for_48_columns_and_off_the_stem_kernel(monkeypatch):
    for case, col0 in ((_Case("stem 48", "conv_s2", 1, 48, (1, 8, 12, 8)), 24), (_Case("halo 64x64", "conv", 32, 32, (1, 4, 8, 8)), 16)):
        case.setenv(monkeypatch)
        xs, ys, _ = case.sizes()
        drv = case.driver()
        xa, ga = case.acts(drv, torch.zeros(xs), torch.zeros(ys))
        d = drv.record(case.name, xa, ga)
        buf = torch.zeros(ys[0], *ys[2:], 32, dtype=torch.bfloat16, device=DEV)
        f = torch.zeros(ys[0], 32, 2, device=DEV)
        d.dyn_col0, d.dyn_g, d.dyn_y, d.dyn_g_ld, d.dyn_y_ld = col0, buf.data_ptr(), buf.data_ptr(), 32, 32
        d.dyn_mean_rstd = d.dyn_alpha = d.dyn_sums = f.data_ptr()
        assert nat.lib().ctseg_wgrad_dy_norm_ok(ctypes.byref(d)) == 0
        assert nat.lib().ctseg_conv_wgrad(ctypes.byref(d), None) != 0
        assert b"dyn_* (dY formed on load) is not implemented for this pass" in nat.lib().ctseg_last_error()


# (Which reduce kernel ran cannot be asked: there is no name query for them.  The cases are chosen from the dispatch conditions of
# ctseg_conv_wgrad_reduce, which the test restates to check that a case's label and its arguments agree -- no more than that.)
# ---- slab reduces, called directly -------------------------------------------------------------------------------------------
def _slabs(nslabs, kpad_w, cn_pad, seed, offset=0):
    g = torch.Generator().manual_seed(seed)
    ws = torch.randint(-512, 513, (nslabs, kpad_w, cn_pad), generator=g, dtype=torch.int64)
    dev = torch.full((ws.numel() + 4,), float("nan"), dtype=torch.float32, device=DEV)
    dev[offset:offset + ws.numel()].copy_(ws.flatten().float())
    return ws, dev, dev.data_ptr() + 4 * offset


def _reduce_ref(ws, A, AS, T, col0, nb):
    s = ws.sum(0)
    dw = s[:T * AS, col0:col0 + nb].reshape(T, AS, nb)[:, :A].permute(2, 1, 0).contiguous().float()      # [nb][A][T]
    return dw, s[T * AS, col0:col0 + nb].float()


# (kernel the dispatch of ctseg_conv_wgrad_reduce picks, nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, with db)
REDUCE_CASES = [
    ("reduce4<8,32>", 64, 128, 16, 10, 16, 1, 0, 10, True),            # nslabs >= 64, aligned; nb % 4 != 0; A < AS
    ("reduce4<8,32>", 200, 256, 32, 16, 16, 9, 16, 14, False),         # col0 > 0, col0 + roundup(nb, 4) == cn_pad, no db
    ("reduce4<32,8>", 1, 128, 16, 8, 8, 8, 0, 16, True),
    ("reduce4<32,8>", 7, 512, 32, 12, 16, 27, 4, 10, True),
    ("reduce4<32,8>", 63, 128, 64, 3, 4, 27, 8, 56, False),            # col0 + nb == cn_pad
    ("reduce<32>", 256, 128, 18, 5, 8, 9, 2, 16, True),                # unaligned (col0 = 2), nslabs >= 256, 37 blocks
    ("reduce<8>", 3, 128, 16, 10, 16, 1, 2, 13, True),                 # unaligned, few slabs
    ("reduce<8>", 2, 1792, 162, 64, 64, 27, 2, 160, True),             # (T * AS + 1) * nb > 8192 * 32: the capped grid loops
    ("reduce<8>", 256, 1792, 20, 64, 64, 27, 0, 20, False),            # ws at a 4-byte offset; nslabs >= 256 but 1081 blocks > 1024
]


@pytest.mark.parametrize("kernel,nslabs,kpad_w,cn_pad,A,AS,T,col0,nb,with_db", REDUCE_CASES,
                         ids=[f"{c[0]}_nslabs{c[1]}_T{c[6]}_col0{c[7]}_nb{c[8]}" for c in REDUCE_CASES])
def test_slab_reduce_kernels_against_an_int64_sum(kernel, nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, with_db):
    L = nat.lib()
    off = 1 if kernel.startswith("reduce<") and col0 == 0 else 0
    ws, dev, ptr = _slabs(nslabs, kpad_w, cn_pad, seed=nslabs + T, offset=off)
    assert nslabs <= 1024 and 512 * nslabs < 2 ** 24
    aligned = L.ctseg_conv_wgrad_reduce_batch_ok(ptr, cn_pad, col0, nb) == 1
    total = (T * AS + 1) * nb
    blocks = min(-(-total // 32), 8192)
    expect = ("reduce4<8,32>" if nslabs >= 64 else "reduce4<32,8>") if aligned else ("reduce<32>" if nslabs >= 256 and blocks <= 1024 else "reduce<8>")
    assert expect == kernel, "the case is not on the kernel its id names (dispatch of ctseg_conv_wgrad_reduce)"
    if kernel == "reduce<8>" and nslabs == 2:
        assert total > 8192 * 32
    dw = torch.full((nb * A * T + 8,), GRAD_SENTINEL, device=DEV)
    db = torch.full((nb + 8,), GRAD_SENTINEL, device=DEV)
    nat.call("ctseg_conv_wgrad_reduce", ptr, nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, dw.data_ptr(), db.data_ptr() if with_db else None)
    torch.cuda.synchronize()
    rw, rb = _reduce_ref(ws, A, AS, T, col0, nb)
    assert torch.equal(dw[:nb * A * T].cpu().view(nb, A, T), rw)
    assert bool((dw[nb * A * T:] == GRAD_SENTINEL).all())
    assert torch.equal(db[:nb].cpu(), rb) if with_db else bool((db == GRAD_SENTINEL).all())
    assert bool((db[nb:] == GRAD_SENTINEL).all())


def test_batched_slab_reduce_equals_the_single_calls_and_the_int64_sum():
    L = nat.lib()
    # nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, with db
    shapes = [(64, 128, 16, 10, 16, 1, 0, 10, True), (7, 512, 32, 12, 16, 27, 4, 10, True), (1, 128, 16, 8, 8, 8, 0, 16, False),
              (130, 256, 32, 16, 16, 9, 16, 14, True), (20, 128, 64, 3, 4, 27, 8, 56, True)]
    jobs = (nat.ReduceJob * len(shapes))()
    keep, block0 = [], 0
    for j, (nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, with_db) in enumerate(shapes):
        ws, dev, ptr = _slabs(nslabs, kpad_w, cn_pad, seed=40 + j)
        assert L.ctseg_conv_wgrad_reduce_batch_ok(ptr, cn_pad, col0, nb) == 1
        bufs = [torch.full((nb * A * T + 8,), GRAD_SENTINEL, device=DEV) for _ in range(2)] + [torch.full((nb + 8,), GRAD_SENTINEL, device=DEV) for _ in range(2)]
        J = jobs[j]
        J.ws, J.dw, J.db = ptr, bufs[0].data_ptr(), bufs[2].data_ptr() if with_db else None
        J.nslabs, J.kpad_w, J.cn_pad, J.A, J.Astride, J.T, J.col0, J.nb = nslabs, kpad_w, cn_pad, A, AS, T, col0, nb
        J.lanes = 8 if nslabs >= 64 else 32                                    # the header's rule
        J.block0 = block0
        block0 += -(-((T * AS + 1) * (-(-nb // 4))) // J.lanes)
        nat.call("ctseg_conv_wgrad_reduce", ptr, nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, bufs[1].data_ptr(), bufs[3].data_ptr() if with_db else None)
        keep.append((ws, dev, bufs))
    table = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(DEV)
    nat.call("ctseg_conv_wgrad_reduce_batch", table.data_ptr(), len(shapes), block0)
    torch.cuda.synchronize()
    for (nslabs, kpad_w, cn_pad, A, AS, T, col0, nb, with_db), (ws, dev, bufs) in zip(shapes, keep):
        rw, rb = _reduce_ref(ws, A, AS, T, col0, nb)
        assert torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[2], bufs[3]), "batched against the per-job calls"
        assert torch.equal(bufs[0][:nb * A * T].cpu().view(nb, A, T), rw) and bool((bufs[0][nb * A * T:] == GRAD_SENTINEL).all())
        assert torch.equal(bufs[2][:nb].cpu(), rb) if with_db else bool((bufs[2] == GRAD_SENTINEL).all())
        assert bool((bufs[2][nb:] == GRAD_SENTINEL).all())
