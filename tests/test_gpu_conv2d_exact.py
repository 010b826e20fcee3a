"""GPU: the forward and input-gradient conv passes of the 2-D U-Net at its real widths, element by element against float64.

The layers are those BaseUNet2D(filters=[64, 128, 256, 512, 1024], use_res_units=True) records in bf16; tests/unet2d_passes.py lists
every pass with the kernel the selector names for it, and tests/test_abi_exports.py holds that list against the plan recorder on the
CPU.  Every case below is one row of the list (test_every_recorded_pass_is_a_case_or_a_named_duplicate), run through
helpers.ConvPassDriver with the classes test_gpu_conv_exact.py runs on (helpers.ConvCase, ConvOps, ConvRun, conv_exact_run: same
operands, same sentinel buffer one 16-byte chunk wider than the pass needs, same column checks).  What the 3-D cases there do not
reach and these do: more than one column block of the 256-column tiles (Cn = 512, 1024, 1536: blockIdx.y up to 5), four parity
classes with 1, 2, 2 and 4 taps, K up to 9 * 1024 = 9216 per class (forward) and 4 * 1536 = 6144 (ConvTranspose2d 1536 -> 256), the
element-wise staged first layer with 128 columns, and the fused [residual | unit0] GEMM of the strided residual units as ONE layer
of two parameter pairs.

No 2-D pass writes a split output (out2): ctseg_conv_split_ok is 0 off the stem and the stride-2 halo kernels, so a fused down unit
writes ONE buffer 2 * C columns wide and the next passes read its halves as column slices.  Both halves are held to the two
separate float64 convolutions (residual, unit0) the GEMM stands for.

Oracle A, exact integers (the method of test_gpu_conv_exact.py).  x and dY in {-1, 0, 1} with P(nonzero) = 2/3, integer bias in
[-2, 2], weights in {-1, 0, 1} with P(nonzero) = wd = min(2/3, 1800 / (K * 2/3)), K the longest class's taps x gathered channels:
the variance of a sum is about K * 2/3 * wd <= 1800 (sigma <= 42.5), which keeps a few 10^5 outputs inside +-256.  That is derived;
the maxima below are computed.  `max |ref| <= 256` (bf16) / 2048 (fp16) / < 2^24 (fp32) and `nonzero share > 85 %` are ASSERTED on the
float64 reference of every case (conditions, not tolerances).  The first layer multiplies 9 products: its weights are all nonzero
(wd = 1), which gives 86.1 % nonzero outputs.
Reference maxima and nonzero shares, computed on the CPU (forward / input gradient; "-": the layer has none):
  fused s2 1->128 11, 86.1 % / -;  conv 64->64 67, 97.3 % / 58, 97.4 %;  fused s2 64->256 69, 97.4 % / 89, 97.3 %
  conv 128->128 116, 98.1 % / 115, 98.1 %;  fused s2 128->512 109, 98.2 % / 125, 98.0 %;  conv 256->256 146, 98.7 % / 152, 98.7 %
  fused s2 256->1024 169, 98.7 % / 189, 98.6 % (wd 0.659);  conv 512->512 (wd 0.586) 196, 99.0 % / duplicate
  k=1 512->1024 76, 97.4 % / 94, 98.1 %;  conv 512->1024 190, 99.0 % (wd 0.586) / 202, 99.0 % (wd 0.293)
  conv 1024->1024 (wd 0.293) 196, 99.0 % / 190, 99.0 %;  convT 1536->256 179, 98.6 % (wd 0.439) / 152, 98.7 %
  convT 512->128 134, 98.0 % / 103, 98.2 %;  convT 256->64 85, 97.2 % / 75, 97.4 %;  convT 128->10 63, 96.2 % / 26, 93.6 %
  largest of all: 202; THIN cases: at most 128, at least 93.0 % nonzero; wd = 2/3 where none is given
  large-magnitude runs: 311 .. 1145;  fp32 storage runs: 641 .. 2511
Large-magnitude bf16 run (operands in [-4, 4], [-16, 16] on the 9-product first layer; stored value = ref.to(bfloat16), round to
nearest even), one per distinct tile and pass; fp16 on every forward and input-gradient case; fp32 storage (integers in [-4, 4]) on
the tiles that take it: in fp32 every 2-D layer runs "generic 128x128" (up to 12 column blocks), "generic 128x64" or "generic
256x16".

Oracle B, normal-valued operands, per element, one case per distinct (name, classes) and pass plus the long-K layers:
|out - y64| <= u * |y64| + 16 * e32 (helpers.elem_bound, unchanged).
Measured on an MI355X, worst error / bound over the elements of the case:
  bf16 (the ulp term dominates the bound: a correctly rounded store alone reaches 1.0 just above a power of two), forward:
    fused s2 1->128 0.993;  conv 64->64 0.993;  conv 128->128 0.993;  fused s2 256->1024 0.991;  conv 1024->1024 (K 9216) 0.988
    convT 1536->256 (K 6144) 0.984;  convT 512->128 0.991;  convT 256->64 0.986;  convT 128->10 0.984
  input gradient:
    of convT 128->10 0.992;  conv 64->64 0.987;  conv 128->128 0.990;  of convT 1536->256 0.993;  conv 1024->1024 (K 9216) 0.992
    of fused s2 256->1024 0.988;  of fused s2 128->512 0.984;  of fused s2 64->256 0.990
  e32 = 2.0e-07 .. 3.7e-06 at max |y| of 1.2 .. 6.3: 16 * e32 is at most 6e-05 beside an ulp term of up to 2.5e-02, so the long-K
  layers sit where the short ones do and no case needed more than the factor 16; none exceeds 1.

Shapes: two samples, (2, 13, 19) for stride-1 layers and as the input of the transposed ones (247 rows: ragged in the 192- and the
128-row tile, two tiles per sample and class), (2, 28, 30) as the input of the stride-2 layers (210 output rows); one sample for the
layers of 9 * 1024 gathered values per output.  THIN: per tile one case with an extent of 1 along x or y.

Duplicates not run (same pass name, tile, classes and number of column blocks as a tested row; the wider one is tested):
  * conv 10(16) -> 10, forward and input gradient ("generic 256x16", one class, one block): "2-D 16->16" of test_gpu_conv_exact.py is
    the wider layer; its addend and fp32 output are extras (test_gpu_conv_extras.py);
  * input gradient of conv 512 -> 512 ("generic ring 192x256", one class, two blocks, K = 4608): the input gradient of the bottom
    512 -> 1024 k = 3 conv is the same pass with K = 9216;
  * the up path's stride-1 unit convs 256 -> 256, 128 -> 128, 64 -> 64: the same layers as the down path's unit1 convs.

Not covered, with the reason the library gives:
  * a split output on any 2-D pass: ctseg_conv_split_ok is 0 off the stem and stride-2 halo kernels (asserted on the fused cases);
  * the stem, x/z-halo, streamed-weight, stride-2 and 8-class families: they need 27 taps, 4 rows along z or 8 classes; the CPU test
    of the recorded names asserts that no 2-D pass is given one;
  * the input gradient of the first layer: built without an input-gradient operand (need_dgrad=False);
  * CTSEG_MAX_WG: it does not size the grid of the generic tiles and the ring kernel;
  * statistics, addend, backward statistics on more than one column block: test_gpu_conv_extras.py (the 64 -> 512 cases);
  * the weight gradients: the 2-D section of test_gpu_wgrad.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd._native import BF16, F16, F32  # noqa: E402
from helpers import (ACT_SENTINEL, G16, G64, G128, RING128, RING256, ULP, ConvCase, ConvOps, ConvRun, conv_exact_run,  # noqa: E402
                     elem_bound)
from reference_ops import conv_dgrad, conv_fwd, conv_module  # noqa: E402
from unet2d_passes import UNET2D_PASSES  # noqa: E402

DEV = "cuda:0"
S1, S2, L1 = (2, 13, 19), (2, 28, 30), (1, 13, 19)


def _wd(K):
    """P(nonzero) of the {-1, 0, 1} weights for sums of K products with x at 2/3: K * 2/3 * wd <= 1800"""
    return min(2 / 3, 1800.0 / (K * 2 / 3))


class _Case2D(ConvCase):
    """a row of UNET2D_PASSES; ``fused``: the [residual | unit0] GEMM (cout = 2 * C, two parameter pairs); K: see _wd"""

    def __init__(self, name, pas, family, kind, cin, cout, shape, dt=BF16, k=3, fused=False, g_ld=None, wide=4, wd=None):
        self.fused = fused
        taps = {"conv": k * k, "conv_s2": k * k, "convT": 4}[kind] if pas == "fwd" else {"conv": k * k, "conv_s2": 4, "convT": 9}[kind]
        K = taps * (cin if pas == "fwd" else cout)
        super().__init__(name, pas, family, kind, cin, cout, shape, dt, k, wd if wd is not None else (1.0 if cin == 1 else _wd(K)),
                         g_ld=g_ld, wide=wide)
        self.K = K

    def with_dt(self, dt, family=None):
        return _Case2D(self.name, self.pas, family or self.family, self.kind, self.cin, self.cout, self.shape, dt, self.k, self.fused,
                       self.g_ld, self.wide, self.wd)

    @property
    def row(self):
        """key of the case's row in UNET2D_PASSES"""
        return (self.pas, self.kind, self.cin, self.cout, self.k, self.fused)

    @property
    def blocks(self):
        """column blocks of the pass's tile (grid.y)"""
        bn = int(self.family.rsplit("x", 1)[1])
        return -(-(self.cout if self.pas == "fwd" else self.cin) // bn)


class _FusedOps(ConvOps):
    """ConvOps of a fused down unit: the operands are drawn as one cin -> 2 * C layer; the device gets them as the two modules
    (residual: output channels [0, C), unit0: [C, 2 * C)) and the references are the two separate convolutions"""
    _cache = {}

    def module(self, case):
        C = case.cout // 2
        mods = [conv_module(case.kind, case.cin, C, case.k, case.dims) for _ in range(2)]
        with torch.no_grad():
            for i, m in enumerate(mods):
                m.weight.copy_(self.w[i * C:(i + 1) * C])
                m.bias.copy_(self.b[i * C:(i + 1) * C])
        return mods

    def ref(self, pas, f32=False):
        key = (pas, f32)
        if key not in self._ref:
            x, w, b, gy = ((t if f32 else t.double()) for t in (self.x, self.w, self.b, self.gy))
            C = w.shape[0] // 2
            with torch.no_grad():
                if pas == "fwd":
                    self._ref[key] = torch.cat([conv_fwd(self.kind, self.k, x, w[h], b[h]) for h in (slice(0, C), slice(C, 2 * C))], 1)
                else:
                    self._ref[key] = sum(conv_dgrad(self.kind, self.k, gy[:, h], w[h], self.x.shape) for h in (slice(0, C), slice(C, 2 * C)))
        return self._ref[key]


def _ops(case, mode):
    return (_FusedOps if case.fused else ConvOps).of(case, mode)


def _exact(case, mode):
    """helpers.conv_exact_run (which asserts the storage type's exactness condition on the reference) with the nonzero share asserted
    before the pass runs -> (ConvRun, float64 reference)"""
    ops = _ops(case, mode)
    nz = float((ops.ref(case.pas) != 0).double().mean())
    print(f"{case.id} [{mode}]: K {case.K}, wd {case.wd:.3f}, nonzero {100 * nz:.1f} %, {case.blocks} column block(s)")
    assert nz > 0.85, ("a sparse draw could hide a dropped tap", nz)
    run, ref = conv_exact_run(case, mode, ops=ops)
    if case.fused:
        assert nat.lib().ctseg_conv_split_ok(run.drv.desc) == 0 and not run.drv.desc.out2, "no split output on a generic / ring pass"
    assert len(run.drv.mods) == (2 if case.fused else 1)
    return run, ref


# ---- case matrix: rows of UNET2D_PASSES -------------------------------------------------------------------------------------------
C = _Case2D
FWD = [
    C("fused s2 1->128", "fwd", G128, "conv_s2", 1, 128, S2, fused=True, wide=16),
    C("conv 64->64", "fwd", G64, "conv", 64, 64, S1),
    C("fused s2 64->256", "fwd", RING256, "conv_s2", 64, 256, S2, fused=True),
    C("conv 128->128", "fwd", RING128, "conv", 128, 128, S1),
    C("fused s2 128->512", "fwd", RING256, "conv_s2", 128, 512, S2, fused=True),
    C("conv 256->256", "fwd", RING256, "conv", 256, 256, S1),
    C("fused s2 256->1024", "fwd", RING256, "conv_s2", 256, 1024, S2, fused=True),
    C("conv 512->512", "fwd", RING256, "conv", 512, 512, S1),
    # the bottom unit gathers the lower 512 columns of the 1536-wide skip concat
    C("k=1 512->1024", "fwd", RING256, "conv", 512, 1024, S1, k=1, g_ld=1536),
    C("conv 512->1024", "fwd", RING256, "conv", 512, 1024, L1, g_ld=1536),
    C("conv 1024->1024", "fwd", RING256, "conv", 1024, 1024, L1),
    C("convT 1536->256", "fwd", RING256, "convT", 1536, 256, S1),
    C("convT 512->128", "fwd", RING128, "convT", 512, 128, S1),
    C("convT 256->64", "fwd", G64, "convT", 256, 64, S1),
    C("convT 128->10", "fwd", G16, "convT", 128, 10, S1),
]
DGRAD = [
    C("of convT 128->10", "dgrad", G128, "convT", 128, 10, S1),
    C("conv 64->64", "dgrad", G64, "conv", 64, 64, S1),
    C("of convT 256->64", "dgrad", RING256, "convT", 256, 64, S1),
    C("conv 128->128", "dgrad", RING128, "conv", 128, 128, S1),
    C("of convT 512->128", "dgrad", RING256, "convT", 512, 128, S1),
    C("conv 256->256", "dgrad", RING256, "conv", 256, 256, S1),
    C("of convT 1536->256", "dgrad", RING256, "convT", 1536, 256, S1),
    C("conv 1024->1024", "dgrad", RING256, "conv", 1024, 1024, L1),
    C("conv 512->1024", "dgrad", RING256, "conv", 512, 1024, L1),
    C("k=1 512->1024", "dgrad", RING256, "conv", 512, 1024, S1, k=1),
    C("of fused s2 256->1024", "dgrad", RING256, "conv_s2", 256, 1024, S2, fused=True),
    C("of fused s2 128->512", "dgrad", RING128, "conv_s2", 128, 512, S2, fused=True),
    C("of fused s2 64->256", "dgrad", G64, "conv_s2", 64, 256, S2, fused=True),
]
# per tile one case with an extent of 1 along x or y
THIN = [
    C("thin convT 128->10", "fwd", G16, "convT", 128, 10, (1, 1, 37)),
    C("thin conv 64->64", "fwd", G64, "conv", 64, 64, (1, 37, 1)),
    C("thin, of convT 128->10", "dgrad", G128, "convT", 128, 10, (1, 1, 37)),
    C("thin conv 128->128", "fwd", RING128, "conv", 128, 128, (1, 1, 37)),
    C("thin fused s2 128->512", "fwd", RING256, "conv_s2", 128, 512, (1, 2, 74), fused=True),
    C("thin, of fused s2 256->1024", "dgrad", RING256, "conv_s2", 256, 1024, (1, 74, 2), fused=True),
]
ALL = FWD + DGRAD + THIN
# fp32 storage: every layer lands on a generic tile; the wide ones, the 4-class ones and the element-wise first layer
F32_CASES = [c.with_dt(F32, fam) for c, fam in (
    (FWD[0], G128), (FWD[6], G128), (FWD[11], G128), (FWD[13], G64), (FWD[14], G16), (DGRAD[6], G128), (DGRAD[10], G128))]
# one case per distinct tile and pass (large-magnitude run) ...
WIDE = [FWD[0], FWD[1], FWD[3], FWD[4], FWD[14], DGRAD[0], DGRAD[1], DGRAD[3], DGRAD[4]]
# ... and per distinct (name, classes) and pass, plus the long-K layers (normal-valued run)
NORMAL = [FWD[0], FWD[1], FWD[3], FWD[6], FWD[10], FWD[11], FWD[12], FWD[13], FWD[14],
          DGRAD[0], DGRAD[1], DGRAD[3], DGRAD[6], DGRAD[7], DGRAD[10], DGRAD[11], DGRAD[12]]
DUPLICATES = {
    ("fwd", "conv", 10, 10, 3, False): "generic 256x16, one class, one block: '2-D 16->16' of test_gpu_conv_exact.py is wider",
    ("dgrad", "conv", 10, 10, 3, False): "generic 256x16, one class, one block: '2-D 16->16' of test_gpu_conv_exact.py is wider",
    ("dgrad", "conv", 512, 512, 3, False): "ring 192x256, one class, two blocks: the input gradient of conv 512->1024 has K = 9216",
}


def _ids(cases):
    return [c.id for c in cases]


def test_every_recorded_pass_is_a_case_or_a_named_duplicate():
    table = {}
    for pas, _, kind, cin, cout, k, fused, Cg, Cn, nclass, name in UNET2D_PASSES:
        if pas != "wgrad":
            assert table.setdefault((pas, kind, cin, cout, k, fused), (name, Cn, nclass)) == (name, Cn, nclass)
    cases = {c.row: c for c in FWD + DGRAD}
    assert set(cases) | set(DUPLICATES) == set(table) and not set(cases) & set(DUPLICATES)
    for c in ALL:
        name, Cn, nclass = table[c.row]
        assert c.family == name and Cn == (c.cout if c.pas == "fwd" else c.cin), c.id
        assert nclass == (4 if (c.kind, c.pas) in (("convT", "fwd"), ("conv_s2", "dgrad")) else 1), c.id
    # what the module is for: several column blocks of both 256-column tiles' kernel, four classes on every tile, the long K
    assert {c.blocks for c in FWD if c.family == RING256} >= {1, 2, 4} and {c.blocks for c in DGRAD if c.family == RING256} >= {1, 2, 4, 6}
    for group in (WIDE, NORMAL, THIN):
        assert {c.family for c in group} == {G16, G64, G128, RING128, RING256}
    assert {(table[c.row][0], table[c.row][2], c.pas) for c in NORMAL} == {(v[0], v[2], r[0]) for r, v in table.items() if r not in DUPLICATES}


# ---- Oracle A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_exact_bf16(monkeypatch, case):
    case.setenv(monkeypatch)
    run, ref = _exact(case, "unit")
    run.check_columns(ref, "bf16, operands in {-1, 0, 1}")


FP16 = [c.with_dt(F16) for c in FWD + DGRAD]


@pytest.mark.parametrize("case", FP16, ids=_ids(FP16))
def test_exact_fp16(monkeypatch, case):
    case.setenv(monkeypatch)
    run, ref = _exact(case, "unit")
    run.check_columns(ref, "fp16, operands in {-1, 0, 1}")


@pytest.mark.parametrize("case", F32_CASES, ids=_ids(F32_CASES))
def test_exact_fp32_storage(monkeypatch, case):
    case.setenv(monkeypatch)
    run, ref = _exact(case, "wide")
    assert run.out.t.dtype == torch.float32
    run.check_columns(ref, "fp32 storage, operands in [-4, 4]")


@pytest.mark.parametrize("case", WIDE, ids=_ids(WIDE))
def test_bf16_store_rounds_to_nearest_even(monkeypatch, case):
    """operands in [-4, 4] ([-16, 16] on the first layer's 9 products): the fp32 result is the exact integer, outside +-256, and the
    stored value must be its round-to-nearest-even bf16"""
    case.setenv(monkeypatch)
    run, ref = _exact(case, "wide")
    assert float(ref.abs().max()) < 2.0 ** 24
    want = ref.to(torch.bfloat16).double()
    assert float(ref.abs().max()) > 256 and bool((want != ref).any()), "the case does not leave the exact range"
    run.check_columns(want, "bf16, large magnitudes, rounded to nearest even")


# ---- Oracle B ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NORMAL, ids=_ids(NORMAL))
def test_normal_operands_per_element(monkeypatch, case):
    """|out - y64| <= u * |y64| + 16 * e32 for EVERY element (helpers.elem_bound)"""
    case.setenv(monkeypatch)
    ops = _ops(case, ("randn", case.dt))
    y64, y32 = (y.unsqueeze(-1) for y in (ops.ref(case.pas), ops.ref(case.pas, f32=True)))
    bound, e32 = elem_bound(y64, y32, case.dt)
    run = ConvRun(case, ops)
    T = run.buffer()
    got = T[..., :run.Cn].permute(0, 4, 1, 2, 3)
    ratio = float(((got - y64).abs() / bound).max())
    print(f"{case.id}: K {case.K}, worst error / bound {ratio:.3f} (e32 {e32:.3e}, u {ULP[case.dt]:.1e}, max |y| {float(y64.abs().max()):.2f})")
    assert bool(((got - y64).abs() <= bound).all()), ("per-element bound", ratio)
    assert bool((T[..., run.Cn:run.Cs] == 0).all()) and bool((T[..., run.Cs:] == ACT_SENTINEL).all())
