"""GPU: the forward and input-gradient passes of ctseg_conv_igemm, every kernel family, element by element.

Every case names the kernel family (or generic / ring tile) it is written for; helpers.ConvPassDriver asserts ctseg_conv_pass_name of
the recorded descriptor before the pass runs.  The existing conv tests bound max |error| / max |reference| by 2.5e-2 (16-bit) or
compare two kernels with each other; here every stored ELEMENT is held to a float64 CPU convolution (conv_fwd / conv_dgrad of
reference_ops.py).

Oracle A, exact.  Operands are small integers, so every product and every partial sum is an integer far below 2^24: the fp32
accumulator holds the exact result in any summation order, and the stored value is exact whenever the storage type holds that integer.
  * bf16 storage: x, w, dY uniform in {-1, 0, 1} (P(nonzero) = 2/3; the 256 -> 256 layer draws its weights with P(nonzero) = 1/3),
    integer bias in [-2, 2] on the forward.  bf16 holds every integer up to 256: `ref.abs().max() <= 256` is ASSERTED on the float64
    reference of every case (a condition, not a tolerance), then torch-equality of every element is required.  Reference maxima,
    computed on the CPU: 64 -> 64 126 (forward) / 131 (input gradient), 128 -> 128 175 / 187, 128 -> 256 176, 256 -> 256 (weights 1/3)
    165, 256 -> 128 input gradient 164, ConvTranspose 384 -> 64 178 / 130, 256 -> 64 149, stride-2 64 -> 256 input gradient 145,
    32 -> 128 90 / 96, every other case below 140; largest of all: 187.  More than 93 % of the outputs are nonzero in every 3 x 3 x 3
    case with at least 16 gathered channels (more than 96.5 % from 64 channels up), 88 % on the stem (27 products), 85 % at k = 1.
  * fp16 storage (forward and input gradient are all it has): the same operands, every case of the two main tables, cap +-2048.
  * fp32 storage, and fp32 output under bf16 storage (out_f32; the families test_fp32_output_under_bf16_storage names: the x-column
    halo pass in forward tap order, with 16-byte and with 12-wide rows, and the generic 256x16 tile): integers in [-4, 4], condition
    |y| < 2^24 (asserted).
  * one large-magnitude bf16 run per family and pass, operands in [-4, 4]: results reach 540 .. 1900, far outside +-256, and the
    stored value must equal ref.to(torch.bfloat16): round to nearest even, as f2bf (ctseg_dev.h) documents.  The stem multiplies 27
    products only (|y| <= 150 with [-4, 4]): its run draws from [-16, 16] (products <= 256, |y| <= 1928).
Every run writes into an output buffer the test filled with a sentinel (-12288, exact in all three types) whose rows are one 16-byte
chunk wider than the pass needs: columns [0, Cn) exact, columns [Cn, Cn_store) zero ("pad columns are zeros", ctseg_hip.h), columns
[Cn_store, o_ld) still the sentinel.  Persistent kernels (every family but the generic / ring tiles, whose grid CTSEG_MAX_WG does not
size) run under CTSEG_MAX_WG unset, "1" and "3".  test_column_slices_and_replay writes the output as a column slice at c0 = 16 bytes
of a wider buffer and gathers the operand from a column slice between columns that hold 3: neighbours keep the sentinel, the bytes
equal the dense run (rows exactly Cn_store wide); the recorded program, run again over a re-poisoned buffer, writes the same bytes.
No launch refused a sliced layout.

Oracle B, normal-valued operands, per element (one case per family / tile and pass): randn operands rounded to the storage type,
weights scaled by fan-in^-1/2, fp32 bias; EVERY element must satisfy |out - y64| <= u * |y64| + 16 * e32, with e32 the largest
|y32 - y64| of torch's float32 evaluation of the same operands (measured per case on the CPU), 16 the allowance for the kernels'
longer sum chains (test_gpu_conv_extras.py), u one unit in the last place of the stored type (2^-8 bf16, 2^-10 fp16, 0 for fp32
values): one ulp, not half, because a sum-order difference in fp32 can cross a rounding boundary.
Measured on an MI355X, worst error / bound over the elements of the case (forward / input gradient):
  bf16 (the ulp term dominates the bound: a correctly rounded store alone reaches 1.0 just above a power of two)
    x-column halo 0.987 / 0.984;  halo 0.987 / 0.984;  up 0.992 / 0.984;  stem 0.993 / -;  streamed-weight halo 0.992 / 0.992, 8-class
    0.992 / 0.992;  stride-2 halo 0.992 / 0.988;  stride-2 register-weight 0.993 / 0.991;  many-channel 8-class 0.994 / 0.993
    generic 256x16 0.986 / 0.993;  256x32 0.992 / 0.986;  128x64 0.988 / 0.992;  128x128 0.993 / 0.989;  192x256 0.991 / 0.991
    ring 192x128 0.993 / 0.988;  ring 192x256 0.992 / 0.991
  fp32 values (u = 0: the bound is 16 * e32, e32 = 9.5e-07 .. 3.9e-06 at max |y| of 3 .. 5)
    halo fp32 0.062 / 0.072;  generic fp32 128x64 0.070 / 0.114;  fp32 output: x-column halo 0.049, generic 256x16 0.085

Case matrix.  Shapes are those of STATS_CASES / DGRAD_ADD_CASES / BST_CASES (test_gpu_conv_extras.py) and of the ring and 8-class
tables of test_gpu_parity.py: two samples, ragged on every tiled axis; none was grown.  Added: the input gradients those tables lack
(stride-2 halo as the gradient of ConvTranspose 64 -> 16 and of 64 -> 10 with 12-wide dY; the gradient of ConvTranspose 128 -> 32 has
32 gathered channels, which conv_down_halo_eligible turns down: it is the stride-2 register-weight kernel's and is pinned as such;
many-channel 8-class as the gradient of stride-2 64 -> 256; ring 192x256 as the gradient of ConvTranspose 384 -> 64; x-column halo
with 12-wide dY), ragged last chunks of every generic tile (pad columns), one 2-D layer and one k = 1 layer in both passes (the
selector names "generic 256x16" for all four), and per family a case with an extent of 1, a 3 x 3 cross-section or an odd long axis
(DEGENERATE; the halo kernels need 4 rows along z, the streamed kernels 2048 rows: 1 x 3 x 683).  16-bit storage reaches the "halo"
kernel only with CTSEG_NO_HALO_X set (conv_halo_x_eligible comes first): those cases set it.

PERMUTED adds the tile orders those shapes do not reach (the (z, x, y) order of the many-channel 8-class, the 8-class streamed-weight
and the stride-2 halo kernels; z and y as the 1-deep axis of the stride-2 register-weight kernel), uncapped and under CTSEG_MAX_WG=1;
tests/test_abi_exports.py pins which order each of those row grids gets.  Reference maxima of the six cases, in table order: 156, 134,
87, 47, 86, 93.

Not covered, with the reason the library gives:
  * the stem's input gradient: the layer is the network's first, GemmLayer builds it without an input-gradient operand
    (need_dgrad=False); test_every_family_and_tile_has_a_forward_and_an_input_gradient_case lists the exemption;
  * fp32 output on anything but the x-column halo pass (forward taps), "halo" (which 16-bit storage reaches behind CTSEG_NO_HALO_X
    only; one case) and the generic tiles: every other family's *_eligible turns a pass with out_f32 down (the logits are the only
    fp32 tensor under 16-bit storage), and tile_rows_for keeps it off the 192-row tiles;
  * fp32 storage on anything but "halo" and the generic 256x16 / 256x32 / 128x64 / 128x128 tiles: all other families are is16() only;
  * the stem's operand as a column slice: conv_stem_eligible wants g_ld == 1 (a single-channel volume), so only its output is sliced;
    12-wide rows are rows of their own by construction (no slice);
  * statistics, addend, split output, backward statistics, operand normalisation: test_gpu_conv_extras.py (per family, by name);
  * fp16 under CTSEG_MAX_WG caps and in the degenerate shapes: the cap and the tile walk are storage-independent code, run in bf16.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd._native import BF16, F16, F32  # noqa: E402
from helpers import (ACT_SENTINEL, CAP_IDS, CAPS, DOWN_HALO, DOWN_R, G16, G32, G64, G128, G256, HALO, HALO_SW, HALO_X, RING128, RING256,  # noqa: E402
                     STEM, ULP, UP, UP8, elem_bound)
from helpers import ConvCase as _Case, ConvOps as _Ops, ConvRun as _Run, conv_exact_run as _exact  # noqa: E402

DEV = "cuda:0"
NO_X = {"CTSEG_NO_HALO_X": "1"}      # conv_halo_x_eligible turns every pass down: 16-bit storage on the "halo" kernel


# ---- case matrix -------------------------------------------------------------------------------------------------------------
S = (2, 7, 9, 11)          # the generic tiles' volume: 693 rows per sample, ragged in every tile
C = _Case
FWD = [
    C("halo_x 16->16", "fwd", HALO_X, "conv", 16, 16, (2, 9, 11, 13)),
    C("halo_x 32->32", "fwd", HALO_X, "conv", 32, 32, (2, 5, 9, 13)),
    C("halo_x 16->10", "fwd", HALO_X, "conv", 16, 10, (2, 7, 11, 13)),
    C("halo_x 10(16)->10 12-wide rows", "fwd", HALO_X, "conv", 10, 10, (2, 7, 11, 13), g_ld=12, o_ld=12, cg=16),
    C("halo 16->16", "fwd", HALO, "conv", 16, 16, (2, 9, 11, 13), env=NO_X),
    C("halo 32->24", "fwd", HALO, "conv", 32, 24, (2, 5, 9, 13), env=NO_X),
    C("up 64->10", "fwd", UP, "convT", 64, 10, (2, 7, 9, 5)),
    C("up 64->10 12-wide out", "fwd", UP, "convT", 64, 10, (2, 7, 9, 5), o_ld=12),
    C("up 32->16", "fwd", UP, "convT", 32, 16, (2, 7, 9, 5)),
    C("stem 1->32", "fwd", STEM, "conv_s2", 1, 32, (2, 10, 12, 20), wide=16),
    C("stem 1->64", "fwd", STEM, "conv_s2", 1, 64, (2, 10, 12, 10), wide=16),
    C("halo_sw 64->64", "fwd", HALO_SW, "conv", 64, 64, (2, 9, 20, 13)),
    C("halo_sw 8-class 128->32", "fwd", HALO_SW, "convT", 128, 32, (2, 9, 20, 12)),
    C("down_halo 16->64", "fwd", DOWN_HALO, "conv_s2", 16, 64, (2, 36, 20, 24)),
    C("down_r 32->128", "fwd", DOWN_R, "conv_s2", 32, 128, (2, 18, 40, 24)),
    C("up8 256->64", "fwd", UP8, "convT", 256, 64, (2, 9, 20, 12)),
    C("up8 384->64", "fwd", UP8, "convT", 384, 64, (1, 9, 20, 12)),
    C("generic 256x16 40->12", "fwd", G16, "conv", 40, 12, S),
    C("generic 256x32 40->24", "fwd", G32, "conv", 40, 24, S),
    C("generic 128x64 40->48", "fwd", G64, "conv", 40, 48, S),
    C("generic 128x128 40->96", "fwd", G128, "conv", 40, 96, S),
    C("generic 192x256 40->160", "fwd", G256, "conv", 40, 160, S),
    # the same tiles with a ragged last chunk: pad columns [Cn, Cn_store) to zero
    C("generic 256x32 40->20", "fwd", G32, "conv", 40, 20, S),
    C("generic 128x64 40->44", "fwd", G64, "conv", 40, 44, S),
    C("generic 128x128 40->90", "fwd", G128, "conv", 40, 90, S),
    C("generic 192x256 40->150", "fwd", G256, "conv", 40, 150, S),
    C("ring 192x128 128->100", "fwd", RING128, "conv", 128, 100, S),
    C("ring 192x128 128->128", "fwd", RING128, "conv", 128, 128, S),
    C("ring 192x256 128->256", "fwd", RING256, "conv", 128, 256, (2, 7, 9, 5)),
    C("ring 192x256 256->256", "fwd", RING256, "conv", 256, 256, (1, 8, 8, 6), wd=1 / 3),
    C("2-D 16->16", "fwd", G16, "conv", 16, 16, (2, 33, 45)),
    C("k=1 16->16", "fwd", G16, "conv", 16, 16, S, k=1),
]
DGRAD = [
    C("halo_x 16->16", "dgrad", HALO_X, "conv", 16, 16, (2, 9, 11, 13)),
    C("halo_x 32->32", "dgrad", HALO_X, "conv", 32, 32, (2, 5, 9, 13)),
    C("halo_x 16->10, 12-wide dY", "dgrad", HALO_X, "conv", 16, 10, (2, 7, 11, 13), g_ld=12),
    C("halo 16->16", "dgrad", HALO, "conv", 16, 16, (2, 9, 11, 13), env=NO_X),
    C("halo_sw 64->64", "dgrad", HALO_SW, "conv", 64, 64, (2, 9, 20, 13)),
    C("halo_sw 8-class, of 32->128 s2", "dgrad", HALO_SW, "conv_s2", 32, 128, (2, 18, 40, 24)),
    C("up, of 16->64 s2", "dgrad", UP, "conv_s2", 16, 64, (2, 8, 10, 12)),
    C("down_halo, of convT 64->16", "dgrad", DOWN_HALO, "convT", 64, 16, (2, 18, 10, 13)),
    C("down_halo, of convT 64->10, 12-wide dY", "dgrad", DOWN_HALO, "convT", 64, 10, (2, 18, 10, 13), g_ld=12),
    C("down_r, of convT 128->32", "dgrad", DOWN_R, "convT", 128, 32, (2, 9, 20, 12)),
    C("up8, of 64->256 s2", "dgrad", UP8, "conv_s2", 64, 256, (2, 18, 40, 24)),
    C("generic 256x16 16->40", "dgrad", G16, "conv", 16, 40, S),
    C("generic 256x32 24->40", "dgrad", G32, "conv", 24, 40, S),
    C("generic 128x64 40->96", "dgrad", G64, "conv", 40, 96, S),
    C("generic 128x128 96->40", "dgrad", G128, "conv", 96, 40, S),
    C("generic 192x256 160->40", "dgrad", G256, "conv", 160, 40, S),
    C("ring 192x128 128->128", "dgrad", RING128, "conv", 128, 128, S),
    C("ring 192x256, of convT 384->64", "dgrad", RING256, "convT", 384, 64, (1, 5, 6, 4)),
    C("ring 192x256 256->128", "dgrad", RING256, "conv", 256, 128, (1, 9, 7, 6)),
    C("2-D 16->16", "dgrad", G16, "conv", 16, 16, (2, 33, 45)),
    C("k=1 16->16", "dgrad", G16, "conv", 16, 16, S, k=1),
]
# extents of 1, 3 x 3 cross-sections, odd long axes (the halo kernels need 4 rows along z, the streamed kernels 2048 rows)
DEGENERATE = [
    C("halo_x thin", "fwd", HALO_X, "conv", 16, 16, (1, 1, 3, 37)),
    C("halo_x thin", "dgrad", HALO_X, "conv", 16, 16, (1, 1, 3, 37)),
    C("halo thin", "fwd", HALO, "conv", 16, 16, (1, 3, 3, 37), env=NO_X),
    C("up thin", "fwd", UP, "convT", 64, 10, (1, 1, 3, 7)),
    C("up thin, of 16->64 s2", "dgrad", UP, "conv_s2", 16, 64, (1, 2, 6, 14)),
    C("stem thin", "fwd", STEM, "conv_s2", 1, 32, (1, 2, 6, 14), wide=16),
    C("halo_sw 3x3 column", "fwd", HALO_SW, "conv", 64, 64, (1, 229, 3, 3)),
    C("halo_sw one slice", "dgrad", HALO_SW, "conv", 64, 64, (1, 1, 47, 45)),
    C("halo_sw 8-class one slice", "fwd", HALO_SW, "convT", 128, 32, (1, 1, 3, 683)),
    C("down_halo one slice", "fwd", DOWN_HALO, "conv_s2", 16, 64, (1, 2, 6, 1366)),
    C("down_halo one slice, of convT 64->16", "dgrad", DOWN_HALO, "convT", 64, 16, (1, 1, 3, 683)),
    C("down_r one slice", "fwd", DOWN_R, "conv_s2", 32, 128, (1, 2, 6, 1366)),
    C("down_r one slice, of convT 128->32", "dgrad", DOWN_R, "convT", 128, 32, (1, 1, 3, 683)),
    C("up8 one slice", "fwd", UP8, "convT", 256, 64, (1, 1, 3, 683)),
    C("up8 one slice, of 64->256 s2", "dgrad", UP8, "conv_s2", 64, 256, (1, 2, 6, 1366)),
    C("generic 128x128 thin", "fwd", G128, "conv", 40, 96, (1, 1, 3, 37)),
    C("generic 128x64 thin", "dgrad", G64, "conv", 40, 96, (1, 1, 3, 37)),
    C("ring 192x128 thin", "fwd", RING128, "conv", 128, 128, (1, 3, 3, 37)),
    C("ring 192x256 thin", "dgrad", RING256, "conv", 256, 128, (1, 1, 3, 37)),
]
# the permuted tile orders the tables above do not reach: (z, x, y) on the many-channel 8-class kernel (both passes), on the 8-class
# streamed-weight halo kernel and on the stride-2 halo kernel with 12-wide dY, and the stride-2 register-weight kernel with z / with y
# as its 1-deep axis.  One sample of 2.2k-3.1k rows; only CTSEG_MAX_WG=1 makes one workgroup walk several permuted tiles
PERMUTED = [
    C("up8 zxy", "fwd", UP8, "convT", 256, 64, (1, 16, 16, 9)),
    C("up8 zxy, of 64->256 s2", "dgrad", UP8, "conv_s2", 64, 256, (1, 32, 32, 18)),
    C("halo_sw 8-class zxy", "fwd", HALO_SW, "convT", 128, 32, (1, 16, 16, 12)),
    C("down_halo zxy, of convT 64->10, 12-wide dY", "dgrad", DOWN_HALO, "convT", 64, 10, (1, 16, 16, 12), g_ld=12),
    C("down_r 1-deep z", "fwd", DOWN_R, "conv_s2", 32, 128, (1, 16, 32, 34)),
    C("down_r 1-deep y", "fwd", DOWN_R, "conv_s2", 32, 128, (1, 16, 34, 32)),
]
ALL = FWD + DGRAD + DEGENERATE
PERSISTENT = [c for c in ALL if c.persistent]
TILED = [c for c in ALL if not c.persistent]
F32_CASES = [
    C("halo fp32 16->16", "fwd", HALO, "conv", 16, 16, (2, 9, 11, 13), F32),
    C("halo fp32 16->10", "fwd", HALO, "conv", 16, 10, (2, 7, 11, 13), F32),
    C("halo fp32 8->8", "fwd", HALO, "conv", 8, 8, (2, 7, 11, 13), F32),
    C("halo fp32 16->16", "dgrad", HALO, "conv", 16, 16, (2, 9, 11, 13), F32),
    C("generic fp32 256x16 24->12", "fwd", G16, "conv", 24, 12, S, F32),
    C("generic fp32 128x64 24->48", "fwd", G64, "conv", 24, 48, S, F32),
    C("generic fp32 128x128 24->96", "fwd", G128, "conv", 24, 96, S, F32),
    C("generic fp32 128x64 48->24", "dgrad", G64, "conv", 48, 24, S, F32),
    C("generic fp32 256x32, of convT 24->12", "dgrad", G32, "convT", 24, 12, (2, 4, 5, 6), F32),
    # fp32 output under bf16 storage: the families test_fp32_output_under_bf16_storage names
    C("logits 10(16)->10, 12-wide rows, fp32 out", "fwd", HALO_X, "conv", 10, 10, (2, 7, 11, 13), g_ld=12, cg=16, out_f32=True),
    C("logits 16->10, fp32 out", "fwd", HALO_X, "conv", 16, 10, (2, 7, 11, 13), out_f32=True),
    C("generic 256x16 40->12, fp32 out", "fwd", G16, "conv", 40, 12, S, out_f32=True),
    C("halo 16->10, fp32 out", "fwd", HALO, "conv", 16, 10, (2, 7, 11, 13), env=NO_X, out_f32=True),
]
# one case per family and tile name, per pass: the large-magnitude, the sliced-layout and the normal-valued runs
REPR = [c for c in FWD + DGRAD if c.name in (
    "halo_x 16->16", "halo 16->16", "up 64->10", "up, of 16->64 s2", "stem 1->32", "halo_sw 64->64", "halo_sw 8-class 128->32",
    "halo_sw 8-class, of 32->128 s2", "down_halo 16->64", "down_halo, of convT 64->16", "down_r 32->128", "down_r, of convT 128->32",
    "up8 256->64", "up8, of 64->256 s2", "generic 256x16 40->12", "generic 256x32 40->24", "generic 128x64 40->48",
    "generic 128x128 40->96", "generic 192x256 40->160", "generic 256x16 16->40", "generic 256x32 24->40", "generic 128x64 40->96",
    "generic 128x128 96->40", "generic 192x256 160->40", "ring 192x128 128->128", "ring 192x256 128->256",
    "ring 192x256, of convT 384->64")]
REPR_F32 = [c for c in F32_CASES if c.name in ("halo fp32 16->16", "generic fp32 128x64 24->48", "generic fp32 128x64 48->24",
                                               "logits 16->10, fp32 out", "generic 256x16 40->12, fp32 out")]


def _ids(cases):
    return [c.id for c in cases]


def test_every_family_and_tile_has_a_forward_and_an_input_gradient_case():
    names = {HALO_X, HALO, UP, STEM, HALO_SW, DOWN_HALO, DOWN_R, UP8, G16, G32, G64, G128, G256, RING128, RING256}
    for cases in (FWD + DGRAD, REPR):
        assert {c.family for c in cases if c.pas == "fwd"} == names
        assert {c.family for c in cases if c.pas == "dgrad"} == names - {STEM}      # (the stem's layer has no input gradient)


# ---- 1. + 3.: exact integers, pad columns, untouched columns -------------------------------------------------------------------
@pytest.mark.parametrize("max_wg", CAPS, ids=CAP_IDS)
@pytest.mark.parametrize("case", PERSISTENT, ids=_ids(PERSISTENT))
def test_exact_bf16_persistent_kernels(monkeypatch, case, max_wg):
    case.setenv(monkeypatch, max_wg)
    run, ref = _exact(case, "unit")
    run.check_columns(ref, "bf16, operands in {-1, 0, 1}")


@pytest.mark.parametrize("max_wg", CAPS[:2], ids=CAP_IDS[:2])
@pytest.mark.parametrize("case", PERMUTED, ids=_ids(PERMUTED))
def test_exact_bf16_permuted_tile_axes(monkeypatch, case, max_wg):
    case.setenv(monkeypatch, max_wg)
    run, ref = _exact(case, "unit")
    run.check_columns(ref, "bf16, operands in {-1, 0, 1}, permuted tile axes")


@pytest.mark.parametrize("case", TILED, ids=_ids(TILED))
def test_exact_bf16_tiled_kernels(monkeypatch, case):
    case.setenv(monkeypatch)
    run, ref = _exact(case, "unit")
    run.check_columns(ref, "bf16, operands in {-1, 0, 1}")


FP16 = [c.with_dt(F16) for c in FWD + DGRAD]


@pytest.mark.parametrize("case", FP16, ids=_ids(FP16))
def test_exact_fp16(monkeypatch, case):
    case.setenv(monkeypatch)
    run, ref = _exact(case, "unit")
    run.check_columns(ref, "fp16, operands in {-1, 0, 1}")


# (CTSEG_MAX_WG does not size the generic tiles' grid: those run uncapped only)
F32_RUNS = [(c, cap) for c in F32_CASES for cap in (CAPS if c.persistent else CAPS[:1])]


@pytest.mark.parametrize("case,max_wg", F32_RUNS, ids=[f"{c.id}-{CAP_IDS[CAPS.index(cap)]}" for c, cap in F32_RUNS])
def test_exact_fp32_storage_and_fp32_output(monkeypatch, case, max_wg):
    case.setenv(monkeypatch, max_wg)
    run, ref = _exact(case, "wide")
    assert run.out.t.dtype == torch.float32
    run.check_columns(ref, "fp32 values, operands in [-4, 4]")


@pytest.mark.parametrize("case", REPR, ids=_ids(REPR))
def test_bf16_store_rounds_to_nearest_even(monkeypatch, case):
    """operands in [-4, 4] ([-16, 16] on the stem, whose 27 products of such operands stay inside +-256): the fp32 result is the exact
    integer, far outside +-256, and the stored value must be its round-to-nearest-even bf16 (f2bf of ctseg_dev.h)"""
    case.setenv(monkeypatch)
    run, ref = _exact(case, "wide")
    assert float(ref.abs().max()) < 2.0 ** 24
    want = ref.to(torch.bfloat16).double()
    moved = want != ref
    ties = (ref.abs() > 256) & ((ref.abs() % 2) == 1) & (ref.abs() < 512)        # odd integers in (256, 512): exactly half way
    print(f"{case.id}: {100 * float(moved.double().mean()):.1f} % of the results are rounded, {int(ties.sum())} ties")
    assert float(ref.abs().max()) > 256 and bool(moved.any()), "the case does not leave the exact range"
    run.check_columns(want, "bf16, operands in [-4, 4], rounded to nearest even")


# ---- 3.: column slices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REPR + REPR_F32, ids=_ids(REPR + REPR_F32))
def test_column_slices_and_replay(monkeypatch, case):
    """the output as a column slice at c0 > 0 of a wider buffer and (where the family's rows allow: not the stem's 1-wide rows,
    not 12-wide rows) the gathered operand as a column slice among columns holding 3: same family, the neighbours keep the
    sentinel, the bytes equal the dense run's; the recorded program run a second time over a re-poisoned buffer writes the same
    bytes again"""
    case.setenv(monkeypatch)
    mode = "unit" if (case.dt == BF16 and not case.out_f32) else "wide"
    dense, ref = _exact(case, mode, "dense")
    Td = dense.check_columns(ref, "dense rows")
    ops = _Ops.of(case, mode)
    sl = _Run(case, ops, "sliced")
    assert sl.c0 > 0 and (sl.sliced_in or case.family == STEM or case.g_ld == 12)
    Ts = sl.check_columns(ref, "column slices")
    assert torch.equal(Ts[..., sl.c0:sl.c0 + sl.Cs], Td), "the sliced run against the dense run"
    raw = sl.out.t.view(torch.uint8).cpu().clone()
    sl.out.t.fill_(ACT_SENTINEL)
    sl.drv.replay()
    assert torch.equal(sl.out.t.view(torch.uint8).cpu(), raw), "second run of the recorded program"


# ---- 4.: normal-valued operands, per element ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REPR + REPR_F32, ids=_ids(REPR + REPR_F32))
def test_normal_operands_per_element(monkeypatch, case):
    """|out - y64| <= u * |y64| + 16 * e32 for EVERY element: u one unit in the last place of the stored type (0 for fp32 values),
    e32 the largest error of torch's float32 evaluation of the same operands, 16 the allowance for the kernels' longer sum chains
    (test_gpu_conv_extras.py)"""
    case.setenv(monkeypatch)
    ops = _Ops.of(case, ("randn", case.dt))
    y64, y32 = ops.ref(case.pas), ops.ref(case.pas, f32=True)
    odt = F32 if case.out_f32 else case.dt
    want, want32 = (y if y.ndim == 5 else y.unsqueeze(-1) for y in (y64, y32))
    bound, e32 = elem_bound(want, want32, odt)
    u = ULP[odt]
    run = _Run(case, ops)
    T = run.buffer()
    got = T[..., :run.Cn].permute(0, 4, 1, 2, 3)
    ratio = float(((got - want).abs() / bound).max())
    print(f"{case.id}: worst error / bound {ratio:.3f} (e32 {e32:.3e}, u {u:.1e}, max |y| {float(want.abs().max()):.2f})")
    assert bool(((got - want).abs() <= bound).all()), ("per-element bound", ratio)
    assert bool((T[..., run.Cn:run.Cs] == 0).all()) and bool((T[..., run.Cs:] == ACT_SENTINEL).all())
