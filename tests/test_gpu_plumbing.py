"""GPU: the kernels of csrc/optim_misc.hip, each at op level against a plain reference written from include/ctseg_hip.h.

  casts / layout / packing / gather / scale: bit-exact (compared as integers; a NaN only has to be a NaN) against numpy / torch on
    the CPU.  The cast rule of a store: fp32 -> bf16 is round-to-nearest-even (``x.to(torch.bfloat16)``), fp32 -> half SATURATES
    (``x.clamp(-65504, 65504).to(torch.float16)``, ctseg_dev.h), NaN stays NaN in both.
  one case above every block cap of ``nblocks`` (4096 blocks by default, 2048 for Adam and scale, 8192 for the 8-wide cast, 1024
    per window for the batched gather), so that the grid stride runs a second time.  Where a host reference would dominate the run
    time (the 8-wide cast, ctseg_cast, ctseg_gather_cast, ctseg_scale_inplace) the same torch expression is evaluated on the device
    and compared with torch.equal: torch's kernels are independent of ours.
  Adam, window blend: float64 reference; the tolerance is measured per case on the CPU, never fixed (below).

What the half store does with a NaN on the device (MI355X, measured through ctseg_cast F32 -> F16):
  with f2h<F16> as one v_med3_f32 clamp: 0xfbff = -65504 for the quiet NaNs 0x7fc00000, 0xffc00000 and for 0x7fffffff, 0x7bff = +65504
  for the signalling 0x7f800001.  v_med3_f32 drops a NaN operand, so a diverged fp16 network came out as finite logits, against the
  header's "NaN stays NaN".  f2h<F16> now clamps with IEEE-754 minimum / maximum (v_minimum3_f32, v_maximum3_f32), which hand a NaN on:
  every other input gets the same bits as before, a NaN is stored as a NaN (test_f16_store_keeps_nan, the NaN among the special values,
  and the fp16 cases whose inputs carry them).  A select around the old clamp does the same but spills registers in
  conv_halo_sw_kernel<F16, 128, true, true, false> (tests/test_isa_hazards.py::test_scratch_ratchet); minimum / maximum need no second
  live register and leave every kernel's scratch where it was.

Adam.  Reference: torch.optim.Adam (amsgrad=False, no weight decay) restated in float64.  A case is one (grad_scale, betas) pair with
one input vector of 1026 elements; the kernel is elementwise, n only decides which elements the 16-byte body and which the scalar
tail take, so n in {1, 2, 3, 4, 5, 1023, 1024, 1026} run on prefixes of that vector, each in buffers of its own with a sentinel at
element n.  Checkpoints: after steps 1, 2, 10, and after one call with step = 1000 on the carried state (with elements whose v is
0 and m is not: m / eps).  Error of a buffer (p, m, v): elementwise |x - x64| / |x64| where x64 != 0 (exact equality where it is 0),
its maximum and its root mean square.  Bound = 4 x the same figure of torch.optim.Adam(foreach=False) in fp32 against the float64
restatement on the whole 1026-element vector (a maximum over one to five elements can be zero by accident; the root mean square is
only asked of n >= 1023).  Gradients keep their sign over the steps and p starts small and moves away from zero, so |p| never
cancels and an error of the update shows in p.  On the CPU, in the same test, both wrong restatements -- 1 - beta2 formed in fp32,
bias correction with step - 1 -- must exceed a bound at every checkpoint of every case; they do.  (The first one at betas (0.5, 0.9)
is only 3 ulp of 0.1f off, 2.2e-07: the maximum lets it through, the root mean square of v does not, by 1.5 x .. 1.8 x; that is why
the gradients grow by 1.5 x per step.  The first is carried through all steps, the second is applied in the checkpoint's own step
from the correct state.  At step = 1000 with beta2 = 0.9 both bias corrections are exactly 1 in float64 for step and step - 1: the
second restatement is not wrong there, and that one checkpoint is exempt.)
Measured on an MI355X, worst over the cases, n and checkpoints, as a fraction of the bound:
  p 0.31, m 0.59, v 0.30 (four cases);  n = 2048 * 256 * 4 + 1203, two steps: p 0.23, m 0.25, v 0.26
  the bounds themselves (4 x torch fp32), maximum: p 5.9e-07 .. 9.7e-07, m 1.8e-07 .. 4.1e-07, v 3.5e-07 .. 6.4e-07; root mean square:
  p 1.9e-07 .. 3.2e-07, m 8.3e-08 .. 1.4e-07, v 1.3e-07 .. 2.7e-07 (m after step 1 at beta1 = 0.5 is exact in torch and in the kernel)
test_adam_matches_torch's rtol = 1e-6, atol = 1e-7 against torch fp32 is kept for p at every checkpoint.

Window blend.  Reference in float64 of the header's formula; bound = 4 x the error of a float32 numpy evaluation of the same
expression (same association, windows in the same order) against it; asserted to be below half the smallest single-window term
(logits in [1, 2], importance in [0.5, 1], inv_count in [0.25, 1]: no term below 0.125), so a dropped or doubled window fails.
Measured on an MI355X (max |out - out64|, bound in brackets):
  per window 1.0e-07 .. 1.5e-07 (5.4e-07 .. 8.3e-07);  batch 2.5e-07 .. 3.1e-07 (1.2e-06 .. 1.7e-06), the same with and without a bbox

Every entry point picks one template instantiation per storage kind (with_dtype, ctseg_dev.h); entry point x accepted kind, all
compared bit for bit here: ctseg_cast 6 pairs; ctseg_gather_cast, ctseg_nc_to_cl (general and 8-wide), ctseg_cl_to_nc,
ctseg_pack_weights (plan-built and hand-written descriptions), ctseg_window_gather, ctseg_window_gather_batch fp32 / bf16 / fp16;
ctseg_scale_inplace fp32 / bf16.  A dtype code that is no storage kind is refused; asserted for the layout, gather_cast and window
gather entry points (test_layout_and_gather_refuse_a_dtype_that_is_no_storage_kind).

Not covered, with the library's own reason:
  * ctseg_cast F16 -> BF16, BF16 -> F16, F16 -> F16: refused ("cast: bad dtypes"), asserted;
  * ctseg_scale_inplace on half storage: refused ("scale_inplace: bad arguments": the two users scale fp32 and bf16 gradients; half is
    inference-only), asserted;
  * pack descriptions with more than CTSEG_PACK_LDS_FLOATS staged floats or more than 2 parts: the header forbids them, Packer.finalize
    takes the ctseg_gather_cast path instead (tested here by removing the description);
  * ctseg_window_blend_batch with ld > 16, ld != out_ld or a bounding box outside the volume: refused, asserted.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd import _native as nat  # noqa: E402
from capstone_amd._native import BF16, F16, F32, NativeError  # noqa: E402
from capstone_amd.engine import GemmLayer  # noqa: E402
from helpers import MiniPlan, rel_err_nonzero  # noqa: E402

DEV = "cuda:0"
DTS = [F32, BF16, F16]
DT_IDS = ["fp32", "bf16", "fp16"]
SENT = 7.0                      # sentinel: exact in every storage type, never a value a test expects


# ---- the cast rule and bit comparison --------------------------------------------------------------------------------------
def _store(x, dt):
    """fp32 -> storage type dt, as the header documents a store"""
    if dt == F32:
        return x.clone()
    if dt == BF16:
        return x.to(torch.bfloat16)
    return x.clamp(-65504.0, 65504.0).to(torch.float16)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_bits(got, want, what=""):
    """same bits, NaNs excepted: where the reference is a NaN the result only has to be one (works on either device)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (_bits(got).masked_fill(gn, 0) != _bits(want).masked_fill(wn, 0))
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: got "
                             f"{got.reshape(-1)[i].item()!r} ({int(_bits(got).reshape(-1)[i]) & 0xffffffff:#x}), want "
                             f"{want.reshape(-1)[i].item()!r} ({int(_bits(want).reshape(-1)[i]) & 0xffffffff:#x})")


def _dst(n, dt, pad=8):
    return torch.full((n + pad,), SENT, dtype=nat.torch_dtype(dt), device=DEV)


def _tail_untouched(d, n):
    return bool((d[n:] == SENT).all())


def _words(*w):
    """fp32 values given by their bit patterns"""
    return torch.from_numpy(np.array(w, dtype=np.uint32).view(np.float32).copy())


def _src_f32(n, seed, device="cpu"):
    """magnitudes 1e-6 .. 1e5 (both sides of the half range), both signs"""
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, generator=g, device=device) * 10 ** (torch.rand(n, generator=g, device=device) * 11 - 6)


SPECIALS = _words(
    0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x00012345,        # +-0, fp32 denormals, least normal
    0x00008000, 0x00008001, 0x00018000,                                                          # ties among bf16 denormals
    0x3F808000, 0x3F807FFF, 0x3F808001, 0x3F818000, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000,   # bf16 ties, +-1 ulp
    0x3F801000, 0x3F800FFF, 0x3F801001, 0x3F803000, 0x3F802FFF, 0x3F803001, 0xBF801000, 0xBF803000,   # half ties, +-1 ulp
    0x33000000, 0x32FFFFFF, 0x33000001, 0x33800000, 0x33C00000, 0x387FC000, 0x38800000,        # half denormals: 2^-25 (tie to 0) ..
    0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,                                 # largest finite bf16, tie to inf
    0x477FE000, 0x477FEFFF, 0x477FF000, 0x47800000, 0x47C35000, 0xC77FE000, 0xC77FF000, 0xC7C35000,   # 65504, 65520, 65536, 1e5
    0x7F800000, 0xFF800000, 0x7FC00000)                                                          # +-inf, quiet NaN

CAST_PAIRS = [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32)]
PAIR_IDS = ["f32-bf16", "bf16-f32", "f32-f32", "bf16-bf16", "f32-f16", "f16-f32"]


def _cast_ref(x, sd, dd):
    if sd == F32:
        return _store(x, dd)
    return x.float() if dd == F32 else x.clone()


def _cast_source(sd, n, seed, device="cpu"):
    if sd == F32:
        x = _src_f32(n, seed, device)
        k = min(n, len(SPECIALS))
        x[:k] = SPECIALS[len(SPECIALS) - k:].to(device)       # n = 1 casts the NaN, 255 .. the whole list
        return x
    g = torch.Generator(device=device).manual_seed(seed)        # 16-bit sources: random bit patterns (NaNs, infs, denormals included)
    return torch.randint(-32768, 32768, (n,), generator=g, device=device, dtype=torch.int16).view(nat.torch_dtype(sd))


def _run_cast(src, sd, dd):
    n = src.numel()
    d = _dst(n, dd)
    nat.call("ctseg_cast", src.data_ptr(), sd, d.data_ptr(), dd, n)
    torch.cuda.synchronize()
    assert _tail_untouched(d, n)
    return d[:n]


# ---- 1. casts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("sd,dd", CAST_PAIRS, ids=PAIR_IDS)
def test_cast_lengths(sd, dd, n):
    x = _cast_source(sd, n, 100 + n)
    _assert_bits(_run_cast(x.to(DEV), sd, dd).cpu(), _cast_ref(x, sd, dd), f"cast n={n}")


@pytest.mark.parametrize("sd,dd", CAST_PAIRS, ids=PAIR_IDS)
def test_cast_special_values(sd, dd):
    """fp32 sources: the list above; 16-bit sources: every one of the 65536 bit patterns"""
    x = SPECIALS.clone() if sd == F32 else torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(nat.torch_dtype(sd))
    _assert_bits(_run_cast(x.to(DEV), sd, dd).cpu(), _cast_ref(x, sd, dd), "cast of special values")


def test_f16_store_keeps_nan():
    """the header's contract for both 16-bit kinds: NaN stays NaN (a diverged network must not come out as finite logits)"""
    x = _words(0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF)
    got = _run_cast(x.to(DEV), F32, F16).cpu()
    print("F32 -> F16 store of NaNs:", [hex(int(b) & 0xffff) for b in got.view(torch.int16)], got.tolist())
    assert bool(torch.isnan(got).all()), got
    assert bool(torch.isnan(_run_cast(x.to(DEV), F32, BF16).cpu()).all())


@pytest.mark.parametrize("sd,dd", CAST_PAIRS, ids=PAIR_IDS)
def test_cast_above_the_block_cap(sd, dd):
    n = 4096 * 256 + 777                    # 4096 blocks of 256 threads: the last 777 elements are a second trip of the stride
    x = _cast_source(sd, n, 7, DEV)
    _assert_bits(_run_cast(x, sd, dd), _cast_ref(x, sd, dd), "cast above the cap")


@pytest.mark.parametrize("sd,dd", [(F16, BF16), (BF16, F16), (F16, F16)])
def test_cast_refuses_unsupported_pairs(sd, dd):
    s, d = torch.zeros(8, dtype=nat.torch_dtype(sd), device=DEV), _dst(8, dd, 0)
    with pytest.raises(NativeError, match="bad dtypes"):
        nat.call("ctseg_cast", s.data_ptr(), sd, d.data_ptr(), dd, 8)
    torch.cuda.synchronize()
    assert _tail_untouched(d, 0)


# ---- 2. layout ---------------------------------------------------------------------------------------------------------------
def _nc_to_cl(x, dt, N, C, S, ld, byte_off=0):
    """x: device fp32 holding [N][C][S] from byte_off on"""
    n = N * S * ld
    d = _dst(n, dt)
    nat.call("ctseg_nc_to_cl", x.data_ptr() + byte_off, d.data_ptr(), dt, N, C, S, ld)
    torch.cuda.synchronize()
    assert _tail_untouched(d, n), "nc_to_cl wrote past the end"
    return d[:n].view(N, S, ld)


def _nc_to_cl_ref(x, dt, N, C, S, ld):
    want = torch.zeros(N, S, ld, dtype=nat.torch_dtype(dt), device=x.device)        # pad columns: +0
    want[..., :C] = _store(x.view(N, C, S).permute(0, 2, 1), dt)
    return want


def _cl_source(dt, N, C, S, ld, seed):
    """[N][S][ld] of storage type dt whose pad columns hold NaN"""
    s = torch.full((N, S, ld), float("nan"), dtype=nat.torch_dtype(dt))
    s[..., :C] = _store(_src_f32(N * S * C, seed), dt).view(N, S, C)
    return s


def _cl_to_nc(s, dt, N, C, S, ld):
    n = N * C * S
    d = _dst(n, F32)
    nat.call("ctseg_cl_to_nc", s.data_ptr(), dt, d.data_ptr(), N, C, S, ld)
    torch.cuda.synchronize()
    assert _tail_untouched(d, n), "cl_to_nc wrote past the end"
    return d[:n].view(N, C, S)


GENERAL = [(2, 3, 1001, 4), (1, 10, 777, 12), (2, 10, 513, 16), (1, 16, 300, 16)]
ABOVE_CAP = (1, 3, 350001, 4)            # S * ld and S * C both above 4096 * 256


@pytest.mark.parametrize("N,C,S,ld", GENERAL + [ABOVE_CAP])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_nc_to_cl_general_kernel(dt, N, C, S, ld):
    assert (N, C, S, ld) != ABOVE_CAP or S * ld > 4096 * 256
    x = _src_f32(N * C * S, 21)
    _assert_bits(_nc_to_cl(x.to(DEV), dt, N, C, S, ld).cpu(), _nc_to_cl_ref(x, dt, N, C, S, ld), "nc_to_cl")


@pytest.mark.parametrize("N,C,S,ld", GENERAL + [ABOVE_CAP])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_cl_to_nc_ignores_pad_columns(dt, N, C, S, ld):
    assert (N, C, S, ld) != ABOVE_CAP or S * C > 4096 * 256
    s = _cl_source(dt, N, C, S, ld, 22)
    want = s[..., :C].float().permute(0, 2, 1).contiguous()
    assert not bool(torch.isnan(want).any())
    _assert_bits(_cl_to_nc(s.to(DEV), dt, N, C, S, ld).cpu(), want, "cl_to_nc")


@pytest.mark.parametrize("case", ["eight_wide", "not_a_multiple_of_8", "source_off_by_4_bytes"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_nc_to_cl_one_channel_fast_path_and_fallbacks(dt, case):
    """C == ld == 1: N * S = 4096 from 16-byte aligned pointers takes the 8-wide kernel; 4099, or a source 4 bytes off, the general one"""
    N, S = {"eight_wide": (2, 2048), "not_a_multiple_of_8": (1, 4099), "source_off_by_4_bytes": (2, 2048)}[case]
    off = 1 if case == "source_off_by_4_bytes" else 0
    x = _src_f32(N * S + off, 23)
    x[off:off + len(SPECIALS)] = SPECIALS
    xd = x.to(DEV)
    assert xd.data_ptr() % 16 == 0
    got = _nc_to_cl(xd, dt, N, 1, S, 1, byte_off=4 * off)
    _assert_bits(got.cpu(), _nc_to_cl_ref(x[off:], dt, N, 1, S, 1), case)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_nc_to_cl_eight_wide_above_the_block_cap(dt):
    N, S = 2, (8192 * 256 * 8 + 8 * 1000) // 2           # 8192 blocks x 256 threads x 8 elements, and 1000 more threads' worth
    assert N * S > 8192 * 256 * 8 and (N * S) % 8 == 0
    x = _src_f32(N * S, 24, DEV)
    assert x.data_ptr() % 16 == 0
    _assert_bits(_nc_to_cl(x, dt, N, 1, S, 1), _nc_to_cl_ref(x, dt, N, 1, S, 1), "8-wide cast above the cap")


def test_layout_and_gather_refuse_a_dtype_that_is_no_storage_kind():
    """code 2 (CTSEG_I16) is a raw-input dtype of the resize pass only: every entry point that picks a kernel by storage kind refuses it"""
    s, d = torch.zeros(64, device=DEV), _dst(64, F32, 0)
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    calls = {"nc_to_cl": ("ctseg_nc_to_cl", s.data_ptr(), d.data_ptr(), 2, 1, 1, 8, 1),
             "cl_to_nc": ("ctseg_cl_to_nc", s.data_ptr(), 2, d.data_ptr(), 1, 1, 8, 1),
             "gather_cast": ("ctseg_gather_cast", s.data_ptr(), idx.data_ptr(), d.data_ptr(), 2, 8),
             "window_gather": ("ctseg_window_gather", s.data_ptr(), 1, 2, 2, 2, 0, 0, 0, 2, 2, 2, 0.0, d.data_ptr(), 2, 1),
             "window_gather_batch": ("ctseg_window_gather_batch", s.data_ptr(), 1, 2, 2, 2, idx.data_ptr(), 1, 2, 2, 2, 0.0, d.data_ptr(), 2, 1)}
    for name, args in calls.items():
        with pytest.raises(NativeError, match=name + ": bad arguments"):
            nat.call(*args)
    torch.cuda.synchronize()
    assert _tail_untouched(d, 0)


# ---- 3. weight packing -------------------------------------------------------------------------------------------------------
def _pack_plan(dt, first=None):
    """the layers the issue names in one plan (one packed buffer, many blocks): name -> GemmLayer"""
    torch.manual_seed(11)
    conv = lambda cin, cout, s=1: torch.nn.Conv3d(cin, cout, 3, s, 1)                                   # noqa: E731
    convT = lambda cin, cout: torch.nn.ConvTranspose3d(cin, cout, 3, 2, 1, output_padding=1)            # noqa: E731
    m = {"stem": conv(1, 32), "c32": conv(32, 32), "down": conv(32, 64, 2), "up10": convT(64, 10), "up384": convT(384, 64),
         "res": conv(16, 10), "unit0": conv(16, 10)}
    with torch.no_grad():                   # values a half store saturates, and one below the least half denormal
        m["c32"].weight.view(-1)[:5] = torch.tensor([1e5, -1e5, 65520.0, 3e-8, -0.0])
    plan = MiniPlan([p for mod in m.values() for p in (mod.weight, mod.bias)], DEV, dt, 3)
    one = lambda k: [(m[k].weight, m[k].bias, m[k].out_channels)]                                       # noqa: E731
    layers = {
        "stem": GemmLayer(plan, "stem", False, 3, 1, 1, one("stem"), 1, need_dgrad=False),
        "c32": GemmLayer(plan, "c32", False, 3, 1, 32, one("c32"), 32),
        "down": GemmLayer(plan, "down", False, 3, 2, 32, one("down"), 32),
        "up10": GemmLayer(plan, "up10", True, 3, 2, 64, one("up10"), 64),
        "up384": GemmLayer(plan, "up384", True, 3, 2, 384, one("up384"), 384),
        "res+unit0": GemmLayer(plan, "res+unit0", False, 3, 1, 16, one("res") + one("unit0"), 16),     # as the residual unit builds it
    }
    if first is not None:
        info = layers[first].fwd_pack
        plan.packer.first = (info["base"], info["base"] + info["size"])
    plan.packer.finalize()
    return plan, layers


def _pack_reference(plan):
    """what the buffers must hold: the host index applied to the flat parameters, cast by the rule of a store"""
    pk, flat = plan.packer, plan.store.flat_p.cpu()
    return _store(flat[pk.idx.cpu().long()], plan.dt), flat[pk.bias_idx.cpu().long()]


def _staged(d):
    return sum((min(g_hi, d["gs"]) - g_lo) * d["T"] for (_, _, _, g_lo, g_hi, _, _) in d["parts"])


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_pack_weights_and_gather_cast_equal_the_host_index(dt):
    plan, _ = _pack_plan(dt)
    pk = plan.packer
    assert pk.pack_blocks is not None, "the structured description must fit LDS for these layers"
    ds = pk.descs
    assert any(d["gs"] % 8 == 0 for d in ds) and any(d["gs"] % 8 != 0 for d in ds)           # vector and scalar store paths
    assert any(len(d["parts"]) == 2 for d in ds)
    assert any(_staged(d) > 2048 for d in ds) and max(_staged(d) for d in ds) <= nat.PACK_LDS_FLOATS   # staging loop runs twice
    assert any(d["ntaps"] * d["gs"] < d["kpad"] for d in ds) and any(d["ntaps"] < d["T"] for d in ds)
    want, want_bias = _pack_reference(plan)
    assert bool((want.float() != 0).any())
    pk.refresh(force=True)
    torch.cuda.synchronize()
    _assert_bits(pk.buf.cpu(), want, "ctseg_pack_weights")          # padding rows and pad K slots included: zeros
    _assert_bits(pk.bias_buf.cpu(), want_bias, "biases")
    # the fallback (a description that does not fit LDS): the index-driven gather must give the same bits
    pk.pack_blocks = None
    pk.buf.zero_()
    pk.bias_buf.zero_()
    pk.refresh(force=True)
    torch.cuda.synchronize()
    _assert_bits(pk.buf.cpu(), want, "ctseg_gather_cast")
    _assert_bits(pk.bias_buf.cpu(), want_bias, "biases (fallback)")


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_pack_split_refresh_first_then_rest(dt):
    plan, layers = _pack_plan(dt, first="c32")
    pk = plan.packer
    lo, hi = pk.first
    assert pk.can_split() and pk.n_first_rows == 32 and lo > 0          # one block of 32 real rows, not the first of the buffer
    want, want_bias = _pack_reference(plan)
    real, in_first = torch.zeros(pk.total, dtype=torch.bool), torch.zeros(pk.total, dtype=torch.bool)
    for d in pk.descs:
        span = slice(d["dst_off"], d["dst_off"] + d["rows"] * d["kpad"])
        real[span] = True
        in_first[span] = lo <= d["dst_off"] < hi
    assert bool(in_first.any()) and bool((real & ~in_first).any()) and bool((~real).any())
    sent = torch.full_like(want, 3.0)
    pk.buf.fill_(3.0)
    pk.bias_buf.fill_(3.0)
    pk.refresh(force=True, part="first")
    torch.cuda.synchronize()
    _assert_bits(pk.buf.cpu(), torch.where(in_first, want, sent), 'refresh(part="first")')
    _assert_bits(pk.bias_buf.cpu(), want_bias, 'biases after refresh(part="first")')
    assert pk.stale()
    pk.refresh(force=True, part="rest")
    torch.cuda.synchronize()
    _assert_bits(pk.buf.cpu(), torch.where(real, want, sent), 'refresh(part="rest")')      # rows it does not list are never written
    assert not pk.stale()


def _synthetic_blocks():
    """ctseg_pack_block descriptions filled by hand; parts are (o, n_lo, n_hi, g_lo, g_hi, SN, SG)"""
    return [
        # vector path, two parts whose g ranges are no multiples of 8, g 13..15 supplied by nobody, SG != T in part 1, zero fill 32..39
        dict(dst_off=0, kpad=40, gs=16, T=3, taps=[2, 0], alloc=6, rows=[0, 1, 2, 3, 4, 5],
             parts=[(5, 0, 6, 0, 5, 40, 3), (400, 0, 6, 5, 13, 70, 7)]),
        # scalar path (gs, kpad and dst_off odd); the part supplies rows 2..4 only: rows 0, 1, 5, 6 are all zero
        dict(dst_off=243, kpad=23, gs=5, T=4, taps=[3, 1, 0], alloc=7, rows=[0, 1, 2, 3, 4, 5, 6], parts=[(1000, 2, 5, 0, 5, 20, 4)]),
        # exactly CTSEG_PACK_LDS_FLOATS staged floats in two parts
        dict(dst_off=408, kpad=4616, gs=1536, T=8, taps=[7, 0, 3], alloc=3, rows=[0, 1, 2],
             parts=[(2000, 0, 3, 0, 1024, 12288, 8), (2000 + 8192, 0, 3, 1024, 1536, 12288, 8)]),
        # vector path, 2317 staged floats (neither a multiple of 256 nor of 2048); row 1 is not listed
        dict(dst_off=14256, kpad=680, gs=336, T=7, taps=[6, 3], alloc=3, rows=[0, 2], parts=[(40000, 0, 3, 0, 331, 2400, 7)]),
    ]


def _synthetic_reference(src, blocks, n_dst):
    """the header's formula, element by element in numpy; what no listed row covers keeps the sentinel"""
    out = np.full(n_dst, SENT, dtype=np.float32)
    for B in blocks:
        for n in B["rows"]:
            row = np.zeros(B["kpad"], dtype=np.float32)
            for j, t in enumerate(B["taps"]):
                for (o, n_lo, n_hi, g_lo, g_hi, SN, SG) in B["parts"]:
                    if n_lo <= n < n_hi:
                        g = np.arange(g_lo, g_hi)
                        row[j * B["gs"] + g] = src[o + (n - n_lo) * SN + (g - g_lo) * SG + t]
            out[B["dst_off"] + n * B["kpad"]:B["dst_off"] + (n + 1) * B["kpad"]] = row
    return out


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_pack_weights_synthetic_descriptions(dt):
    blocks = _synthetic_blocks()
    staged = [sum((gh - gl) * B["T"] for (_, _, _, gl, gh, _, _) in B["parts"]) for B in blocks]
    assert staged[2] == nat.PACK_LDS_FLOATS and staged[3] % 256 != 0 and staged[3] > 2048 and max(staged) <= nat.PACK_LDS_FLOATS
    n_src = 1 + max(o + (n_hi - 1 - n_lo) * SN + (g_hi - 1 - g_lo) * SG + B["T"] - 1
                    for B in blocks for (o, n_lo, n_hi, g_lo, g_hi, SN, SG) in B["parts"])         # the last element a row stages
    n_dst = max(B["dst_off"] + B["alloc"] * B["kpad"] for B in blocks)
    for a, b in zip(blocks, blocks[1:]):
        assert a["dst_off"] + a["alloc"] * a["kpad"] <= b["dst_off"]
    for B in blocks:
        assert len(B["parts"]) <= 2 and max(B["taps"]) < B["T"] and len(B["taps"]) * B["gs"] <= B["kpad"] and max(B["rows"]) < B["alloc"]
        if B["gs"] % 8 == 0 and B["kpad"] % 8 == 0:
            assert B["dst_off"] % 8 == 0
    src = _src_f32(n_src, 31)
    arr = (nat.PackBlock * len(blocks))()
    for b, B in enumerate(blocks):
        A = arr[b]
        A.dst_off, A.kpad, A.gs, A.ntaps, A.T, A.nparts = B["dst_off"], B["kpad"], B["gs"], len(B["taps"]), B["T"], len(B["parts"])
        for j, t in enumerate(B["taps"]):
            A.tap[j] = t
        for k, part in enumerate(B["parts"]):
            P = A.part[k]
            P.o, P.n_lo, P.n_hi, P.g_lo, P.g_hi, P.SN, P.SG = part
    pairs = [(b, n) for b, B in enumerate(blocks) for n in B["rows"]]
    pairs = [pairs[i] for i in np.random.RandomState(5).permutation(len(pairs))]                 # rows of the blocks interleaved
    d_blocks = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(DEV)
    d_rows = torch.tensor(pairs, dtype=torch.int32).reshape(-1).to(DEV)
    d, d_src = _dst(n_dst, dt), src.to(DEV)
    nat.call("ctseg_pack_weights", d_src.data_ptr(), d_blocks.data_ptr(), len(blocks), d_rows.data_ptr(), len(pairs),
             d.data_ptr(), dt)
    torch.cuda.synchronize()
    assert _tail_untouched(d, n_dst)
    want = torch.from_numpy(_synthetic_reference(src.numpy(), blocks, n_dst))
    assert bool((want[:240] != 0).any()) and bool((want[243:404].view(7, 23)[[0, 1, 5, 6]] == 0).all())
    _assert_bits(d[:n_dst].cpu(), _store(want, dt), "synthetic pack descriptions")


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 515])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_gather_cast(dt, n):
    """a random index with repeats and the zero element; the length above the cap is compared on the device"""
    dev = DEV if n > 4096 * 256 else "cpu"
    src = _src_f32(1000, 41, dev)
    src[:len(SPECIALS)] = SPECIALS.to(dev)
    src[999] = 0.0
    g = torch.Generator(device=dev).manual_seed(42 + n)
    idx = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int32)
    idx[n // 2] = 999
    d, dsrc, didx = _dst(n, dt), src.to(DEV), idx.to(DEV)
    nat.call("ctseg_gather_cast", dsrc.data_ptr(), didx.data_ptr(), d.data_ptr(), dt, n)
    torch.cuda.synchronize()
    assert _tail_untouched(d, n)
    _assert_bits(d[:n].to(dev), _store(src[idx.long()], dt), "gather_cast")


# ---- 4. Adam and scale -------------------------------------------------------------------------------------------------------
LR, EPS = 1e-3, 1e-8
ADAM_CASES = [(1.0, (0.9, 0.999)), (0.5, (0.9, 0.999)), (1.0, (0.5, 0.9)), (0.5, (0.5, 0.9))]
ADAM_NS = [1, 2, 3, 4, 5, 1023, 1024, 1026]
ADAM_L = 1026
ZERO_G = [3, 700, 1024]                 # gradient exactly zero at every step: m = v = 0, p stays
M_OVER_EPS = [2, 601, 1025]             # at the step-1000 call: v = 0, m != 0, g = 0  ->  the update is m / eps


def _adam_inputs(L, seed):
    r = np.random.RandomState(seed)
    g0 = (10 ** r.uniform(-6, 3, L) * r.choice([-1.0, 1.0], L)).astype(np.float32)
    g0[[i for i in ZERO_G if i < L]] = 0.0
    p0 = (-np.where(g0 == 0, -1.0, np.sign(g0)) * r.uniform(1e-4, 1e-3, L)).astype(np.float32)   # small, moving away from zero
    return p0, g0


def _grad(g0, k):
    """gradient of step k: the same sign at every step (m never changes sign), growing by 1.5 x per step so that the newest term
    leads m and v (with a constant gradient the roundings of ten steps pile up in torch's v and its bound lets 1.f - 0.9f through)"""
    return (g0 * np.float32(1.5 ** (k - 1))).astype(np.float32)


def _adam64_step(p, m, v, g, b1, b2, step, gscale, omb2=None, bc_step=None):
    """one step of torch.optim.Adam (amsgrad=False, weight_decay=0) in float64; omb2 / bc_step: the two wrong restatements"""
    g = g.astype(np.float64) * gscale
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2 if omb2 is None else omb2) * g * g
    s = step if bc_step is None else bc_step
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = np.float64(1.0 - b1 ** s), np.float64(1.0 - b2 ** s)
        p = p - (LR / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + EPS))
    return p, m, v


def _carry(L):
    idx = [i for i in M_OVER_EPS if i < L]
    return idx, np.float32(1e-3)


def _adam_restated(p0, g0, gscale, betas, steps, carried, mutant=None):
    """checkpoint -> (p, m, v) in float64.  mutant "omb2": 1 - beta2 formed in fp32, at every step (a constant formed wrongly is wrong
    throughout).  mutant "step": bias correction with step - 1 in the checkpoint's own step only, from the correct state before it
    (carried through, the division by zero of step 1 would make every later checkpoint fail for that reason alone)"""
    b1, b2 = betas
    omb2 = float(np.float32(1.0) - np.float32(b2)) if mutant == "omb2" else None
    p, m, v = p0.astype(np.float64), np.zeros(len(p0)), np.zeros(len(p0))
    out = {}
    for k in range(1, max(steps) + 1):
        if k in steps and mutant == "step":
            out[k] = _adam64_step(p, m, v, _grad(g0, k), b1, b2, k, gscale, None, k - 1)
        p, m, v = _adam64_step(p, m, v, _grad(g0, k), b1, b2, k, gscale, omb2)
        if k in steps and mutant != "step":
            out[k] = (p.copy(), m.copy(), v.copy())
    if carried:
        idx, mval = _carry(len(p0))
        m[idx], v[idx] = np.sign(g0[idx]) * float(mval), 0.0
        g = _grad(g0, 11)
        g[idx] = 0.0
        out[1000] = _adam64_step(p, m, v, g, b1, b2, 1000, gscale, omb2, 999 if mutant == "step" else None)
    return out


def _adam_torch(p0, g0, gscale, betas, steps, carried):
    """the same trajectory through torch.optim.Adam in fp32 on the CPU"""
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=LR, betas=betas, eps=EPS, foreach=False)
    snap = lambda: tuple(t.detach().numpy().copy() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))   # noqa: E731
    out = {}
    for k in range(1, max(steps) + 1):
        p.grad = torch.from_numpy(_grad(g0, k)) * gscale             # 1 and 0.5: exact, as the kernel's g * grad_scale
        opt.step()
        if k in steps:
            out[k] = snap()
    if carried:
        idx, mval = _carry(len(p0))
        st = opt.state[p]
        with torch.no_grad():
            st["exp_avg"][idx] = torch.from_numpy(np.sign(g0[idx]) * mval)
            st["exp_avg_sq"][idx] = 0.0
        if torch.is_tensor(st["step"]):
            st["step"].fill_(999.0)
        else:
            st["step"] = 999
        g = _grad(g0, 11)
        g[idx] = 0.0
        p.grad = torch.from_numpy(g) * gscale
        opt.step()
        out[1000] = snap()
    return out


def _adam_bounds(p0, g0, gscale, betas, steps=(1, 2, 10), carried=True):
    """-> (float64 reference, torch fp32 trajectory, bounds[checkpoint][buffer] = (max, rms)); asserts on the CPU that both wrong
    restatements exceed a bound at every checkpoint"""
    b2 = betas[1]
    ref = _adam_restated(p0, g0, gscale, betas, steps, carried)
    tor = _adam_torch(p0, g0, gscale, betas, steps, carried)
    bounds = {}
    for ck in ref:
        bounds[ck] = []
        for x, x64 in zip(tor[ck], ref[ck]):
            mx, rms, zeros = rel_err_nonzero(x, x64)
            assert zeros and mx < 1e-5, (ck, mx)               # torch in fp32 is itself close (m of step 1 at beta1 = 0.5 is exact)
            bounds[ck].append((4 * mx, 4 * rms))
    for mutant in ("omb2", "step"):
        mut = _adam_restated(p0, g0, gscale, betas, steps, carried, mutant)
        for ck in ref:
            errs = [rel_err_nonzero(x, x64)[:2] for x, x64 in zip(mut[ck], ref[ck])]
            if ck == 1000 and all(e == 0 for es in errs for e in es):
                assert b2 ** 999 < 1e-17 and mutant == "step"      # 1 - beta2^999 == 1 - beta2^1000 == 1 in float64: not wrong here
                continue
            caught = any(not (e <= b) for es, bs in zip(errs, bounds[ck]) for e, b in zip(es, bs))
            assert caught, f"the bound lets the wrong restatement '{mutant}' through at checkpoint {ck}: {errs} vs {bounds[ck]}"
    return ref, tor, bounds


def _adam_device_run(p0, g0, n, gscale, betas, steps, carried):
    """the kernel on raw buffers holding the first n elements and a sentinel behind them -> checkpoint -> (p, m, v) as numpy"""
    def buf(a):
        t = torch.full((n + 4,), SENT, dtype=torch.float32, device=DEV)
        t[:n] = torch.from_numpy(np.ascontiguousarray(a[:n])).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    p, m, v = buf(p0), buf(np.zeros_like(p0)), buf(np.zeros_like(p0))
    grads = {k: buf(_grad(g0, k)) for k in range(1, max(steps) + 1)}
    snap = lambda: tuple(t[:n].cpu().numpy() for t in (p, m, v))                                  # noqa: E731
    out = {}

    def step(g, k):
        nat.call("ctseg_adam_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, betas[0], betas[1], EPS, k, gscale)
    for k in range(1, max(steps) + 1):
        step(grads[k], k)
        if k in steps:
            out[k] = snap()
    if carried:
        idx, mval = _carry(n)
        gl = _grad(g0, 11)[:n].copy()
        gl[idx] = 0.0
        if idx:
            m[idx] = torch.from_numpy(np.sign(g0[idx]) * mval).to(DEV)
            v[idx] = 0.0
        g = buf(gl)
        grads[1000] = g
        step(g, 1000)
        out[1000] = snap()
    torch.cuda.synchronize()
    for t in [p, m, v, *grads.values()]:
        assert _tail_untouched(t, n), "adam_step touched element n"
    for k, g in grads.items():
        assert torch.equal(g[:n].cpu(), torch.from_numpy(gl if k == 1000 else _grad(g0, k)[:n])), "adam_step wrote the gradient"
    return out


def _adam_check(got, ref, tor, bounds, n, worst):
    for ck in got:
        for name, x, x64, (bmax, brms) in zip("pmv", got[ck], ref[ck], bounds[ck]):
            mx, rms, zeros = rel_err_nonzero(x, x64[:n])
            worst[name] = max(worst[name], mx / bmax if mx else 0.0, rms / brms if n >= 1023 and rms else 0.0)
            assert zeros, (name, ck, n)
            assert mx <= bmax, f"{name} after step {ck}, n={n}: max relative error {mx:.3e} > 4 x torch fp32's ({bmax:.3e})"
            if n >= 1023:
                assert rms <= brms, f"{name} after step {ck}, n={n}: rms relative error {rms:.3e} > 4 x torch fp32's ({brms:.3e})"
        np.testing.assert_allclose(got[ck][0], tor[ck][0][:n], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("gscale,betas", ADAM_CASES)
def test_adam_step_vs_float64_restatement(gscale, betas):
    p0, g0 = _adam_inputs(ADAM_L, 51)
    ref, tor, bounds = _adam_bounds(p0, g0, gscale, betas)
    # v = 0, m != 0 really is m / eps: the update of those elements is lr * (beta1 * the carried 1e-3) / eps = 100 * beta1
    i = M_OVER_EPS[0]
    assert abs(abs(ref[1000][0][i] - ref[10][0][i]) - LR * betas[0] * 1e-3 / EPS) < 1e-3 and ref[1000][2][i] == 0
    worst = dict(p=0.0, m=0.0, v=0.0)
    for n in ADAM_NS:
        _adam_check(_adam_device_run(p0, g0, n, gscale, betas, (1, 2, 10), True), ref, tor, bounds, n, worst)
    print(f"adam grad_scale={gscale} betas={betas}: torch fp32 vs float64 (max, rms) x 4 per checkpoint "
          + "; ".join(f"{ck}: " + " ".join(f"{n_}=({a:.1e},{b:.1e})" for n_, (a, b) in zip("pmv", bounds[ck])) for ck in bounds)
          + " | kernel worst error / bound: " + " ".join(f"{k}={v_:.2f}" for k, v_ in worst.items()))


def test_adam_step_above_the_block_cap():
    n = 2048 * 256 * 4 + 4 * 300 + 3        # 2048 blocks x 256 threads x 4 elements, 300 more vectors (a second trip), a 3-element tail
    assert n > 2048 * 256 * 4 and n % 4 == 3
    p0, g0 = _adam_inputs(n, 52)
    ref, tor, bounds = _adam_bounds(p0, g0, 0.5, (0.9, 0.999), steps=(1, 2), carried=False)
    worst = dict(p=0.0, m=0.0, v=0.0)
    _adam_check(_adam_device_run(p0, g0, n, 0.5, (0.9, 0.999), (1, 2), False), ref, tor, bounds, n, worst)
    print("adam above the cap: kernel worst error / bound: " + " ".join(f"{k}={v_:.2f}" for k, v_ in worst.items()))


SCALE_FACTORS = [("host", 0.37, None), ("device", 1.0, 1.7), ("both", 0.3, 1.0 / 3.0)]


def _scale_ref(x, f):
    f = float(f)                        # an fp32 value: exact as a Python float
    return x * f if x.dtype == torch.float32 else (x.float() * f).to(torch.bfloat16)


def _run_scale(x, dt, n, host, dev):
    ds = None if dev is None else torch.tensor([dev], dtype=torch.float32, device=DEV)
    nat.call("ctseg_scale_inplace", x.data_ptr(), dt, n, nat.ptr(ds), host)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which,host,dev", SCALE_FACTORS, ids=[f[0] for f in SCALE_FACTORS])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_scale_inplace(dt, which, host, dev):
    f = np.float32(host) * (np.float32(1.0) if dev is None else np.float32(dev))     # formed in fp32, as the kernel forms it
    assert f != 1
    for n in [1, 7, 8, 9, 4099, 2048 * 256 * (4 if dt == F32 else 8) + (403 if dt == F32 else 805)]:
        big = n > 4099
        x = _store(_src_f32(n, 60 + n % 50, DEV if big else "cpu"), dt)
        d = _dst(n, dt)
        d[:n] = x.to(DEV)
        assert d.data_ptr() % 16 == 0
        _run_scale(d, dt, n, host, dev)
        assert _tail_untouched(d, n), n
        _assert_bits(d[:n] if big else d[:n].cpu(), _scale_ref(x, f), f"scale_inplace n={n}")     # the big one: on the device


@pytest.mark.parametrize("host,dev", [(1.0, None), (0.5, 2.0)])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_scale_inplace_by_exactly_one_touches_nothing(dt, host, dev):
    """NaN payloads (signalling ones included) would not survive a multiplication by 1; the launch must leave them alone"""
    if dt == F32:
        pat = torch.from_numpy(np.array([0x7F800001, 0x7FC12345, 0xFFFFFFFF, 0x7FA00000, 0xFF812345, 0x3F800000] * 700,
                                        dtype=np.uint32).view(np.int32).copy())
    else:
        pat = torch.from_numpy(np.array([0x7F81, 0x7FC1, 0xFFFF, 0x7FA0, 0xFF85, 0x3F80] * 700, dtype=np.uint16).view(np.int16).copy())
    d = pat.to(DEV)
    _run_scale(d, dt, d.numel(), host, dev)
    assert torch.equal(d.cpu(), pat)


def test_scale_inplace_refuses_half_storage():
    d = _dst(16, F16, 0)
    with pytest.raises(NativeError, match="scale_inplace: bad arguments"):
        nat.call("ctseg_scale_inplace", d.data_ptr(), F16, 16, None, 0.5)
    torch.cuda.synchronize()
    assert _tail_untouched(d, 0)


# ---- 5. sliding-window kernels -----------------------------------------------------------------------------------------------
def _gather_ref(vol, start, roi, cval, ld):
    """the header's definition in numpy: [rx][ry][rz][ld] fp32; outside the volume = cval, pad channels = 0"""
    Cin, X, Y, Z = vol.shape
    gx, gy, gz = (start[a] + np.arange(roi[a]) for a in range(3))
    inside = (((gx >= 0) & (gx < X))[:, None, None] & ((gy >= 0) & (gy < Y))[None, :, None] & ((gz >= 0) & (gz < Z))[None, None, :])
    sub = vol[:, np.clip(gx, 0, X - 1)[:, None, None], np.clip(gy, 0, Y - 1)[None, :, None], np.clip(gz, 0, Z - 1)[None, None, :]]
    out = np.zeros(tuple(roi) + (ld,), dtype=np.float32)
    out[..., :Cin] = np.where(inside[None], sub, np.float32(cval)).transpose(1, 2, 3, 0)
    return out


def _gather_check(vol, starts, roi, cval, ld, dt):
    """every window alone, the batch of all of them, and the numpy reference: all the same bits"""
    Cin, X, Y, Z = vol.shape
    dv = torch.from_numpy(vol).to(DEV)
    n = roi[0] * roi[1] * roi[2] * ld
    want = [_store(torch.from_numpy(_gather_ref(vol, s, roi, cval, ld)), dt).reshape(-1) for s in starts]
    for s, w in zip(starts, want):
        d = _dst(n, dt)
        nat.call("ctseg_window_gather", dv.data_ptr(), Cin, X, Y, Z, *s, *roi, cval, d.data_ptr(), dt, ld)
        torch.cuda.synchronize()
        assert _tail_untouched(d, n)
        _assert_bits(d[:n].cpu(), w, f"window_gather at {s}")
    st = torch.tensor(starts, dtype=torch.int32).to(DEV)
    d = _dst(len(starts) * n, dt)
    nat.call("ctseg_window_gather_batch", dv.data_ptr(), Cin, X, Y, Z, st.data_ptr(), len(starts), *roi, cval, d.data_ptr(), dt, ld)
    torch.cuda.synchronize()
    assert _tail_untouched(d, len(starts) * n)
    _assert_bits(d[:len(starts) * n].cpu(), torch.cat(want), "window_gather_batch")


def _volume(shape, seed):
    return np.random.RandomState(seed).uniform(-2000, 2000, shape).astype(np.float32)


@pytest.mark.parametrize("ld", [2, 4])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_window_gather_against_the_header(dt, ld):
    vol = _volume((2, 9, 7, 5), 71)
    # inside; straddling the low and high face of x, y, z; negative origins (one window wholly outside)
    starts = [(3, 2, 1), (-2, 1, 0), (7, 1, 0), (2, -1, 0), (2, 5, 0), (2, 1, -3), (2, 1, 3), (-1, -2, -3), (-5, -5, -5)]
    _gather_check(vol, starts[:5], (4, 4, 4), -3.5, ld, dt)
    _gather_check(vol, starts[5:], (4, 4, 4), -3.5, ld, dt)
    _gather_check(vol, [(-1, 0, -1), (-3, -1, 0), (0, 0, 0), (-2, -1, -1), (0, -1, 0)], (12, 8, 6), -3.5, ld, dt)   # larger than the volume


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_window_gather_batch_above_the_block_cap(dt):
    roi, ld = (44, 40, 38), 4
    assert roi[0] * roi[1] * roi[2] * ld > 1024 * 256
    vol = _volume((3, 50, 45, 40), 72)
    dv = torch.from_numpy(vol).to(DEV)
    starts = [(-3, 2, 1), (10, -4, 5)]
    n = roi[0] * roi[1] * roi[2] * ld
    d = _dst(2 * n, dt)
    st = torch.tensor(starts, dtype=torch.int32).to(DEV)
    nat.call("ctseg_window_gather_batch", dv.data_ptr(), 3, 50, 45, 40, st.data_ptr(), 2, *roi, -3.5, d.data_ptr(), dt, ld)
    torch.cuda.synchronize()
    assert _tail_untouched(d, 2 * n)
    want = torch.cat([_store(torch.from_numpy(_gather_ref(vol, s, roi, -3.5, ld)), dt).reshape(-1) for s in starts])
    _assert_bits(d[:2 * n].cpu(), want, "window_gather_batch above the cap")


def _blend_ref(logits, starts, imp, inv, out0, C, dtype):
    """out[x0+x][y0+y][z0+z][c] += importance[x][y][z] * inv_count[voxel] * logits[w][x][y][z][c], windows in order, in `dtype`.
    -> (out, the smallest single-window term)"""
    X, Y, Z = out0.shape[:3]
    rx, ry, rz = imp.shape
    out = out0.astype(dtype)
    imp, smallest = imp.astype(dtype), np.inf
    for w, (x0, y0, z0) in enumerate(starts):
        xs, ys, zs = (np.arange(max(0, -o), min(r, e - o)) for o, r, e in ((x0, rx, X), (y0, ry, Y), (z0, rz, Z)))
        if min(len(xs), len(ys), len(zs)) == 0:
            continue
        ix = np.ix_(xs, ys, zs)
        ox = np.ix_(xs + x0, ys + y0, zs + z0)
        wgt = imp[ix] * (inv[ox].astype(dtype) if inv is not None else dtype(1))
        term = wgt[..., None] * logits[w][ix][..., :C].astype(dtype)
        out[ox + (slice(0, C),)] = out[ox][..., :C] + term
        smallest = min(smallest, float(term.min()))
    return out, smallest


def _blend_case(X, Y, Z, roi, starts, ld, out_ld, C, with_inv, seed):
    r = np.random.RandomState(seed)
    logits = r.uniform(1, 2, (len(starts),) + roi + (ld,)).astype(np.float32)
    imp = r.uniform(0.5, 1, roi).astype(np.float32)
    inv = r.uniform(0.25, 1, (X, Y, Z)).astype(np.float32) if with_inv else None
    out0 = np.full((X, Y, Z, out_ld), SENT, dtype=np.float32)            # columns C.. must keep the sentinel
    out0[..., :C] = 0
    ref, smallest = _blend_ref(logits, starts, imp, inv, out0, C, np.float64)
    f32, _ = _blend_ref(logits, starts, imp, inv, out0, C, np.float32)
    bound = 4 * float(np.abs(f32.astype(np.float64) - ref).max())
    assert 0 < bound < 0.5 * smallest and smallest >= 0.125, (bound, smallest)
    assert bool((ref[..., :C] == 0).any()) or len(starts) > 3           # (the per-window cases leave part of the volume uncovered)
    return logits, imp, inv, out0, ref, bound


BLEND_STARTS = [(-2, -1, -1), (2, 3, 1), (6, 6, 4)]      # roi (6, 5, 4) in a 10 x 9 x 6 volume: overlapping, overhanging both sides


@pytest.mark.parametrize("ld,out_ld,C,with_inv", [(12, 16, 10, True), (3, 3, 3, True), (12, 16, 10, False), (4, 4, 2, True)])
def test_window_blend_against_float64(ld, out_ld, C, with_inv):
    X, Y, Z, roi = 10, 9, 6, (6, 5, 4)
    logits, imp, inv, out0, ref, bound = _blend_case(X, Y, Z, roi, BLEND_STARTS, ld, out_ld, C, with_inv, 81)
    dl, di, out = torch.from_numpy(logits).to(DEV), torch.from_numpy(imp).to(DEV), torch.from_numpy(out0).to(DEV)
    dinv = torch.from_numpy(inv).to(DEV) if with_inv else None
    for w, s in enumerate(BLEND_STARTS):
        nat.call("ctseg_window_blend", dl[w].data_ptr(), ld, C, *roi, *s, di.data_ptr(), nat.ptr(dinv), out.data_ptr(), X, Y, Z, out_ld)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    err = float(np.abs(got[..., :C].astype(np.float64) - ref[..., :C]).max())
    print(f"window_blend ld={ld} out_ld={out_ld} C={C} inv_count={with_inv}: max error {err:.2e}, bound {bound:.2e}")
    assert np.array_equal(got[..., C:], out0[..., C:]), "columns C..out_ld-1 of out were written"
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("with_bbox", [False, True], ids=["whole_volume", "bbox"])
@pytest.mark.parametrize("ld,C", [(4, 2), (12, 10), (16, 13)])
def test_window_blend_batch_against_float64(ld, C, with_bbox):
    X, Y, Z, roi = 12, 11, 9, (6, 5, 4)
    starts = [(1, 2, 1), (4, 4, 3), (-2, 5, 2), (6, 6, 5), (3, 3, 2)]         # clipped union: x 0..11, y 2..10, z 1..8
    bbox = (0, 2, 1, 12, 9, 8)
    logits, imp, inv, out0, ref, bound = _blend_case(X, Y, Z, roi, starts, ld, ld, C, True, 82)
    dl, di, dinv = (torch.from_numpy(a).to(DEV) for a in (logits, imp, inv))
    out = torch.from_numpy(out0).to(DEV)
    st = torch.tensor(starts, dtype=torch.int32).to(DEV)
    nat.call("ctseg_window_blend_batch", dl.data_ptr(), ld, C, *roi, st.data_ptr(), len(starts), di.data_ptr(), dinv.data_ptr(),
             out.data_ptr(), X, Y, Z, ld, (ctypes.c_int32 * 6)(*bbox) if with_bbox else None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    err = float(np.abs(got[..., :C].astype(np.float64) - ref[..., :C]).max())
    print(f"window_blend_batch ld={ld} C={C} bbox={with_bbox}: max error {err:.2e}, bound {bound:.2e}")
    assert np.array_equal(got[..., C:], out0[..., C:]), "pad columns of out changed"
    assert bool((ref[..., :C] == 0).any()) and np.array_equal(got[..., :C] == 0, ref[..., :C] == 0)    # voxels no window covers
    assert err <= bound, (err, bound)


def test_window_blend_batch_refusals():
    X, Y, Z, roi = 8, 8, 8, (4, 4, 4)
    z = torch.zeros(2 * 64 * 20 + X * Y * Z * 20, device=DEV)
    st = torch.zeros(6, dtype=torch.int32, device=DEV)

    def call(ld, out_ld, bbox):
        nat.call("ctseg_window_blend_batch", z.data_ptr(), ld, 3, *roi, st.data_ptr(), 2, z.data_ptr(), None, z.data_ptr(), X, Y, Z,
                 out_ld, None if bbox is None else (ctypes.c_int32 * 6)(*bbox))
    with pytest.raises(NativeError, match="16-byte vectors"):
        call(20, 20, None)
    with pytest.raises(NativeError, match="16-byte vectors"):
        call(12, 16, None)
    for bbox in [(0, 0, 0, X + 1, Y, Z), (-1, 0, 0, 4, 4, 4), (5, 0, 0, 4, 4, 4), (0, 0, 0, 0, 4, 4)]:
        with pytest.raises(NativeError, match="bounding box outside the volume"):
            call(12, 12, bbox)
    torch.cuda.synchronize()
    assert bool((z == 0).all())
