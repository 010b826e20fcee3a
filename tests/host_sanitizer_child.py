"""Run INSIDE a process that preloaded the AddressSanitizer runtime and points CTSEG_LIB at the host-sanitizer build
(tests/test_host_sanitizer.py starts it): drives every host-only path of the C ABI — descriptor validation, kernel selection,
sizing / capability queries — over a few thousand random descriptors, plus the argument checks of the launch entry points that
reject before any HIP call.  No GPU, no launches.  Prints "SANITIZER-CHILD-OK <n>" when it got through."""
import ctypes
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ct-image-segmentation_amd"))
from capstone_amd import _native as nat  # noqa: E402

L = nat.lib()
assert "lib_asan" in nat.LIB_PATH, nat.LIB_PATH
rnd = random.Random(12342)
buf = ctypes.create_string_buffer(1 << 16)          # a real (host) address for the "pointer" fields: never dereferenced by the host code
base = ctypes.addressof(buf)


def tap(dx, dy, dz):
    return (dx & 255) | ((dy & 255) << 8) | ((dz & 255) << 16)


def rand_conv():
    d = nat.ConvDesc()
    d.dtype = rnd.choice([nat.F32, nat.BF16, nat.F16, 7])
    d.N = rnd.choice([1, 2, 3, 17])
    sp = [rnd.choice([1, 3, 4, 8, 16, 24, 48, 64, 256, 512]) for _ in range(3)]
    d.sin, d.sout = rnd.choice([(1, 1), (2, 1), (1, 2), (3, 1)])
    d.Xr, d.Yr, d.Zr = sp
    d.Xi, d.Yi, d.Zi = [s * d.sin for s in sp]
    d.Xo, d.Yo, d.Zo = [s * d.sout for s in sp]
    d.Cg = rnd.choice([1, 8, 16, 32, 64, 128, 256, 384])
    d.Cn = rnd.choice([10, 12, 16, 32, 64, 128, 256, 384])
    d.Cn_store = rnd.choice([d.Cn, (d.Cn + 7) // 8 * 8, (d.Cn + 3) // 4 * 4])
    d.g_ld = rnd.choice([d.Cg, 12, d.Cg + 8])
    d.o_ld = rnd.choice([d.Cn_store, 12, d.Cn_store + 8])
    d.add_ld = d.o_ld
    d.in_, d.w, d.out = base, base + 4096, base + 8192
    if rnd.random() < 0.4:
        d.add = rnd.choice([base, base + 12288])
    if rnd.random() < 0.3:
        d.out2, d.out2_col0, d.o2_ld = base + 16384, rnd.choice([0, 4, 16, 32, 64]), rnd.choice([16, 32, 64])
    d.out_f32, d.add_f32 = rnd.choice([0, 0, 1]), rnd.choice([0, 0, 1])
    d.nclass = rnd.choice([1, 1, 8, 9])
    for c in range(min(d.nclass, nat.MAX_CLASSES)):
        k = d.cls[c]
        k.ntaps = rnd.choice([1, 2, 4, 8, 27, 28])
        k.kpad = (max(1, min(k.ntaps, 27)) * d.Cg + 127) // 128 * 128 + rnd.choice([0, 0, 64])
        k.w_off = rnd.choice([0, 8, 1024, 3])
        k.ox, k.oy, k.oz = [rnd.choice([0, 1]) for _ in range(3)]
        order = rnd.choice([1, -1])
        for j in range(min(k.ntaps, 27)):
            k.taps[j] = tap(order * (j // 9 - 1), order * ((j // 3) % 3 - 1), order * (j % 3 - 1)) if k.ntaps == 27 else tap(0, 0, rnd.choice([-1, 0, 1, 2]))
    if rnd.random() < 0.3:
        d.in_mean_rstd, d.in_alpha, d.in_norm_C = base, base, rnd.choice([10, 12, 32])
    if rnd.random() < 0.4:
        d.bst_y, d.bst_y_ld, d.bst_C, d.bst_col0 = base + 20480, rnd.choice([12, 16, 32, 64, 256]), rnd.choice([10, 32, 64, 256]), rnd.choice([0, 0, 32, 128, 5])
    return d


def rand_wgrad():
    d = nat.WgradDesc()
    d.dtype = rnd.choice([nat.F32, nat.BF16, nat.F16])
    d.N = rnd.choice([1, 2])
    sp = [rnd.choice([3, 4, 8, 16, 24, 64, 256]) for _ in range(3)]
    d.sin = rnd.choice([1, 2])
    d.Xr, d.Yr, d.Zr = sp
    d.Xi, d.Yi, d.Zi = [s * d.sin for s in sp]
    d.Cg, d.Cn = rnd.choice([1, 16, 32, 64, 256]), rnd.choice([10, 16, 64, 256, 384])
    d.g_ld, d.d_ld = rnd.choice([d.Cg, 12]), rnd.choice([(d.Cn + 7) // 8 * 8, 12])
    d.ntaps = rnd.choice([1, 27])
    for j in range(d.ntaps):
        d.taps[j] = tap(j // 9 - 1, (j // 3) % 3 - 1, j % 3 - 1)
    d.splits = rnd.choice([1, 8, 72, 128])
    d.kpad_w = (d.ntaps * d.Cg + 1 + 127) // 128 * 128
    d.cn_pad = (d.Cn + 127) // 128 * 128
    d.in_, d.dy, d.ws = base, base + 4096, base + 8192
    if rnd.random() < 0.3:
        d.in_mean_rstd, d.in_alpha, d.in_norm_C = base, base, rnd.choice([10, 12, 32])
    if rnd.random() < 0.4:
        d.dyn_col0 = rnd.choice([0, 16, 32, d.Cn // 2])
        if rnd.random() < 0.7:
            d.dyn_g, d.dyn_y, d.dyn_mean_rstd, d.dyn_alpha, d.dyn_sums = base + 12288, base + 16384, base, base, base
        d.dyn_g_ld, d.dyn_y_ld = rnd.choice([12, 16, 32]), rnd.choice([12, 16, 32])
    return d


n = 0
for _ in range(4000):
    d = rand_conv()
    r = ctypes.byref(d)
    for q in ("ctseg_conv_num_tiles", "ctseg_conv_split_ok", "ctseg_conv_narrow_ok", "ctseg_conv_in_norm_ok", "ctseg_conv_bwd_stats_slots"):
        getattr(L, q)(r)
        n += 1
    L.ctseg_conv_logits_ce_slots(r, rnd.choice([2, 10, 12, 13]))
    # launch entry points with arguments that are rejected BEFORE any HIP call: a foreign struct size, null tensors
    d.struct_size -= 8
    assert L.ctseg_conv_igemm(r, None) < 0
    d.struct_size += 8
    d.out = None
    assert L.ctseg_conv_igemm(r, None) < 0 and L.ctseg_last_error()
    n += 3
for _ in range(2000):
    w = rand_wgrad()
    r = ctypes.byref(w)
    L.ctseg_conv_wgrad_slabs(r)
    per_cu, stage_bytes = ctypes.c_int32(), ctypes.c_int32()
    L.ctseg_conv_wgrad_wgs_per_slab(r, ctypes.byref(per_cu), ctypes.byref(stage_bytes))
    L.ctseg_conv_wgrad_wgs_per_slab(r, None, None)
    L.ctseg_wgrad_dy_norm_ok(r)
    L.ctseg_wgrad_narrow_ok(r)
    L.ctseg_wgrad_in_norm_ok(r)
    w.ws = None
    assert L.ctseg_conv_wgrad(r, None) < 0
    n += 7
for c in (1, 10, 16, 33, 64, 200, 256, 1024):
    L.ctseg_conv_tile_rows(c), L.ctseg_conv_tile_cols(c), L.ctseg_wgrad_tile_cols(c)
assert L.ctseg_adam_step(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None) < 0


def rejects(fn, fragment, *args):
    assert getattr(L, fn)(*args) < 0, fn
    err = L.ctseg_last_error().decode()
    assert fragment in err, (fn, fragment, err)


# norm / column-sum entry points: one shared channel-chunk check (dtype, chunk width, strides), grid sizing and argument checks
p = base
F16_BWD = "bad dtype %d (CTSEG_F16 is accepted by the forward pass only)" % nat.F16
STRIDE = "channel stride 10 not chunked for C=16"
rejects("ctseg_instnorm_finalize", "instnorm_finalize: bad arguments", None, 2, 8, 16, 0, 16, 1.0, 1e-5, p, p, None)
for dt, frag in ((7, "bad dtype 7"), (nat.F32, STRIDE)):
    rejects("ctseg_instnorm_prelu_fwd", frag, dt, p, 10, p, p, None, 0, p, 16, 2, 64, 16, None)
    rejects("ctseg_scale_shift_prelu_fwd", frag, dt, p, 10, p, p, None, 0, p, 16, 2, 64, 16, None)
rejects("ctseg_instnorm_prelu_fwd", "instnorm_prelu_fwd: bad arguments", nat.BF16, None, 16, p, p, None, 0, p, 16, 2, 64, 16, None)
rejects("ctseg_instnorm_prelu_fwd", "instnorm_prelu_fwd: alpha missing", nat.F16, p, 16, p, None, None, 0, p, 16, 2, 64, 16, None)
rejects("ctseg_instnorm_prelu_fwd", "channel stride 18 not chunked", nat.F16, p, 16, None, None, p, 18, p, 16, 2, 64, 16, None)
rejects("ctseg_scale_shift_prelu_fwd", "scale_shift_prelu_fwd: bad arguments", nat.F32, p, 16, None, p, None, 0, p, 16, 2, 64, 16, None)
for dt, C, g_ld, frag in ((7, 16, 16, "bad dtype 7"), (nat.F16, 16, 16, F16_BWD), (nat.F32, 16, 10, STRIDE),
                          (nat.F32, 2048, 2048, "too many channels")):
    rejects("ctseg_instnorm_prelu_bwd_reduce", frag, dt, p, g_ld, p, C, p, p, p, 8, C, 2, 4096, C, None)
    rejects("ctseg_batchnorm_prelu_bwd_reduce", frag, dt, p, g_ld, p, C, p, p, p, p, p, 8, C, 2, 4096, C, None)
    if C <= 256:
        args = (dt, p, g_ld, p, C, p, p, p, p, C, None, 0, 2, 4096, C)
        rejects("ctseg_instnorm_prelu_bwd_apply", frag, *args, None, 0, None, None)
        rejects("ctseg_instnorm_prelu_bwd_apply_colsum", frag, *args, p, 64, p, None, 0, None, None)
        rejects("ctseg_batchnorm_prelu_bwd_apply", frag, dt, p, g_ld, p, C, p, p, p, p, p, p, C, None, 0, 2, 4096, C, None, 0, None,
                None)
    rejects("ctseg_colsum", frag if dt != nat.F16 else "bad dtype 4", dt, p, g_ld, 4096, C, p, 8, p, None)
rejects("ctseg_instnorm_prelu_bwd_reduce", "instnorm_prelu_bwd_reduce: bad arguments", nat.F32, None, 16, p, 16, p, p, p, 8, 16, 2,
        4096, 16, None)
rejects("ctseg_batchnorm_prelu_bwd_reduce", "batchnorm_prelu_bwd_reduce: bad arguments", nat.F32, p, 16, p, 16, p, None, p, p, p, 8,
        16, 2, 4096, 16, None)
# 16-bit storage in 12-wide rows: 8-byte chunks where the pass allows them, rejected by the column sum (16-byte chunks only)
rejects("ctseg_colsum", "channel stride 12 not chunked for C=10", nat.BF16, p, 12, 4096, 10, p, 8, p, None)
rejects("ctseg_instnorm_prelu_bwd_apply", "instnorm_prelu_bwd_apply: bad arguments", nat.F32, p, 16, p, 16, p, p, p, None, 16, None,
        0, 2, 4096, 16, None, 0, None, None)
rejects("ctseg_instnorm_prelu_bwd_apply", "instnorm_prelu_bwd_apply: slope-gradient arguments", nat.F32, p, 16, p, 16, p, p, p, p, 16,
        None, 0, 2, 4096, 16, p, 8, None, None)
rejects("ctseg_batchnorm_prelu_bwd_apply", "batchnorm_prelu_bwd_apply: bad arguments", nat.F32, p, 16, p, 16, p, p, p, p, p, p, 16,
        None, 0, 2, 0, 16, None, 0, None, None)
rejects("ctseg_batchnorm_prelu_bwd_apply", "batchnorm_prelu_bwd_apply: slope-gradient arguments", nat.F32, p, 16, p, 16, p, p, p, p,
        p, p, 16, None, 0, 2, 4096, 16, p, 0, p, None)
ca = (nat.F32, p, 16, p, 16, p, p, p, p, 16, None, 0, 2, 4096)
rejects("ctseg_instnorm_prelu_bwd_apply_colsum", "instnorm_prelu_bwd_apply_colsum: partial buffer", *ca, 16, None, 64, p, None, 0,
        None, None)
rejects("ctseg_instnorm_prelu_bwd_apply_colsum", "instnorm_prelu_bwd_apply_colsum: partial buffer", *ca, 16, p, 1, p, None, 0, None,
        None)
rejects("ctseg_instnorm_prelu_bwd_apply_colsum", "instnorm_prelu_bwd_apply_colsum: partial buffer", nat.F32, p, 512, p, 512, p, p, p,
        p, 512, None, 0, 2, 4096, 512, p, 64, p, None, 0, None, None)
# C = 12: Cv = 3 and a grid stride that is a multiple of 3 needs at least 3 blocks per sample
rejects("ctseg_instnorm_prelu_bwd_apply_colsum", "partial buffer too small for C=12", nat.F32, p, 12, p, 12, p, p, p, p, 12, None, 0,
        2, 4096, 12, p, 5, p, None, 0, None, None)
rejects("ctseg_colsum", "colsum: bad arguments", nat.F32, p, 16, 4096, 16, None, 8, p, None)
rejects("ctseg_instnorm_prelu_bwd_finalize", "instnorm_prelu_bwd_finalize: bad arguments", p, 2, 8, 16, 16, 4096.0, None, p, None, None)
rejects("ctseg_instnorm_prelu_dalpha", "instnorm_prelu_dalpha: bad arguments", p, 32, None, None)
rejects("ctseg_batchnorm_finalize", "batchnorm_finalize: bad arguments", p, 2, 8, 16, 0, 16, 1.0, 1e-5, 0.1, p, p, p, p, None, p, p, None)
rejects("ctseg_batchnorm_eval_table", "batchnorm_eval_table: bad arguments", p, p, p, None, 16, 1e-5, p, None)
rejects("ctseg_batchnorm_prelu_bwd_finalize", "batchnorm_prelu_bwd_finalize: bad arguments", p, 2, 8, 16, 16, 8192.0, p, p, p, None, None)
n += 1
print("SANITIZER-CHILD-OK", n)
