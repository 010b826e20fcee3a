"""Shared test helpers: a one-layer plan around capstone_amd.engine.GemmLayer so single conv modules can be
driven through the C ABI exactly as the UNet plan drives them (same packing, taps, descriptors); the names, grid caps and error
bounds the op-level tests share (the float64 references themselves: reference_ops.py)."""
import json
import os
import zlib

import numpy as np
import torch

from capstone_amd import _native as nat
from capstone_amd._native import BF16, F16, F32
from capstone_amd.engine import Act, GemmLayer, Packer, ParamStore, new_act, rup
from capstone_amd.plan import Plan, _NormAct
from reference_ops import conv_dgrad, conv_fwd, conv_module, conv_out_shape, rounded


class MiniPlan:
    """duck-typed stand-in for plan.Plan holding one or more GemmLayers"""

    def __init__(self, params, device, dt, dims):
        self.device, self.dt, self.dims = torch.device(device), dt, dims
        self.store = ParamStore(params, self.device)
        self.packer = Packer(self)
        self.prog, self._keep, self.need_input_grad = [], [], True
        self.ready_marks = []

    def emit(self, name, *args, keep=()):
        self._keep.append((args, keep))
        self.prog.append((name, getattr(nat.lib(), name), tuple(args)))

    emit_colsum = Plan.emit_colsum

    def grads_ready(self, params):
        pass

    def run(self):
        self.packer.refresh(force=True)
        Plan.run(self.prog, nat.stream_ptr())
        self.prog = []


def to_cl(x, dt, device, ld=None):
    """(N,C,*sp) fp32 cpu tensor -> Act (channels-last storage on device)"""
    if x.ndim == 4:
        x = x.unsqueeze(-1)
    N, C = x.shape[:2]
    a = new_act(N, x.shape[2], x.shape[3], x.shape[4], C, dt, device, ld=ld)
    a.t[..., :C].copy_(x.permute(0, 2, 3, 4, 1).to(device))
    return a


def from_cl(a, two_d=False):
    v = a.valid().float().cpu()
    return v[..., 0] if two_d else v


def run_conv_module(mod, x, gy, dt, device):
    """forward, input-gradient and weight-gradient of one torch conv module through the HIP passes.
    Returns (y, gx, gw, gb) as fp32 cpu tensors in torch layout."""
    transposed = isinstance(mod, (torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d))
    dims = 3 if mod.weight.ndim == 5 else 2
    plan = MiniPlan([mod.weight, mod.bias], device, dt, dims)
    e = nat.epc(dt)
    cin = mod.in_channels
    xa = to_cl(x, dt, device, ld=cin if cin % e else None)
    layer = GemmLayer(plan, "t", transposed, mod.kernel_size[0], mod.stride[0], cin, [(mod.weight, mod.bias, mod.out_channels)],
                      cin if cin % e else rup(cin, e), need_dgrad=(cin % e == 0))
    plan.packer.finalize()
    y, _ = layer.emit_fwd(xa)
    plan.run()
    ga = to_cl(gy, dt, device)
    gx = None
    if layer.dg_pack is not None:
        gxa = layer.emit_dgrad(ga)
        plan.run()
        gx = from_cl(gxa, dims == 2)
    if dt == nat.F16:           # IEEE half storage: forward / input-gradient passes only (no weight-gradient kernels)
        torch.cuda.synchronize()
        return from_cl(y, dims == 2), gx, None, None
    layer.emit_wgrad(xa, ga)
    plan.run()
    torch.cuda.synchronize()
    gw = plan.store.grad_view(mod.weight).cpu().clone()
    gb = plan.store.grad_view(mod.bias).cpu().clone()
    return from_cl(y, dims == 2), gx, gw, gb


def autograd_conv_module(mod, shape):
    """operands of one conv module drawn from torch's global generator (the caller seeds it: x of (N, *spatial) = ``shape``, then dY)
    and torch's float32 autograd on the CPU -> (x, gy, y, gx); the weight / bias gradient are left on the module's parameters"""
    x = torch.randn(shape[0], mod.in_channels, *shape[1:])
    xr = x.clone().requires_grad_(True)
    y = mod(xr)
    gy = torch.randn_like(y)
    y.backward(gy)
    return x, gy, y.detach(), xr.grad


def check_conv_module(mod, shape, dt, device, tol):
    """all four passes of the module (the input gradient where the layer has one) against autograd_conv_module, by rel_err"""
    x, gy, y, gx_ref = autograd_conv_module(mod, shape)
    yy, gx, gw, gb = run_conv_module(mod, x, gy, dt, device)
    assert rel_err(yy, y) < tol, "forward"
    assert (gx is None) == (mod.in_channels == 1)
    if gx is not None:
        assert rel_err(gx, gx_ref) < tol, "input gradient"
    assert rel_err(gw, mod.weight.grad) < tol, "weight gradient"
    assert rel_err(gb, mod.bias.grad) < tol, "bias gradient"


class ConvPassDriver:
    """One GemmLayer in a MiniPlan, driven one pass at a time with the extras of ctseg_conv_desc (statistics, addend, fp32 / split
    output, backward statistics, a pending norm on the operand).  Every recorded pass is checked against the kernel family the
    caller names (ctseg_conv_pass_name of the recorded descriptor) BEFORE it runs: a shape that an eligibility change moved to
    another kernel fails instead of passing on something else."""

    def __init__(self, mod, dt, device, extra_params=(), cg=None, dims=3, guard_params=()):
        """cg: gathered channel stride of the input when it is not the default (16 for a <= 12-channel input in 12-wide rows);
        guard_params: a (before, after) pair of parameters laid around the layer's own in the flat buffers"""
        # ``mod``: one conv module, or the (residual, unit0) pair of a strided residual unit: same input and geometry, ONE GemmLayer of
        # two parts whose columns are [residual | unit0], as plan._ResUnit builds it.  self.mod is the first part
        self.mods = mods = list(mod) if isinstance(mod, (list, tuple)) else [mod]
        self.mod = mod = mods[0]
        self.dt, self.device = dt, device
        transposed = isinstance(mod, (torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d))
        own = [p for m in mods for p in (m.weight, m.bias)]
        self.plan = MiniPlan([*guard_params[:1], *own, *guard_params[1:], *extra_params], device, dt, dims)
        e = nat.epc(dt)
        cin = mod.in_channels
        self.layer = GemmLayer(self.plan, "t", transposed, mod.kernel_size[0], mod.stride[0], cin,
                               [(m.weight, m.bias, m.out_channels) for m in mods], cg or (cin if cin % e else rup(cin, e)),
                               need_dgrad=(cin % e == 0))
        self.plan.packer.finalize()
        self.desc = self.prog = None

    def act(self, x, ld=None):
        cin = x.shape[1]
        return to_cl(x, self.dt, self.device, ld=ld if ld is not None else (cin if cin == 1 else None))

    def _go(self, family):
        self.desc = self.plan.prog[-1][2][0]
        name = nat.lib().ctseg_conv_pass_name(self.desc)
        assert name is not None and name.decode() == family, (name, family)
        self.prog = list(self.plan.prog)
        self.plan.run()
        torch.cuda.synchronize()

    def replay(self):
        """runs the program of the last pass again, as recorded (same descriptor, same buffers)"""
        Plan.run(self.prog, nat.stream_ptr())
        torch.cuda.synchronize()

    def fwd(self, family, xa, **extras):
        """-> (output Act or SplitAct, NormStats or None); extras: want_stats, add, out_f32, split_at, out"""
        out, stats = self.layer.emit_fwd(xa, **extras)
        self._go(family)
        return out, stats

    def set_input_dims(self, dims):
        self.layer.x_dims = tuple(dims)

    def dgrad(self, family, ga, **extras):
        """-> the written gradient (Act or SplitAct); extras: add, bst, bst_col0, split_at, out.  Needs the input dims of a forward
        (a forward pass recorded before, or set_input_dims)"""
        out = self.layer.emit_dgrad(ga, **extras)
        self._go(family)
        return out


ACT_SENTINEL = -12288.0      # -3 * 2^12: exact in bf16, fp16 and fp32


def sentinel_act(dims, C, dt, device, ld, c0=0):
    """an output Act the caller prepares: ``C`` channels from column ``c0`` of rows ``ld`` wide, every element of the buffer set to
    ACT_SENTINEL (what a pass leaves of it shows which columns it wrote)"""
    buf = new_act(*dims, ld, dt, device, ld=ld)
    buf.t.fill_(ACT_SENTINEL)
    return buf.slice(c0, C) if (c0 or C != ld) else buf


def wide_act(x, dt, device, c0, tail, fill):
    """(N,C,*sp) cpu tensor -> Act that is the column slice [c0, c0 + C) of a buffer c0 + C + tail wide whose other columns hold
    ``fill``: an operand as a pass gathers it from a wider tensor (a half of the skip concat)"""
    if x.ndim == 4:
        x = x.unsqueeze(-1)
    N, C = x.shape[:2]
    buf = new_act(N, x.shape[2], x.shape[3], x.shape[4], c0 + C + tail, dt, device, ld=c0 + C + tail)
    buf.t.fill_(fill)
    buf.t[..., c0:c0 + C].copy_(x.permute(0, 2, 3, 4, 1).to(device))
    return buf.slice(c0, C)


# ---- one forward / input-gradient pass of one layer against the float64 convolution (test_gpu_conv_exact.py, test_gpu_conv2d_exact.py) ----
CONV_ENV_KEYS = ("CTSEG_MAX_WG", "CTSEG_NO_HALO_X", "CTSEG_NO_DOWN_R")


class ConvCase:
    """one pass ("fwd" / "dgrad") of one layer, on the kernel family it is written for.  shape: (N, *spatial) of the layer's INPUT;
    wd: P(nonzero) of the {-1, 0, 1} weights; g_ld / o_ld: row width of the gathered / written tensor where not the default;
    cg: gathered channel stride of the layer's input where not the default; wide: largest integer of the large-magnitude run"""

    def __init__(self, name, pas, family, kind, cin, cout, shape, dt=BF16, k=3, wd=2 / 3, env=None, g_ld=None, o_ld=None, cg=None,
                 out_f32=False, wide=4):
        self.name, self.pas, self.family, self.kind, self.cin, self.cout, self.shape = name, pas, family, kind, cin, cout, tuple(shape)
        self.dt, self.k, self.wd, self.env, self.g_ld, self.o_ld, self.cg = dt, k, wd, env or {}, g_ld, o_ld, cg
        self.out_f32, self.wide = out_f32, wide
        self.dims = len(shape) - 1

    @property
    def persistent(self):
        """every family but the generic / ring tiles sizes its grid with persistent_grid: CTSEG_MAX_WG caps it"""
        return not self.family.startswith("generic")

    @property
    def id(self):
        st = {BF16: "", F16: " fp16", F32: " fp32"}[self.dt]
        return f"{self.name} | {self.pas} {self.kind} {self.cin}->{self.cout} {self.shape}{st}".replace(" ", "_")

    def with_dt(self, dt):
        return ConvCase(self.name, self.pas, self.family, self.kind, self.cin, self.cout, self.shape, dt, self.k, self.wd, self.env, self.g_ld,
                     self.o_ld, self.cg, self.out_f32, self.wide)

    def setenv(self, monkeypatch, cap=None):
        for k in CONV_ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        cap_env(monkeypatch, cap)


class ConvOps:
    """seeded operands of a case's LAYER (kind, channels, shape, kernel size) in one mode, with the CPU references of both passes:
    made once per (layer, mode), shared by every test and cap, never written to.
    mode: "unit" ({-1, 0, 1}, integer bias in [-2, 2]), "wide" (integers in [-wide, wide], same bias), ("randn", dt) (normal values
    rounded to the storage type, the bias kept in fp32 as the library keeps it)"""
    _cache = {}

    @classmethod
    def of(cls, case, mode):
        key = (case.kind, case.cin, case.cout, case.shape, case.k, mode, case.wd if mode == "unit" else None,
               case.wide if mode == "wide" else None)
        if key not in cls._cache:
            cls._cache[key] = cls(case, mode, zlib.crc32(repr(key).encode()))
        return cls._cache[key]

    def __init__(self, case, mode, seed):
        g = torch.Generator().manual_seed(seed)
        self.kind, self.k = case.kind, case.k
        mod = conv_module(case.kind, case.cin, case.cout, case.k, case.dims)
        N, sp = case.shape[0], case.shape[1:]
        xs = (N, case.cin) + sp
        ys = (N, case.cout) + conv_out_shape(case.kind, case.k, sp)
        ws = tuple(mod.weight.shape)
        if mode == "unit":
            def tern(shape, p):
                return ((torch.randint(0, 2, shape, generator=g) * 2 - 1) * (torch.rand(shape, generator=g) < p)).float()
            self.x, self.w, self.gy = tern(xs, 2 / 3), tern(ws, case.wd), tern(ys, 2 / 3)
            self.b = torch.randint(-2, 3, (case.cout,), generator=g).float()
        elif mode == "wide":
            m = case.wide
            self.x, self.w, self.gy = (torch.randint(-m, m + 1, s, generator=g).float() for s in (xs, ws, ys))
            self.b = torch.randint(-2, 3, (case.cout,), generator=g).float()
        else:
            tdt = nat.torch_dtype(mode[1])
            fan = case.cin * case.k ** case.dims
            self.x, self.gy = (torch.randn(s, generator=g).to(tdt).float() for s in (xs, ys))
            self.w = (torch.randn(ws, generator=g) * fan ** -0.5).to(tdt).float()
            self.b = torch.randn(case.cout, generator=g) * 0.5
        self._ref = {}

    def module(self, case):
        mod = conv_module(case.kind, case.cin, case.cout, case.k, case.dims)
        with torch.no_grad():
            mod.weight.copy_(self.w)
            mod.bias.copy_(self.b)
        return mod

    def ref(self, pas, f32=False):
        """float64 (``f32``: torch float32) evaluation of the pass on the CPU"""
        key = (pas, f32)
        if key not in self._ref:
            x, w, b, gy = ((t if f32 else t.double()) for t in (self.x, self.w, self.b, self.gy))
            with torch.no_grad():
                self._ref[key] = conv_fwd(self.kind, self.k, x, w, b) if pas == "fwd" else conv_dgrad(self.kind, self.k, gy, w, self.x.shape)
        return self._ref[key]


class ConvRun:
    """one recorded and executed pass over an output buffer the test prepared (every element ACT_SENTINEL before the pass)"""

    def __init__(self, case, ops, layout="padded"):
        """layout: "padded" (the written columns, then one more 16-byte chunk of the buffer), "dense" (rows exactly Cn_store wide, the
        gathered operand in rows of its own), "sliced" (the output a column slice at c0 > 0 of a buffer with a further chunk behind
        it, the gathered operand a column slice of a wider buffer whose other columns hold the integer 3)"""
        dt = case.dt
        self.case = case
        drv = self.drv = ConvPassDriver(ops.module(case), dt, DEV, cg=case.cg, dims=case.dims)
        e = nat.epc(dt)
        N, sp = case.shape[0], case.shape[1:] + (1,) * (3 - case.dims)
        xd = (N,) + sp
        odt = F32 if case.out_f32 else dt
        eo = nat.epc(odt)
        fwd = case.pas == "fwd"
        src = ops.x if fwd else ops.gy
        sliced_in = layout == "sliced" and case.g_ld is None and src.shape[1] % e == 0
        if sliced_in:
            ga = wide_act(src, dt, DEV, e, e, 3.0)
        elif fwd:
            ga = drv.act(src, ld=case.g_ld)
        else:
            ga = to_cl(src, dt, DEV, ld=case.g_ld)
        self.sliced_in = sliced_in
        Cn = case.cout if fwd else case.cin
        od = drv.layer.out_dims(xd) if fwd else xd
        narrow = case.o_ld == 12
        Cs = rup(Cn, 4 if (case.out_f32 or narrow) else eo)
        self.c0 = c0 = eo if layout == "sliced" else 0
        ld = case.o_ld if narrow else c0 + Cs + (0 if layout == "dense" else eo)
        self.out = out = sentinel_act(od, Cn, odt, DEV, ld, c0)
        if fwd:
            drv.fwd(case.family, ga, out=out, out_f32=case.out_f32)
        else:
            drv.set_input_dims(xd)
            drv.dgrad(case.family, ga, out=out)
        d = drv.desc
        assert d.Cn == Cn and d.Cn_store == Cs and d.o_ld == ld and d.g_ld == ga.ld, (d.Cn, d.Cn_store, d.o_ld, d.g_ld)
        self.Cn, self.Cs, self.ld = Cn, Cs, ld

    def buffer(self):
        """the whole output buffer as float64 on the CPU: (N, X, Y, Z, ld)"""
        return self.out.t.cpu().double()

    def check_columns(self, want, what):
        """``want``: (N, Cn, *spatial) float64, the values columns [0, Cn) of the pass must hold bit for bit; columns [Cn, Cn_store)
        must be zero and every other column of the buffer must still hold the sentinel"""
        T = self.buffer()
        if want.ndim == 4:
            want = want.unsqueeze(-1)
        c0, Cn, Cs = self.c0, self.Cn, self.Cs
        got = T[..., c0:c0 + Cn].permute(0, 4, 1, 2, 3)
        bad = got != want
        nbad = int(bad.sum())
        if nbad:
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {nbad} of {bad.numel()} elements differ from the reference; first at (n, c, x, y, z) = {i}: "
                                 f"got {float(got[i])}, expected {float(want[i])}")
        pad = T[..., c0 + Cn:c0 + Cs]
        assert bool((pad == 0).all()), f"{what}: pad columns [Cn, Cn_store) = [{Cn}, {Cs}) are not zero: {pad.unique()[:8].tolist()}"
        for lo, hi in ((0, c0), (c0 + Cs, self.ld)):
            rest = T[..., lo:hi]
            assert bool((rest == ACT_SENTINEL).all()), f"{what}: columns [{lo}, {hi}) outside the pass changed: {rest.unique()[:8].tolist()}"
        return T


def conv_exact_run(case, mode, layout="padded", ops=None):
    """the integer run of a case -> (ConvRun, float64 reference); asserts the exactness condition of the storage type on the reference.
    ``ops``: the case's operands where they are not ConvOps.of(case, mode)"""
    ops = ops or ConvOps.of(case, mode)
    ref = ops.ref(case.pas)
    cap = EXACT_CAP[F32 if case.out_f32 else case.dt]
    top = float(ref.abs().max())
    nz = float((ref != 0).double().mean())
    print(f"{case.id} [{mode}]: max |ref| {top:.0f} (cap {cap:.0f}), nonzero {100 * nz:.1f} %")
    if mode == "unit" or case.dt == F32 or case.out_f32:
        assert top <= cap if cap < 2.0 ** 24 else top < cap, ("the reference leaves the exactly representable integers", top, cap)
    return ConvRun(case, ops, layout), ref


GRAD_SENTINEL = -12345.0


class WgradPassDriver(ConvPassDriver):
    """The weight-gradient pass of one GemmLayer (emit_wgrad: the pass, its slab reduce, the column sum of a transposed layer's
    bias), checked by name (ctseg_wgrad_pass_name of the recorded descriptor) BEFORE anything runs.  The flat gradient buffer is
    filled with a sentinel first and the layer's parameters lie between two guard parameters in it, so a write outside the
    layer's weight and bias views shows; the slab buffer the descriptor records can be poisoned, and the recorded program can be
    run again over its own stale slabs (replay) after new operands were copied into the same tensors."""

    def __init__(self, mod, dt, device, cg=None, extra_params=()):
        self.guards = (torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(8)))
        first = mod[0] if isinstance(mod, (list, tuple)) else mod
        super().__init__(mod, dt, device, extra_params=extra_params, cg=cg, dims=3 if first.weight.ndim == 5 else 2,
                         guard_params=self.guards)
        self.prog = self.ws = None

    def act(self, x, ld=None):
        """operand with rows ``ld`` wide (default: 16-byte chunked)"""
        return to_cl(x, self.dt, self.device, ld=ld)

    def record(self, family, xa, ga, splits=None, **extras):
        """records emit_wgrad(xa, ga, **extras) and asserts the family; ``splits`` overrides the mirror's split rule (the C ABI takes
        any count: an empty last split is not reachable through GemmLayer._wgrad_splits)"""
        if splits is not None:
            self.layer._wgrad_splits = lambda *a: splits
        n0 = len(self.plan.prog)
        self.layer.emit_wgrad(xa, ga, **extras)
        idx = [i for i in range(n0, len(self.plan.prog)) if self.plan.prog[i][0] == "ctseg_conv_wgrad"]
        assert len(idx) == 1
        self.desc = self.plan.prog[idx[0]][2][0]
        name = nat.lib().ctseg_wgrad_pass_name(self.desc)
        assert name is not None and name.decode() == family, (name, family)
        self.ws = [k for a, k in self.plan._keep if a and a[0] is self.desc][0][2]
        assert self.ws.data_ptr() == self.desc.ws
        return self.desc

    def go(self, poison=None):
        """fills the flat gradient with the sentinel (and the slabs with ``poison``), runs what is recorded
        -> (gw, gb, desc, flat_g) on the CPU"""
        if self.plan.prog:
            self.prog = list(self.plan.prog)
            self.plan.prog = []
            self.plan.packer.refresh(force=True)
        if poison is not None:
            self.ws.fill_(poison)
        st = self.plan.store
        st.flat_g.fill_(GRAD_SENTINEL)
        Plan.run(self.prog, nat.stream_ptr())
        torch.cuda.synchronize()
        return (st.grad_view(self.mod.weight).cpu().clone(), st.grad_view(self.mod.bias).cpu().clone(), self.desc, st.flat_g.cpu().clone())

    def part_grads(self, flat_g):
        """[(weight gradient, bias gradient)] of every part of the layer, cut out of the flat gradient ``go`` returned"""
        st = self.plan.store
        return [tuple(flat_g[st.off(p):st.off(p) + p.numel()].reshape(p.shape).clone() for p in (m.weight, m.bias)) for m in self.mods]

    def outside_untouched(self, flat_g):
        """no entry of the flat gradient outside the layer's weight and bias views changed from the sentinel"""
        return self.outside_untouched_but(flat_g)

    def outside_untouched_but(self, flat_g, *also):
        """the same, with further parameters (``also``) whose gradient the recorded program may write"""
        st = self.plan.store
        keep = torch.ones(flat_g.numel(), dtype=torch.bool)
        for p in (*(q for m in self.mods for q in (m.weight, m.bias)), *also):
            keep[st.off(p):st.off(p) + p.numel()] = False
        return int(keep.sum()) >= 16 and bool((flat_g[keep] == GRAD_SENTINEL).all())


def norm_for(drv, alpha, N, C, dims, seed, eps=1e-5):
    """a _NormAct with a real forward output y (bf16-rounded, no element within 1e-3 of its mean in units of the standard
    deviation: the sign of xhat decides a PReLU branch, and float32 and float64 must agree on it) and its real (mean, rstd)
    -> (norm, y, mean, rstd); mean / rstd: the float32 table values as float64, shaped (N, C, 1, 1, 1)"""
    torch.manual_seed(seed)
    y = rounded(torch.randn(N, C, *dims) * 1.3 + 0.4, torch.bfloat16)
    mean = y.double().mean((2, 3, 4), keepdim=True)
    rstd = (y.double().var((2, 3, 4), unbiased=False, keepdim=True) + eps).rsqrt()
    mr32 = torch.stack([mean.float().reshape(N, C), rstd.float().reshape(N, C)], -1).contiguous()
    m32, r32 = mr32[..., 0].double().reshape(N, C, 1, 1, 1), mr32[..., 1].double().reshape(N, C, 1, 1, 1)
    for _ in range(3):
        near = ((y.double() - m32) * r32).abs() < 1e-3
        y = rounded(torch.where(near, y + 0.25, y), torch.bfloat16)
    assert float(((y.double() - m32) * r32).abs().min()) >= 1e-3
    na = _NormAct(drv.plan, alpha)
    na.y = to_cl(y, nat.BF16, drv.device)
    na.mr = mr32.to(drv.device)
    return na, y, m32, r32


# ---- kernel family names (ctseg_conv_pass_name) and grid caps -----------------------------------------------------------------
HALO_X, HALO, UP, STEM, HALO_SW = "x-column halo", "halo", "up", "stem", "streamed-weight halo"
DOWN_HALO, DOWN_R, UP8 = "stride-2 halo", "stride-2 register-weight", "many-channel 8-class"
G16, G32, G64, G128, G256 = "generic 256x16", "generic 256x32", "generic 128x64", "generic 128x128", "generic 192x256"
RING128, RING256 = "generic ring 192x128", "generic ring 192x256"
CAPS = [None, "1", "3"]      # CTSEG_MAX_WG: several tiles per workgroup of a persistent kernel
CAP_IDS = ["uncapped", "max_wg1", "max_wg3"]


def cap_env(monkeypatch, max_wg):
    monkeypatch.delenv("CTSEG_MAX_WG", raising=False)
    if max_wg is not None:
        monkeypatch.setenv("CTSEG_MAX_WG", max_wg)


def dump(out_dir, name, obj):
    """a test's figures as JSON under ``out_dir`` (best effort: a read-only tree is no failure)"""
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, name), "w") as f:
            json.dump(obj, f, indent=1)
    except OSError:
        pass


TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}      # storage type -> torch dtype (reference_ops.rounded)
# ---- the error bounds -----------------------------------------------------------------------------------------------------------
EXACT_CAP = {BF16: 256.0, F16: 2048.0, F32: 2.0 ** 24}      # below it every integer is a value of the storage type
REL_TOL = {F32: 2e-5, BF16: 2.5e-2}                         # max |error| / max |reference| of a whole tensor (rel_err)
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -10, F32: 0.0}          # one unit in the last place, relative (fp32: the e32 term alone)


def elem_bound(ref64, ref32, dt):
    """per element: u * |ref64| + 16 * e32, e32 the largest |float32 - float64| evaluation of the case -> (bound, e32)"""
    e32 = float((ref32.double() - ref64).abs().max())
    assert e32 > 0.0
    return ULP[dt] * ref64.abs() + 16.0 * e32, e32


def check_elems(tag, got, ref64, ref32, dt):
    """every element: |got - ref64| <= u * |ref64| + 16 * e32"""
    bound, e32 = elem_bound(ref64, ref32, dt)
    ratio = float(((got.double() - ref64).abs() / bound).max())
    print(f"{tag}: worst error / bound {ratio:.3f} (e32 {e32:.2e})")
    assert ratio <= 1.0, (tag, ratio)
    return ratio


def sum_bound(tag, t64, t32, dims, rows, div=1.0):
    """-> (float64 sums of t64 over ``dims``, sums of |terms| (1 where none is nonzero), which sums have a nonzero term, bound on the error
    normalised by them: 16 x that of the plain float32 evaluation (sum / div, as the kernel stores it), under 1 / (4 * rows))"""
    s64, a64 = t64.sum(dims), t64.abs().sum(dims)
    s32 = (t32.sum(dims) / div).double() * div
    live = a64 > 0
    norm = torch.where(live, a64, torch.ones_like(a64))
    f32 = float(((s32 - s64).abs() / norm)[live].max())
    bound, cap = 16.0 * f32, 1.0 / (4.0 * rows)
    assert 0.0 < bound < cap, (tag, "float32 reference error x 16 is not inside (0, 1 / (4 * rows)): shrink the shape", bound, cap)
    return s64, norm, live, bound


def ulp32(s):
    """spacing of fp32 at |s| (float64 tensor)"""
    _, e = torch.frexp(s.abs())
    return torch.where(s == 0, torch.full_like(s, 2.0 ** -149), torch.pow(2.0, (e - 24).double()))


DEV = "cuda:0"


def on_device(*arrays):
    """numpy arrays (read-only ones too) -> tensors on the GPU: one for one array, a tuple for several"""
    t = tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)
    return t[0] if len(t) == 1 else t


def as_numpy(out):
    """a tuple of tensors -> a tuple of arrays; a result object -> the dict of its fields as arrays"""
    if isinstance(out, (tuple, list)):
        return tuple(t.cpu().numpy() for t in out)
    return {k: v.cpu().numpy() for k, v in vars(out).items()}


def check_bit_exact(got, ref):
    """a 2-D pipeline's outputs (nine masks and squashing) against its oracle's, array_equal on every one"""
    assert got["image"].dtype == np.float32 and ref["image"].dtype == np.float32
    diff = np.abs(got["image"].astype(np.float64) - ref["image"])
    print("image: max |diff|", float(diff.max()), "differing", int((got["image"] != ref["image"]).sum()), "of", diff.size)
    assert np.array_equal(got["image"], ref["image"])
    assert np.array_equal(got["image_sq"], ref["image"])
    assert np.array_equal(got["masks"], ref["masks"])
    assert np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["flat"], ref["labels"].reshape(len(ref["labels"]), -1))
    assert np.array_equal(got["hist"], ref["hist"])
    assert np.array_equal(got["hist"], np.stack([np.bincount(l.reshape(-1), minlength=10) for l in got["labels"]]))
    assert np.array_equal(got["present"], ref["present"]) and np.array_equal(got["present_sq"], ref["present"])


def swapped_oracle(dims, cin, cout, channels, strides, nres):
    """MONAI's UNet with norm=Norm.BATCH: the oracle with each Convolution's InstanceNorm replaced by BatchNorm (same place)"""
    from oracle.monai_unet import Convolution, UNet
    net = UNet(dims, cin, cout, channels, strides, num_res_units=nres)
    for m in net.modules():
        if isinstance(m, Convolution) and "norm" in m._modules:
            m.norm = {2: torch.nn.BatchNorm2d, 3: torch.nn.BatchNorm3d}[dims](m.norm.num_features)
    return net


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def rel_err_nonzero(x, x64):
    """(max, rms) of |x - x64| / |x64| over x64 != 0, and whether x is exactly 0 wherever x64 is (numpy arrays)"""
    nz = x64 != 0
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.abs(x[nz].astype(np.float64) - x64[nz]) / np.abs(x64[nz])
        return float(r.max()), float(np.sqrt(np.mean(r * r))), bool((x[~nz] == 0).all())
