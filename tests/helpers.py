"""Shared test helpers: a one-layer plan around capstone_amd.engine.GemmLayer so single conv modules can be
driven through the C ABI exactly as the UNet plan drives them (same packing, taps, descriptors)."""
import numpy as np
import torch

from capstone_amd import _native as nat
from capstone_amd.engine import Act, GemmLayer, Packer, ParamStore, new_act, rup
from capstone_amd.plan import Plan, _NormAct


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


class ConvPassDriver:
    """One GemmLayer in a MiniPlan, driven one pass at a time with the extras of ctseg_conv_desc (statistics, addend, fp32 / split
    output, backward statistics, a pending norm on the operand).  Every recorded pass is checked against the kernel family the
    caller names (ctseg_conv_pass_name of the recorded descriptor) BEFORE it runs: a shape that an eligibility change moved to
    another kernel fails instead of passing on something else."""

    def __init__(self, mod, dt, device, extra_params=(), cg=None):
        """cg: gathered channel stride of the input when it is not the default (16 for a <= 12-channel input in 12-wide rows)"""
        self.mod, self.dt, self.device = mod, dt, device
        transposed = isinstance(mod, (torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d))
        self.plan = MiniPlan([mod.weight, mod.bias, *extra_params], device, dt, 3)
        e = nat.epc(dt)
        cin = mod.in_channels
        self.layer = GemmLayer(self.plan, "t", transposed, mod.kernel_size[0], mod.stride[0], cin,
                               [(mod.weight, mod.bias, mod.out_channels)], cg or (cin if cin % e else rup(cin, e)),
                               need_dgrad=(cin % e == 0))
        self.plan.packer.finalize()
        self.desc = None

    def act(self, x, ld=None):
        cin = x.shape[1]
        return to_cl(x, self.dt, self.device, ld=ld if ld is not None else (cin if cin == 1 else None))

    def _go(self, family):
        self.desc = self.plan.prog[-1][2][0]
        name = nat.lib().ctseg_conv_pass_name(self.desc)
        assert name is not None and name.decode() == family, (name, family)
        self.plan.run()
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


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))
