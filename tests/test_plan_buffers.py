"""The whole-step buffer contract.  Every device buffer of a plan, its layer objects and its loss engines is entered into a registry
with a role (capstone_amd.engine: scratch / zero-on-entry, self-restoring / zero, never written / zero where unwritten / state;
DESIGN.md "Buffer roles").

CPU (unmarked, under the ABI emulator): the registry is complete (every tensor reachable from a plan lies inside a registered
allocation, no two allocations overlap, the entries of one allocation partition it) and the pad columns it reports are the ones
``default_ld`` / ``narrow_rows`` give.

GPU: the assembled training step computes the SAME BITS (loss, logged Dice, logits, d loss / d logits, Dice counts, the flat
gradient, parameters and Adam moments after the update, BatchNorm running statistics)
  (a) over a workspace whose every scratch buffer holds NaN, then a large finite value (0xA5 bytes in integer buffers); afterwards
      every zero-on-entry buffer is zero again and every never-written range holds what it held; the never-written ranges are also
      filled with a sentinel before a step and must come back bit-unchanged;
  (b) on a plan that ran other batches before as on a fresh one, for one step and for three steps with the updates in between;
  (c) and when (a) fails, the step runs once per registered scratch buffer with only that buffer poisoned: the message names the
      buffers whose content reaches a result.
Each test first asserts that two plain runs of the step from the same state are bit-identical.

The fused head materialises neither logits nor predictions: for its configurations d loss / d logits and the integer Dice counts
(|pred == c & true == c|, |pred == c|, |true == c| per sample and class, taken from the same argmax) stand in for them.

Row layouts.  The library lays the tensors around the 10-class head out 12 wide where every pass can move such rows: with 16
channels on the first level ("3d-bf16-narrow", with and without the fused head; asserted through plan.narrow_rows and the ld of
d loss / d logits and of the head's activations), not with 8 channels there and never for a 2-D plan (depth 1), which the other
configurations assert as the 16-wide layout they get.  The unwritten elements of a "zero where unwritten" buffer are found with a
sentinel run of the code under test, so for the statistics partials this file shows that the unwritten set is stable and zero, not
that it is the right set (a record that should be written and is not: the op and parity tests); for the pad of d loss / d logits the
expected set is derived here: columns 12..15 of a 16-wide row under the fused head, none otherwise.

What the tests found on an MI355X (now declared "zero where unwritten", with the reason at the call site): the statistics partials of
a conv pass (the stem's: poisoning them alone changed every logit, NaN and finite alike) and the pad columns of d loss / d logits
under the fused head (columns 12..15 of a 16-wide row; NaN only: 0 x NaN against zero-packed weights).  With the fused head's
per-sample record fix reverted in a scratch build, (a) fails on "3d-bf16-fused-head" and names "loss/head partial records"."""
import functools

import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import _native as nat
from capstone_amd import engine as E
from capstone_amd import segloss
from capstone_amd.engine import SCRATCH, STATE, ZERO_PAD, ZERO_RESTORED, ZERO_UNWRITTEN, Act, default_ld
from helpers import ACT_SENTINEL

DEV = "cuda:0"
N_CLASSES = 10
F3 = [8, 16, 32]                       # three levels: spatial sizes are multiples of 4
F3_NARROW = [16, 16, 32]               # 16 channels either side of the head: the library takes 12-wide rows at this volume
F2 = [8, 16, 32, 32, 32]               # the 2-D trainers take five widths: spatial sizes are multiples of 16
# 12 x 20 x 12: three 4-row tiles in x, ragged 8-wide tiles in y and z; 6 x 10 x 6 and 3 x 5 x 3 on the levels below
SP3, SP2 = (12, 20, 12), (48, 32)


def _cfg(kind, precision="bf16", losses=("CrossEntropy", "Dice"), N=2, env=None, norm="INSTANCE", keep_logits=True, boundary=False,
         inference=False, filters=None):
    return dict(filters=list(filters or (F3 if kind == "3d" else F2)), narrow=filters is F3_NARROW, kind=kind, precision=precision, losses=list(losses), N=N, env=env or {}, norm=norm, keep_logits=keep_logits,
                boundary=boundary, inference=inference)


CONFIGS = {
    "3d-bf16": _cfg("3d"),
    "3d-fp32": _cfg("3d", "fp32"),
    "3d-bf16-max_wg3": _cfg("3d", env={"CTSEG_MAX_WG": "3"}),
    "3d-bf16-one-stream": _cfg("3d", env={"CTSEG_SIDE_STREAM": "0"}),
    # the fused head (logits convolution + cross-entropy in one launch) runs for a cross-entropy-only step that does not keep the
    # logits; three samples: a workgroup's tile walk can pass over a whole sample (the stale-record bug of the head's partial records)
    "3d-bf16-fused-head": _cfg("3d", losses=("CrossEntropy",), N=3, keep_logits=False),
    "3d-bf16-fused-head-max_wg3": _cfg("3d", losses=("CrossEntropy",), N=3, keep_logits=False, env={"CTSEG_MAX_WG": "3"}),
    # 12-wide rows around the head: the pad of d loss / d logits is columns 10..11, which every writer stores
    "3d-bf16-narrow": _cfg("3d", filters=F3_NARROW),
    "3d-bf16-narrow-fused-head": _cfg("3d", losses=("CrossEntropy",), N=3, keep_logits=False, filters=F3_NARROW),
    "3d-bf16-batchnorm": _cfg("3d", norm="BATCH"),
    "2d-res2-bf16": _cfg("2d", losses=("Dice", "Focal"), N=3),
    "2d-mixup-bf16": _cfg("mixup", losses=("Dice", "Focal"), N=3),
    "3d-bf16-boundary": _cfg("3d", losses=("Boundary", "CrossEntropy"), boundary=True),
    "3d-fp16-inference": _cfg("3d", "fp16", inference=True),
}
IDS = list(CONFIGS)


def _set_env(monkeypatch, cfg):
    for k in ("CTSEG_MAX_WG", "CTSEG_SIDE_STREAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)


def _module(cfg, device):
    """the trainer of a configuration, the same weights every time (seeded), on ``device``"""
    from capstone_amd.models import UNet
    from capstone_amd.training.base_trainer import BaseUNet2D
    from capstone_amd.training.mixup_trainer import MixupUNet2D
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(20)
    kw = dict(loss_fx=list(cfg["losses"]), precision=16 if cfg["precision"] == "fp16" else cfg["precision"])
    if cfg["kind"] == "3d":
        m = BaseUNet3D(filters=list(cfg["filters"]), device_boundary=cfg["boundary"], **kw)
        if cfg["norm"] == "BATCH":
            torch.manual_seed(20)
            m.unet = UNet(3, 1, N_CLASSES, list(cfg["filters"]), [2, 2], num_res_units=2, norm="BATCH", precision=cfg["precision"])
    else:
        cls = MixupUNet2D if cfg["kind"] == "mixup" else BaseUNet2D
        m = cls(filters=list(cfg["filters"]), use_res_units=True, transform_degree=0, **kw)
    with torch.no_grad():          # distinct PReLU slopes, BatchNorm weights off their initial 1 / 0
        g = torch.Generator().manual_seed(21)
        for p in m.unet.parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.rand(p.shape, generator=g))
    return m.to(device)


def _labels(N, sp, seed, special):
    """(N, *sp) label map in [0, 10): blocks of every class; ``special``: sample 0 has class 5 missing, sample 1 is all background"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, N_CLASSES, (N,) + tuple((s + 3) // 4 for s in sp), generator=g)
    for d, s in enumerate(sp):
        lab = lab.repeat_interleave(4, dim=d + 1).narrow(d + 1, 0, s)
    noise = torch.rand(lab.shape, generator=g) < 0.1
    lab = torch.where(noise, torch.randint(0, N_CLASSES, lab.shape, generator=g), lab)
    if special:
        lab[0][lab[0] == 5] = 0
        lab[1] = 0
    return lab


def _batch(cfg, which, device):
    """batch "A" or "B" of a configuration: (images, masks (N, 9, *sp) uint8, indicator[, distance maps])"""
    sp = SP3 if cfg["kind"] == "3d" else SP2
    N = cfg["N"]
    seed = {"A": 100, "B": 200}[which]
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(N, 1, *sp, generator=g)
    lab = _labels(N, sp, seed + 1, special=which == "B")
    assert int(lab.min()) >= 0 and int(lab.max()) < N_CLASSES
    masks = torch.stack([(lab == k + 1) for k in range(N_CLASSES - 1)], 1).to(torch.uint8)
    batch = (images.to(device), masks.to(device), torch.ones(N, N_CLASSES - 1).to(device))
    if cfg["boundary"]:
        from capstone_amd.data import utils as DU
        batch += (DU.compute_distance_map(batch[1], spatial_dims=3),)
    return batch


# ---- the registry, walked ---------------------------------------------------------------------------------------------------------
def _span(t):
    """[lo, hi) in bytes of the memory a tensor (view) touches"""
    n = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


SKIP_ATTRS = {"plan", "engine", "buffers", "mod", "norm", "net", "reducer",
              "_w"}       # (_w: the closed forms' per-step torch temporaries, (B, C) tables no kernel holds a pointer to across steps)


def _reachable(obj, out, seen, path):
    """every tensor reachable from ``obj`` through tuples, lists, dicts, Acts and the objects of capstone_amd -> out[(path)] = tensor"""
    if obj is None or id(obj) in seen:
        return
    if isinstance(obj, torch.Tensor):
        if obj.numel() and obj.device.type != "meta":
            out.append((path, obj))
        return
    seen.add(id(obj))
    if isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _reachable(v, out, seen, f"{path}[{i}]")
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _reachable(v, out, seen, f"{path}[{k!r}]")
    elif isinstance(obj, Act):
        _reachable(obj.t, out, seen, path + ".t")
        _reachable(obj.pending_norm, out, seen, path + ".pending_norm")
        _reachable(obj.bst, out, seen, path + ".bst")
    elif isinstance(obj, torch.nn.Module) or isinstance(obj, (E.ParamStore, E.BufferStore)):
        return            # (parameters and module buffers: views of the stores' flat buffers, checked through the stores' own entries)
    elif type(obj).__module__.startswith("capstone_amd.") and hasattr(obj, "__dict__"):      # (not the ctypes descriptors)
        for k, v in vars(obj).items():
            if k not in SKIP_ATTRS:
                _reachable(v, out, seen, f"{path}.{k}")


def _owners(plan):
    """(name, object) of everything whose tensors must be registered: the plan (``_keep``, its tree of layer and norm objects, its
    packer), the stores it shares and its loss engines"""
    own = [("plan", plan), ("store", vars(plan.store)), ("bufs", vars(plan.engine.bufs) if plan.engine.bufs is not None else None)]
    for attr in ("_ctseg_loss", "_ctseg_loss_pair"):
        own.append((attr, getattr(plan, attr, None)))
    return own


def check_registry(plan):
    """completeness, disjointness and the partition of every allocation -> the entries"""
    entries = plan.all_buffers()
    assert entries
    bases = {}
    for e in entries:
        assert e.role in E.ROLES and (e.role == SCRATCH or e.reason), e
        bases.setdefault(e.base.data_ptr(), (e.base, []))[1].append(e)
    spans = sorted((_span(b) + (es[0].name,)) for b, es in bases.values())
    for (lo0, hi0, n0), (lo1, hi1, n1) in zip(spans[:-1], spans[1:]):
        assert hi0 <= lo1, f"registered buffers overlap: {n0} [{lo0:#x}, {hi0:#x}) and {n1} [{lo1:#x}, {hi1:#x})"
    for base, es in bases.values():      # the entries of one allocation: disjoint, and together all of it
        idx = torch.arange(base.numel()).view(base.shape)
        hit = torch.zeros(base.numel(), dtype=torch.int32)
        for e in es:
            assert e.base.shape == base.shape and e.base.dtype == base.dtype, (e, "two allocations at one address")
            hit[(idx if e.sel is None else idx[e.sel]).reshape(-1)] += 1
        assert bool((hit == 1).all()), f"{[e.name for e in es]}: entries do not partition the allocation " \
                                       f"({int((hit == 0).sum())} elements unregistered, {int((hit > 1).sum())} registered twice)"
    found = []
    for name, obj in _owners(plan):
        _reachable(obj, found, set(), name)
    assert len(found) > 20
    missing = []
    for path, t in found:
        lo, hi = _span(t)
        if not any(blo <= lo and hi <= bhi for blo, bhi, _ in spans):
            missing.append(f"{path} {tuple(t.shape)} {t.dtype}")
    assert not missing, "tensors of the step outside every registered buffer:\n  " + "\n  ".join(missing)
    return entries


def check_pads(plan, entries):
    acts = [e for e in entries if e.act is not None]
    assert acts
    for e in acts:
        C, ld, given = e.act
        assert e.base.shape[4] == ld and 0 < C <= ld, e
        dt = {torch.float32: nat.F32, torch.bfloat16: nat.BF16, torch.float16: nat.F16}[e.base.dtype]
        if not given:
            assert ld == default_ld(C, dt, plan.narrow_rows), (e, ld)
        else:               # the caller's stride: the chunked one, or the input's own channel count
            assert ld in (default_ld(C, dt, False), C), (e, ld)
        want = slice(C, ld) if e.name.endswith(" pad") else slice(0, C)
        assert e.sel == (Ellipsis, want), (e, e.sel)
        assert (ld > C) == any(o.base is e.base and o.name == e.name.replace(" pad", "") + " pad" for o in acts), e


# ---- CPU: the registry of every configuration's plans ------------------------------------------------------------------------------
@pytest.fixture()
def emu():
    with emulated(Emulator()) as e:
        yield e


def _cpu_plan(cfg, inference):
    m = _module(cfg, "cpu")
    sp = SP3 if cfg["kind"] == "3d" else SP2
    eng = m.unet.engine()
    plan = eng.plan_for_shape("cpu", cfg["N"], sp, inference=inference)
    if not inference:        # the loss engine, attached as the trainers (3-D) / the loss wrappers (2-D) attach it
        S = plan.logits.S
        if cfg["kind"] == "mixup":
            le = plan._ctseg_loss_pair = segloss.SegLossPairEngine(torch.device("cpu"), cfg["N"], S, N_CLASSES)
            lab = _labels(cfg["N"], sp, 1, False).reshape(cfg["N"], S)
            le.set_labels_from_i64(lab)
            le.set_pair(le.labels, le.hist, torch.tensor([1, 2, 0]))
        else:
            le = plan._ctseg_loss = segloss.SegLossEngine(torch.device("cpu"), cfg["N"], S, N_CLASSES)
            le.set_labels_from_i64(_labels(cfg["N"], sp, 1, False).reshape(cfg["N"], S))
        if cfg["boundary"]:
            le.set_dist_maps(torch.rand(cfg["N"], N_CLASSES - 1, *sp))
    return plan


@pytest.mark.parametrize("name", IDS)
def test_registry_is_complete_and_pads_are_the_layout_s(emu, monkeypatch, name):
    cfg = CONFIGS[name]
    _set_env(monkeypatch, cfg)
    kinds = [True] if cfg["inference"] else ([False, True] if name in ("3d-bf16", "3d-bf16-batchnorm") else [False])
    for inference in kinds:
        plan = _cpu_plan(cfg, inference)
        entries = check_registry(plan)
        check_pads(plan, entries)
        roles = {e.role for e in entries}
        assert SCRATCH in roles and STATE in roles and ZERO_RESTORED in roles


@pytest.mark.parametrize("name", [n for n in IDS if CONFIGS[n]["narrow"]])
def test_registry_and_pads_of_a_plan_with_12_wide_rows(monkeypatch, name):
    """the emulator declines 12-wide rows: these plans are recorded with the library's own host-only queries (recording runs no
    kernel), as tools/dump_plan.py records"""
    cfg = CONFIGS[name]
    _set_env(monkeypatch, cfg)
    monkeypatch.delenv("CTSEG_NARROW_ROWS", raising=False)
    monkeypatch.setattr(nat, "require_gpu", lambda t, what: None)
    plan = _cpu_plan(cfg, False)
    entries = check_registry(plan)
    check_pads(plan, entries)
    _assert_narrow(plan, entries)


def _assert_narrow(plan, entries):
    """12-wide rows occurred: the plan says so, and d loss / d logits and the head's 10-channel activations are 12 wide"""
    assert plan.narrow_rows and plan.dlogits.ld == 12
    wide = sorted({e.name for e in entries if e.act is not None and e.act[:2] == (N_CLASSES, 12) and e.base.dtype == torch.bfloat16})
    assert "plan/gradient of the logits" in wide and len(wide) >= 6, wide      # (each with its " pad" entry: columns 10..11)
    assert not any(e.act is not None and e.act[0] == N_CLASSES and e.act[1] == 16 and not e.act[2] for e in entries)


def test_an_unregistered_buffer_is_found(emu, monkeypatch):
    """the completeness check bites: a buffer allocated beside the helper, or an entry taken out of the registry, is named"""
    plan = _cpu_plan(CONFIGS["3d-bf16"], False)
    check_registry(plan)
    plan._keep.append((torch.zeros(4),))
    with pytest.raises(AssertionError, match="outside every registered buffer"):
        check_registry(plan)
    plan._keep.pop()
    gone = next(e for e in plan.buffers if e.name.endswith("/wgrad slabs"))
    plan.buffers.remove(gone)
    with pytest.raises(AssertionError, match="outside every registered buffer"):
        check_registry(plan)


def test_one_layer_plans_keep_no_registry():
    """the op tests' duck-typed plan has no ``buffers``: the helpers allocate the same tensors and record nothing"""
    class Bare:
        device, dt = torch.device("cpu"), nat.BF16
    t = E.plan_buf(Bare(), "x", (3, 2), torch.float32)
    a = E.plan_act(Bare(), (1, 2, 2, 2), 10)
    assert t.shape == (3, 2) and not bool(t.any()) and a.ld == 16 and not bool(a.t.any()) and not hasattr(Bare, "buffers")


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
V_PAD = 7.0                            # what the never-written ranges are filled with for the "other side" run (exact in every storage type)
POISONS = (("nan", float("nan")), ("finite", ACT_SENTINEL))


class Stepper:
    """One module of a configuration on the GPU: runs the step on a batch, reads the results back, restores weights / optimizer /
    running-statistics state."""

    def __init__(self, cfg, monkeypatch):
        from capstone_amd.training import mixup_trainer as MT
        from capstone_amd.training.utils import weighted_mixup
        self.cfg = cfg
        if cfg["kind"] == "mixup":
            index = torch.tensor([1, 2, 0][:cfg["N"]]).to(DEV)
            monkeypatch.setattr(MT, "weighted_mixup", functools.partial(weighted_mixup, index=index, lambda_=0.3))
        self.m = _module(cfg, DEV)
        self.eng = self.m.unet.engine()
        self.st = self.eng.ensure(torch.device(DEV))
        self.opt = None if cfg["kind"] == "3d" else self.m.configure_optimizers()["optimizer"]
        torch.cuda.synchronize()
        self.saved = self._state()
        self.plan = None

    def _state(self):
        st, bufs = self.st, self.eng.bufs
        return dict(p=st.flat_p.clone(), step=st.step, m=None if st.adam_m is None else st.adam_m.clone(),
                    v=None if st.adam_v is None else st.adam_v.clone(),
                    bn=None if bufs is None else (bufs.flat.clone(), bufs.nbt.clone()))

    def restore(self):
        """the weights, Adam state and running statistics the module was built with"""
        torch.cuda.synchronize()
        st, s = self.st, self.saved
        st.flat_p.copy_(s["p"])
        st.step = s["step"]
        if st.adam_m is not None:
            st.adam_m.zero_() if s["m"] is None else st.adam_m.copy_(s["m"])
            st.adam_v.zero_() if s["v"] is None else st.adam_v.copy_(s["v"])
        if s["bn"] is not None:
            self.eng.bufs.flat.copy_(s["bn"][0])
            self.eng.bufs.nbt.copy_(s["bn"][1])
        st.touch()                 # the packed operands are rebuilt by the next forward
        torch.cuda.synchronize()

    def step(self, batch):
        """one whole step -> dict of results, read back after a synchronize"""
        cfg, m, out = self.cfg, self.m, {}
        if cfg["inference"]:
            with torch.no_grad():
                y = m(batch[0])
            torch.cuda.synchronize()
            self.plan = self.eng.last_plan
            return {"logits": y.clone()}
        if cfg["kind"] == "3d":
            loss = m.fit_step(batch, keep_logits=cfg["keep_logits"])
            torch.cuda.synchronize()
            self.plan = plan = self.eng.last_plan
            le = plan._ctseg_loss
        else:
            self.opt.zero_grad()
            loss = m.training_step(batch)
            loss.backward()
            torch.cuda.synchronize()
            self.plan = plan = self.eng.last_plan
            le = plan._ctseg_loss_pair if cfg["kind"] == "mixup" else plan._ctseg_loss
            out["grad after backward"] = self.st.flat_g[:self.st.n].clone()
            self.opt.step()
            torch.cuda.synchronize()
        out["loss"] = loss.detach().clone()
        for k, v in m.logged.items():
            if "Dice" in k or "Loss" in k:
                out["logged " + k] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
        if plan.logits_current:
            out["logits"] = plan.logits.valid().clone()
        out["dlogits"] = plan.dlogits.valid().clone()
        out["dice counts"] = (le.cnt2 if cfg["kind"] == "mixup" else le.cnt).clone()
        st = self.st
        out["grad"] = st.flat_g[:st.n].clone()
        out["params"], out["adam m"], out["adam v"] = st.flat_p.clone(), st.adam_m.clone(), st.adam_v.clone()
        if self.eng.bufs is not None:
            out["running statistics"], out["num_batches_tracked"] = self.eng.bufs.flat.clone(), self.eng.bufs.nbt.clone()
        return out

    def entries(self):
        return self.plan.all_buffers()


def _same(a, b):
    """names of the results that differ bit for bit (NaN equal to NaN of the same bits: the results are compared as bytes)"""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = []
    for k in a:
        x, y = a[k].contiguous().reshape(-1), b[k].contiguous().reshape(-1)
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(f"{k} (shape or type)")
        elif not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            d = (x.double() - y.double()).abs()
            bad.append(f"{k} ({int((x != y).sum())} of {x.numel()} differ, {int(torch.isnan(y.double()).sum())} NaN, "
                       f"largest difference {float(d[~torch.isnan(d)].max()) if bool((~torch.isnan(d)).any()) else float('nan'):.3g})")
        else:
            assert not x.dtype.is_floating_point or bool(torch.isfinite(x.float()).all()), (k, "a result is not finite")
    return bad


def _fill(view, value):
    """poison as data: NaN / a finite value into float buffers, 0xA5 bytes into integer ones"""
    if view.dtype.is_floating_point:
        view.fill_(value)
    else:
        size = view.element_size()
        view.fill_(int.from_bytes(b"\xa5" * size, "little", signed=view.dtype != torch.uint8))


def _poison(entries, value, unwritten, only=None):
    for e in entries:
        if only is not None and e.name != only:
            continue
        if e.role == SCRATCH:
            _fill(e.view, value)
        elif e.role == ZERO_UNWRITTEN:
            v = e.view
            v.copy_(torch.where(unwritten[e.name], torch.zeros_like(v), torch.full_like(v, value)))


def _invariants(entries, unwritten):
    """after a step: zero-on-entry buffers are zero again, never-written ranges hold the zeros they held"""
    broken = []
    for e in entries:
        if e.role in (ZERO_RESTORED, ZERO_PAD) and bool(e.view.view(torch.uint8).any() if e.view.is_contiguous() else (e.view != 0).any()):
            broken.append(f"{e.name} ({e.role}) is not zero after the step")
        if e.role == ZERO_UNWRITTEN and bool((e.view[unwritten[e.name]] != 0).any()):
            broken.append(f"{e.name} ({e.role}): an element the step does not write is not zero")
    return broken


def _other_side(s, batch, entries):
    """fill the never-written ranges with V_PAD, run the step (its results may change: the role says the zeros are relied upon) and
    demand them back bit-unchanged; -> the unwritten elements of every zero-where-unwritten buffer.  Zeros are put back."""
    s.restore()
    for e in entries:
        if e.role in (ZERO_PAD, ZERO_UNWRITTEN):
            e.view.fill_(V_PAD)
    s.step(batch)
    unwritten, bad = {}, []
    for e in entries:
        if e.role == ZERO_PAD and not bool((e.view == V_PAD).all()):
            bad.append(e.name)
        if e.role == ZERO_UNWRITTEN:
            unwritten[e.name] = (e.view == V_PAD)
        if e.role in (ZERO_PAD, ZERO_UNWRITTEN):
            e.view.zero_()
    assert not bad, f"declared zero, never written, but written by the step: {bad}"
    return unwritten


def _blame(s, batch, ref, entries, unwritten):
    """(c): the step once per scratch buffer and poison value with only that buffer poisoned"""
    lines = []
    names = list(dict.fromkeys(e.name for e in entries if e.role in (SCRATCH, ZERO_UNWRITTEN)))
    for name in names:
        for tag, value in POISONS:
            s.restore()
            for e in entries:                    # the state of a fresh plan: what an earlier run left behind is not this buffer's doing
                if e.role != STATE:
                    e.view.zero_()
            _poison(entries, value, unwritten, only=name)
            bad = _same(ref, s.step(batch)) + _invariants(s.entries(), unwritten)
            if bad:
                lines.append(f"{name} [{tag}] -> {bad}")
                for e in s.entries():            # leave nothing of a broken invariant to the next buffer's run
                    if e.role in (ZERO_RESTORED, ZERO_PAD):
                        e.view.zero_()
    return lines


@gpu
@pytest.mark.parametrize("name", IDS)
def test_poisoned_workspace(monkeypatch, name):
    cfg = CONFIGS[name]
    _set_env(monkeypatch, cfg)
    s = Stepper(cfg, monkeypatch)
    batch = _batch(cfg, "A", DEV)
    ref = s.step(batch)
    entries = check_registry(s.plan)             # (after a step: the tensors the caller handed the loss engine included)
    check_pads(s.plan, entries)
    if cfg["narrow"]:
        _assert_narrow(s.plan, entries)
    elif not cfg["inference"] and cfg["precision"] == "bf16":
        # 8 channels on the first level, or a 2-D plan (depth 1: its head does not take the LDS-halo kernel): 16-wide rows
        assert not s.plan.narrow_rows and s.plan.dlogits.ld == 16
    if not cfg["keep_logits"]:
        assert s.plan.head_ce_slots(N_CLASSES) > 0 and "logits" not in ref, "the fused head did not run"
    s.restore()
    again = s.step(batch)
    assert not _same(ref, again), f"precondition: two plain runs of the step differ in {_same(ref, again)}"
    assert not _invariants(entries, {e.name: torch.zeros_like(e.view, dtype=torch.bool) for e in entries if e.role == ZERO_UNWRITTEN})
    unwritten = _other_side(s, batch, entries)
    if not cfg["inference"]:
        # the pad of d loss / d logits, derived here and not from the run: the loss passes store zeros in every pad column, the fused
        # head stores columns 0..11 of a row
        pad = unwritten.get("plan/gradient of the logits pad")
        ld = s.plan.dlogits.ld
        assert (pad is not None) == (ld > N_CLASSES)
        if pad is not None:
            want = torch.zeros_like(pad)
            if not cfg["keep_logits"]:
                want[..., 12 - N_CLASSES:] = True
            assert torch.equal(pad, want), f"unwritten pad columns of d loss / d logits (ld {ld}): {pad.flatten(0, 3).any(0).tolist()}"
    for tag, value in POISONS:
        s.restore()
        _poison(entries, value, unwritten)
        got = s.step(batch)
        assert s.entries()[0] is entries[0] and len(s.plan.buffers) == len([e for e in entries if e in s.plan.buffers])
        bad = _same(ref, got) + _invariants(entries, unwritten)
        if bad:
            lines = _blame(s, batch, ref, entries, unwritten)
            raise AssertionError(f"{name}: workspace poisoned with {tag}: {bad}\nbuffers whose content reaches a result or breaks an "
                                 "invariant:\n  " + "\n  ".join(lines or ["(none alone: a combination)"]))


@gpu
@pytest.mark.parametrize("name", IDS)
def test_used_plan_equals_fresh_plan(monkeypatch, name):
    cfg = CONFIGS[name]
    _set_env(monkeypatch, cfg)
    A, B = _batch(cfg, "A", DEV), _batch(cfg, "B", DEV)
    lab = B[1].flatten(2).any(2)                 # (N, 9): which structures a sample of B holds
    assert not bool(lab[1].any()) and not bool(lab[0, 4]) and bool(lab[0].any())
    used = Stepper(cfg, monkeypatch)
    a1 = used.step(A)
    used.restore()
    assert not _same(a1, used.step(A)), "precondition: two plain runs of the step differ"
    used.restore()
    b_used = used.step(B)
    fresh = Stepper(cfg, monkeypatch)
    assert torch.equal(fresh.saved["p"], used.saved["p"])
    b_fresh = fresh.step(B)
    assert not _same(b_fresh, b_used), f"step on B after a step on A differs from a fresh plan's in {_same(b_fresh, b_used)}"
    # three steps with the updates (and the repack, the running statistics) carried across them
    used.restore()
    fresh2 = Stepper(cfg, monkeypatch)
    for i, batch in enumerate((A, B, A)):
        u, f = used.step(batch), fresh2.step(batch)
        assert not _same(f, u), f"step {i} of A, B, A on a used plan differs from a fresh plan's in {_same(f, u)}"
