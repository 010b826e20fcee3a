"""CPU: UNet(norm="BATCH") — module tree, state_dict keys, refusals, and the host logic of the BatchNorm plans (recording, mode keys,
running-statistics buffers, which fusions a BatchNorm layer declines) run through the numpy ABI emulator extended by the six
BatchNorm entry points, against MONAI's network (the oracle with every Convolution's norm swapped for nn.BatchNorm{2,3}d)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from abi_emulator import Emulator, emulated
from capstone_amd import _native as nat
from capstone_amd.models import UNet
from feature_emulators import BatchNormEntries
from helpers import swapped_oracle

class E(BatchNormEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E()) as e:
        yield e


def _pair(dims, cin, cout, chans, strides, nres, seed=0):
    """swapped oracle + product network with the same, non-trivial state (gamma, beta, running statistics, PReLU slopes)"""
    torch.manual_seed(seed)
    ref = swapped_oracle(dims, cin, cout, chans, strides, nres)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            if isinstance(m, nn.PReLU):
                m.weight.fill_(0.05 + 0.3 * float(torch.rand(1, generator=g)))
    net = UNet(dims, cin, cout, chans, strides, num_res_units=nres, norm="BATCH")
    net.load_state_dict(ref.state_dict())
    return ref, net


def _bn_state(mod):
    return {k: v.detach().cpu().clone() for k, v in mod.state_dict().items() if "running" in k or "num_batches" in k}


# ---- module surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["BATCH", "batch", "Batch"])
def test_batch_norm_tree_keys_and_seeded_conv_weights(norm):
    args = (3, 1, 2, (16, 32, 64, 128, 256), (2, 2, 2, 2))
    torch.manual_seed(3)
    net = UNet(*args, num_res_units=2, norm=norm)
    torch.manual_seed(3)
    inst = UNet(*args, num_res_units=2)
    torch.manual_seed(3)
    ref = swapped_oracle(*args, 2)
    assert list(net.state_dict()) == list(ref.state_dict())
    assert isinstance(net.model[0].conv.unit0.norm, nn.BatchNorm3d)
    for k in ("model.0.conv.unit0.norm.weight", "model.0.conv.unit0.norm.bias", "model.0.conv.unit0.norm.running_mean",
              "model.0.conv.unit0.norm.running_var", "model.0.conv.unit0.norm.num_batches_tracked"):
        assert k in net.state_dict(), k
    # BatchNorm draws no random numbers: the convolutions equal the INSTANCE model's under the same seed (and MONAI's)
    si, sb, so = inst.state_dict(), net.state_dict(), ref.state_dict()
    for k, v in si.items():
        assert torch.equal(v, sb[k]), k
    for k, v in sb.items():
        assert torch.equal(v, so[k]), k
    with pytest.raises(nat.NativeError):
        net.model[0].conv.unit0.norm(torch.zeros(2, 16, 4, 4, 4))     # a parameter container, like the rest of the tree


def test_batch_norm_2d_tree_and_instance_unchanged():
    net = UNet(2, 1, 10, (4, 8, 16), (2, 2), num_res_units=2, norm="BATCH")
    ref = swapped_oracle(2, 1, 10, (4, 8, 16), (2, 2), 2)
    assert list(net.state_dict()) == list(ref.state_dict())
    assert isinstance(net.model[2][0].norm, nn.BatchNorm2d)
    inst = UNet(2, 1, 10, (4, 8, 16), (2, 2), num_res_units=2, norm="instance")
    assert isinstance(inst.model[2][0].norm, nn.InstanceNorm2d)
    for bad in ("GROUP", "LAYER", "batchnorm"):
        with pytest.raises(NotImplementedError):
            UNet(3, 1, 2, (4, 8), (2,), norm=bad)


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["momentum", "affine", "track"])
def test_unsupported_batch_norm_settings_are_refused_when_recording(what):
    net = UNet(3, 1, 2, (4, 8), (2,), num_res_units=2, norm="BATCH")
    m = net.model[1].submodule.conv.unit1
    if what == "momentum":
        m.norm.momentum = None
    elif what == "affine":
        m.norm = nn.BatchNorm3d(8, affine=False)
    else:
        m.norm = nn.BatchNorm3d(8, track_running_stats=False)
    with pytest.raises(NotImplementedError):
        net.engine().plan_for_shape("cpu", 1, (8, 8, 8))


def test_gradient_forward_in_eval_mode_is_refused(emu):
    ref, net = _pair(3, 1, 2, (4, 8), (2,), 2)
    net.eval()
    with pytest.raises(NotImplementedError):
        net(torch.randn(1, 1, 8, 8, 8))                   # backward through frozen statistics
    with torch.no_grad():
        net(torch.randn(1, 1, 8, 8, 8))                   # inference is fine


def test_data_parallel_attach_is_refused(monkeypatch):
    import torch.distributed as dist
    from capstone_amd import distributed as cdist

    class Holder(nn.Module):
        def __init__(self, unet):
            super().__init__()
            self.unet = unet

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        cdist.attach(Holder(UNet(3, 1, 2, (4, 8), (2,), norm="BATCH")))


def test_sliding_window_refuses_training_mode():
    from capstone_amd.inferers import sliding_window_inference
    net = UNet(3, 1, 2, (4, 8), (2,), num_res_units=2, norm="BATCH")
    with pytest.raises(ValueError, match="eval"):
        sliding_window_inference(torch.zeros(1, 1, 16, 16, 16), (8, 8, 8), 1, net.train())


# ---- host logic on the emulator -------------------------------------------------------------------------------------------
CASES = [
    (3, 1, 10, (4, 8, 16, 32), (2, 2, 2), 2, (2, 1, 16, 16, 8)),
    (3, 2, 3, (4, 8, 12), (2, 2), 0, (2, 2, 8, 8, 4)),
    (3, 1, 10, (8, 4, 8), (2, 2), 1, (2, 1, 8, 8, 8)),
    (2, 1, 10, (4, 8, 16), (2, 2), 2, (2, 1, 16, 12)),
]


@pytest.mark.parametrize("case", CASES)
def test_training_step_matches_monai_batch_norm(emu, case):
    dims, cin, cout, chans, strides, nres, shape = case
    ref, net = _pair(dims, cin, cout, chans, strides, nres)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    y_ref = ref(x)
    eng = net.engine()
    eng.forward(x)
    y = eng.logits_view().clone()
    np.testing.assert_allclose(y.numpy(), y_ref.detach().numpy(), rtol=2e-4, atol=3e-5)
    for k, v in _bn_state(ref).items():
        np.testing.assert_allclose(net.state_dict()[k].numpy(), v.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy)
    pl = eng.last_plan
    pl.dlogits.t[..., :cout].copy_((gy if dims == 3 else gy.unsqueeze(-1)).permute(0, 2, 3, 4, 1))
    eng.backward()
    for (k, p), q in zip(ref.named_parameters(), net.parameters()):
        got, want = eng.store.grad_view(q).numpy(), p.grad.numpy()
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=3e-3, atol=(5e-3 if k.endswith(".bias") else 5e-5) * scale, err_msg=k)
    # no InstanceNorm fusion reached a BatchNorm layer
    for name, _, args in pl.fwd + pl.bwd:
        assert not name.startswith("ctseg_instnorm_prelu_bwd") and name != "ctseg_instnorm_finalize", name
        for a in args:
            if isinstance(a, nat.ConvDesc):
                assert not a.in_mean_rstd and not a.bst_partials and not a.bst_y, name
            if isinstance(a, nat.WgradDesc):
                assert not a.in_mean_rstd and not a.dyn_g and not a.dyn_sums, name
    assert pl.norm_bwd == []


def test_modes_keys_and_running_statistics_round_trip(emu):
    ref, net = _pair(3, 1, 10, (4, 8, 16), (2, 2), 2)
    eng = net.engine()
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, 1, 8, 8, 8, generator=g) for _ in range(4)]
    with torch.no_grad():
        # eval first: running statistics are read, never written
        net.eval(), ref.eval()
        before = _bn_state(net)
        np.testing.assert_allclose(net(xs[0]).numpy(), ref(xs[0]).numpy(), rtol=2e-4, atol=3e-5)
        for k, v in _bn_state(net).items():
            assert torch.equal(v, before[k]), k
        # train() under no_grad: batch statistics, running statistics updated exactly as torch does
        net.train(), ref.train()
        np.testing.assert_allclose(net(xs[1]).numpy(), ref(xs[1]).numpy(), rtol=2e-4, atol=3e-5)
        net.eval(), ref.eval()
        np.testing.assert_allclose(net(xs[2]).numpy(), ref(xs[2]).numpy(), rtol=2e-4, atol=3e-5)
        net.train(), ref.train()
        np.testing.assert_allclose(net(xs[3]).numpy(), ref(xs[3]).numpy(), rtol=2e-4, atol=3e-5)
    for k, v in _bn_state(ref).items():
        np.testing.assert_allclose(net.state_dict()[k].numpy(), v.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    assert int(net.state_dict()["model.0.conv.unit0.norm.num_batches_tracked"]) == 2
    assert sorted(k for k in eng.plans) == [(2, 8, 8, 8, "bn-eval", "inference"), (2, 8, 8, 8, "bn-train", "inference")]
    # load_state_dict writes into the engine's buffers; a replaced buffer (`.data = ...`) is copied back in before the next forward
    sd = ref.state_dict()
    sd["model.0.conv.unit0.norm.running_mean"] = torch.full_like(sd["model.0.conv.unit0.norm.running_mean"], 0.25)
    ref.load_state_dict(sd)
    net.load_state_dict(sd)
    net.model[1].submodule[0].conv.unit1.norm.running_var = torch.full((8,), 2.0)
    ref.model[1].submodule[0].conv.unit1.norm.running_var = torch.full((8,), 2.0)
    net.eval(), ref.eval()
    with torch.no_grad():
        np.testing.assert_allclose(net(xs[0]).numpy(), ref(xs[0]).numpy(), rtol=2e-4, atol=3e-5)
    assert eng.bufs.attached()


def test_instance_networks_keep_their_plan_keys(emu):
    torch.manual_seed(0)
    net = UNet(3, 1, 10, (4, 8), (2,), num_res_units=2)
    eng = net.engine()
    eng.forward(torch.randn(1, 1, 8, 8, 8))
    assert list(eng.plans) == [(1, 8, 8, 8)] and eng.bufs is None
