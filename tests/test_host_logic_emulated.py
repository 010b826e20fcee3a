"""CPU: the product's HOST logic (plan recording, tap tables, packed-weight indices, channel slices,
backward graph, gradient placement, Adam, loss tables) executed through the numpy emulator of the C ABI
(tests/abi_emulator.py) and compared with the oracle.  No HIP kernel runs here; -m gpu tests cover those."""
import numpy as np
import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd.models import UNet
from oracle.monai_unet import UNet as OracleUNet
from oracle import losses as OL
from oracle import metrics as OM


@pytest.fixture()
def emu():
    with emulated(Emulator()) as e:
        yield e


def _tol(key, ref):
    """conv biases that feed an InstanceNorm have an analytically ZERO gradient: both sides hold only
    rounding noise there (~1e-4), so biases get an absolute floor; everything else is relative."""
    scale = max(1.0, float(np.abs(ref).max()))
    return dict(rtol=3e-3, atol=(5e-3 if key.endswith(".bias") else 5e-5) * scale)


def _pair(dims, cin, cout, channels, strides, nres, seed=0):
    torch.manual_seed(seed)
    ref = OracleUNet(dims, cin, cout, channels, strides, num_res_units=nres)
    net = UNet(dims, cin, cout, channels, strides, num_res_units=nres)
    net.load_state_dict(ref.state_dict())
    with torch.no_grad():  # make PReLU slopes distinct so a mixed-up alpha shows
        for i, (p, q) in enumerate(zip(ref.parameters(), net.parameters())):
            if p.numel() == 1:
                p.fill_(0.1 + 0.03 * i)
                q.fill_(0.1 + 0.03 * i)
    return ref, net


CASES = [
    (3, 1, 10, (4, 8, 16, 32), (2, 2, 2, 2), 2, (2, 1, 16, 16, 8)),
    (3, 1, 10, (4, 8), (2,), 2, (1, 1, 8, 4, 6)),
    (3, 2, 3, (4, 8, 12), (2, 2), 0, (1, 2, 8, 8, 4)),
    (3, 1, 10, (8, 4, 8), (2, 2), 1, (1, 1, 8, 8, 8)),
    (2, 1, 10, (4, 8, 16), (2, 2), 2, (2, 1, 16, 12)),
    (2, 3, 5, (4, 8, 16), (2, 2), 0, (1, 3, 8, 8)),
]


@pytest.mark.parametrize("case", CASES)
def test_forward_backward_match_oracle(emu, case):
    dims, cin, cout, chans, strides, nres, shape = case
    ref, net = _pair(dims, cin, cout, chans, strides, nres)
    assert list(ref.state_dict()) == list(net.state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    y_ref = ref(x)
    eng = net.engine()
    eng.forward(x)
    y = eng.logits_view().clone()
    assert y.shape == y_ref.shape
    np.testing.assert_allclose(y.numpy(), y_ref.detach().numpy(), rtol=2e-4, atol=2e-5)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy)
    pl = eng.last_plan
    gv = gy if dims == 3 else gy.unsqueeze(-1)
    pl.dlogits.t[..., :cout].copy_(gv.permute(0, 2, 3, 4, 1))
    eng.backward()
    for (k, p), q in zip(ref.named_parameters(), net.parameters()):
        got = eng.store.grad_view(q).numpy()
        np.testing.assert_allclose(got, p.grad.numpy(), err_msg=k, **_tol(k, p.grad.numpy()))


def test_autograd_surface_and_losses(emu):
    """UNet.forward -> MultipleLossWrapper -> .backward() through the autograd Functions, all five losses."""
    from capstone_amd.models.losses import MultipleLossWrapper
    ref, net = _pair(3, 1, 10, (4, 8, 16), (2, 2), 2)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 8, 8, 8, generator=g)
    target = torch.randint(0, 10, (2, 8, 8, 8), generator=g)
    target[0][target[0] == 4] = 0
    names = ["CrossEntropy", "Dice", "Focal", "GeneralizedDice", "WeightedCrossEntropy"]
    ind = torch.ones(2, 9)
    y_ref = ref(x)
    ref_vals = OL.MultipleLoss(names)(y_ref, target, ind)
    torch.stack(list(ref_vals.values())).sum().backward()
    y = net(x)
    y._ctseg_plan = net.engine().last_plan
    vals = MultipleLossWrapper(names)(input=y, target=target, mask_indicator=ind)
    for n in names:
        np.testing.assert_allclose(vals[n].detach().numpy(), ref_vals[n].detach().numpy(), rtol=2e-4, atol=1e-6, err_msg=n)
    torch.stack(list(vals.values())).sum().backward()
    for (k, p), q in zip(ref.named_parameters(), net.parameters()):
        np.testing.assert_allclose(q.grad.numpy(), p.grad.numpy(), err_msg=k, **_tol(k, p.grad.numpy()))


def test_exclude_missing_tables(emu):
    from capstone_amd.models.losses import MultipleLossWrapper
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(3, 10, 4, 4, 4, generator=g)
    target = torch.randint(0, 10, (3, 4, 4, 4), generator=g)
    ind = (torch.rand(3, 9, generator=g) < 0.7).float()
    ind[0] = 1
    names = ["Dice", "Focal", "GeneralizedDice"]
    x_ref = logits.clone().requires_grad_(True)
    rv = OL.MultipleLoss(names, exclude_missing=True)(x_ref, target, ind)
    torch.stack(list(rv.values())).sum().backward()
    x = logits.clone().requires_grad_(True)
    v = MultipleLossWrapper(names, exclude_missing=True)(input=x, target=target, mask_indicator=ind)
    for n in names:
        np.testing.assert_allclose(v[n].detach().numpy(), rv[n].detach().numpy(), rtol=2e-4, atol=1e-6, err_msg=n)
    torch.stack(list(v.values())).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), x_ref.grad.numpy(), rtol=2e-3, atol=2e-6)


def test_tiny_step_fixture_fit_step(emu, golden):
    """BaseUNet3D.fit_step (native order: forward, fused CE, backward, Adam) reproduces the oracle fixture."""
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    g = golden("unet_tiny.npz")
    for tag in ("a", "b"):
        m = BaseUNet3D(filters=[int(v) for v in g[f"{tag}_filters"]], loss_fx=[str(s) for s in g[f"{tag}_losses"]])
        m.load_state_dict({k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}_w:")})
        batch = tuple(torch.from_numpy(g[f"{tag}_{n}"]) for n in ("images", "masks", "indicator"))
        loss = m.fit_step(batch)
        np.testing.assert_allclose(loss.numpy(), g[f"{tag}_loss"], rtol=2e-4)
        np.testing.assert_allclose(m.logged["Mean Dice Score (train)"].numpy(), g[f"{tag}_dice_mean"], atol=1e-6)
        np.testing.assert_allclose(m.logged["Dice per class (train)"].numpy(), g[f"{tag}_dice_per_class"], atol=1e-6)
        st = m.unet.engine().store
        for k, p in m.named_parameters():
            np.testing.assert_allclose(st.grad_view(p).numpy(), g[f"{tag}_g:{k}"], err_msg=k, **_tol(k, g[f"{tag}_g:{k}"]))
            # Adam's first step is -lr*sign(g): where the reference gradient is rounding noise the sign is arbitrary
            gref, w1 = g[f"{tag}_g:{k}"], g[f"{tag}_w1:{k}"]
            solid = np.abs(gref) > 1e-3 * max(np.abs(gref).max(), 1e-6)
            if k.endswith(".bias") and "residual" not in k:
                solid &= False
            got = p.detach().numpy()
            np.testing.assert_allclose(got[solid], w1[solid], rtol=1e-3, atol=2.5e-4, err_msg=k)
            np.testing.assert_allclose(got, w1, rtol=0, atol=2.1e-3, err_msg=k)


def test_drop_in_helpers(emu, golden):
    from capstone_amd.training.utils import _squash_predictions
    from capstone_amd.volumetric.utils import _squash_masks_3D
    from capstone_amd.volumetric.metrics import DiceMetricWrapper3D
    leaf = golden("ref_leaf.npz")
    got = _squash_masks_3D(torch.from_numpy(leaf["squash_masks_in"]), 10, "cpu")
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(got.numpy(), leaf["squash_masks_out"])
    np.testing.assert_array_equal(_squash_predictions(torch.from_numpy(leaf["squash_pred_in"])).numpy(), leaf["squash_pred_out"])
    m, pc = DiceMetricWrapper3D()(torch.from_numpy(leaf["dice_pred"]), torch.from_numpy(leaf["dice_target"]))
    np.testing.assert_array_equal(pc.numpy(), leaf["dice_per_class"])
    np.testing.assert_array_equal(m.numpy(), leaf["dice_mean"])


def test_optimizer_update_reaches_every_cached_plan(emu):
    """train on shape A, evaluate on shape B, train, evaluate: ctseg_adam_step rewrites the flat parameter buffer through raw
    pointers (no Parameter version changes), so plan B's packed operands must be rebuilt from the store's generation counter —
    its second forward has to equal the oracle's forward with the UPDATED weights."""
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    from oracle.trainer import OracleUNet3D
    torch.manual_seed(2)
    om = OracleUNet3D(filters=(4, 8, 16), loss_fx=("CrossEntropy",), lr=0.05)
    m = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"], lr=0.05)
    m.load_state_dict(om.state_dict())
    g = torch.Generator().manual_seed(4)
    xa, xb = torch.randn(1, 1, 8, 8, 8, generator=g), torch.randn(2, 1, 8, 4, 4, generator=g)
    masks = (torch.rand(1, 9, 8, 8, 8, generator=g) < 0.1).to(torch.uint8)
    batch = (xa, masks, torch.ones(1, 9))
    opt = om.configure_optimizers()
    eng = m.unet.engine()
    with torch.no_grad():
        yb0 = m(xb).clone()                      # plan B recorded and packed with the initial weights
    np.testing.assert_allclose(yb0.numpy(), om(xb).detach().numpy(), rtol=2e-3, atol=2e-4)
    for _ in range(2):
        m.fit_step(batch)                        # plan A: forward, backward, native Adam (lr large enough to show)
        om.fit_step(batch, opt)
    assert len(eng.plans) == 2
    with torch.no_grad():
        yb1 = m(xb).clone()
    ref = om(xb).detach()
    assert float((ref - yb0).abs().max()) > 0.05, "the update must be visible in plan B's output"
    np.testing.assert_allclose(yb1.numpy(), ref.numpy(), rtol=2e-3, atol=2e-3)
    # the re-attach path (someone replaced Parameter storage): every plan repacks as well
    with torch.no_grad():
        for p in m.unet.parameters():
            p.data = p.data.clone() * 0.5
        for p in om.unet.parameters():
            p.mul_(0.5)
        np.testing.assert_allclose(m(xb).numpy(), om(xb).numpy(), rtol=2e-3, atol=2e-3)


def test_native_optimizer_state_round_trips_through_torch_adam_layout(emu):
    """fit_step keeps Adam's moments in the flat store; optimizer_state_dict() exports them in torch.optim.Adam's own layout
    (what Lightning's ModelCheckpoint stores, volumetric/base_trainer.py:224-225): a resumed module continues bit-identically,
    and torch's Adam accepts the same dict."""
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 1, 8, 8, 8, generator=g)
    masks = (torch.rand(1, 9, 8, 8, 8, generator=g) < 0.1).to(torch.uint8)
    batch = (x, masks, torch.ones(1, 9))
    m1 = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"])
    for _ in range(2):
        m1.fit_step(batch)
    ck = m1.checkpoint()
    assert set(ck["state_dict"]) == set(m1.state_dict())            # weights keep the reference's keys only
    osd = ck["optimizer_states"][0]
    assert len(osd["state"]) == len(list(m1.parameters())) and float(osd["state"][0]["step"]) == 2.0
    m2 = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"])
    m2.load_checkpoint(ck)
    l1, l2 = m1.fit_step(batch), m2.fit_step(batch)
    assert float(l1) == float(l2)
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p.detach(), q.detach())
    opt = torch.optim.Adam(m2.parameters(), lr=m2.hparams.lr)
    opt.load_state_dict(m2.optimizer_state_dict())                   # torch's own Adam takes the layout
    st = m2.unet.engine().store
    p0 = next(iter(m2.parameters()))
    assert torch.equal(opt.state[p0]["exp_avg"].reshape(-1), st.adam_m[st.off(p0):st.off(p0) + p0.numel()])


@pytest.mark.parametrize("fused", ["1", "0"])
def test_drop_in_surface_training_step_backward_optimizer_step_equals_fit_step(emu, monkeypatch, fused):
    """The surface the reference's Lightning loop drives (capstone/volumetric/base_trainer.py:80-82,113-114): ``training_step`` ->
    ``loss.backward()`` -> ``configure_optimizers().step()`` -> ``zero_grad()``.  With a cross-entropy-only loss the step runs
    fused (plan._StepLossFn), ``p.grad`` is a view of the flat gradient buffer (no copies) and the optimizer is one ctseg_adam_step
    launch — and the weights after K steps are BIT-identical to K ``fit_step`` calls, for both zero_grad conventions, for an upstream
    gradient != 1, and with gradient accumulation (two backwards, one step) equal to the oracle."""
    from capstone_amd.optim import Adam
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    import oracle.trainer as OT
    monkeypatch.setenv("CTSEG_DROPIN_FUSED", fused)      # "0": the two-pass route through _shared_step (same results)
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 8, 8, 8, generator=g)
    masks = (torch.rand(2, 9, 8, 8, 8, generator=g) < 0.1).to(torch.uint8)
    batch = (x, masks, torch.ones(2, 9))
    ref = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"], lr=1e-2)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    ref_losses = [float(ref.fit_step(batch)) for _ in range(3)]
    for set_to_none in (True, False):
        m = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"], lr=1e-2)
        m.load_state_dict(sd)
        opt = m.configure_optimizers()
        assert isinstance(opt, torch.optim.Adam) and isinstance(opt, Adam) and opt.defaults["lr"] == 1e-2
        losses = []
        for _ in range(3):
            opt.zero_grad(set_to_none=set_to_none)
            loss = m.training_step(batch, 0)
            assert loss.requires_grad and loss.ndim == 0
            loss.backward()
            st = m.unet.engine().store
            p0 = st.params[0]
            assert p0.grad.data_ptr() == st.flat_g.data_ptr() + 4 * st.off(p0)        # a view, not a copy
            opt.step()
            losses.append(float(loss.detach()))
        assert losses == ref_losses, (set_to_none, losses, ref_losses)
        for p, q in zip(ref.parameters(), m.parameters()):
            assert torch.equal(p.detach(), q.detach())
        assert m.logged["CrossEntropy Loss (train)"].item() == losses[-1] and "BrainStem Dice (train)" in m.logged
        # the optimizer's state_dict is torch.optim.Adam's layout, the engine's moments included; it round-trips
        osd = opt.state_dict()
        assert len(osd["state"]) == len(list(m.parameters())) and float(osd["state"][0]["step"]) == 3.0
        plain = torch.optim.Adam(m.parameters(), lr=1e-2)
        plain.load_state_dict(osd)
        m2 = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"], lr=1e-2)
        m2.load_state_dict(m.state_dict())
        # plain torch's resume order: the optimizer state is loaded into a FRESH module, before any forward built the flat store
        # (the moments then stayed in torch's self.state and the first native step ran on zeroed moments, step 0)
        assert m2.unet.engine().store is None
        opt2 = m2.configure_optimizers()
        opt2.load_state_dict(osd)
        assert m2.unet.engine().store.step == 3 and not opt2.state
        a, b = float(ref.fit_step(batch)), None
        opt2.zero_grad()
        l2 = m2.training_step(batch, 0)
        l2.backward()
        opt2.step()
        assert float(l2.detach()) == a
        for p, q in zip(ref.parameters(), m2.parameters()):      # the 4th update used the checkpointed moments and step count
            assert torch.equal(p.detach(), q.detach())
        ref.load_state_dict(m.state_dict())        # rewind the reference model for the next convention
        ref.load_optimizer_state_dict(osd)
    # an upstream gradient != 1 and gradient accumulation, against the oracle (torch autograd + torch Adam)
    om = OT.OracleUNet3D(filters=(4, 8, 16), loss_fx=("CrossEntropy",), lr=1e-2)
    om.load_state_dict(sd)
    m = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"], lr=1e-2)
    m.load_state_dict(sd)
    opt, oopt = m.configure_optimizers(), om.configure_optimizers()
    opt.zero_grad()
    oopt.zero_grad()
    (0.25 * m.training_step(batch, 0)).backward()
    (0.25 * om.training_step(batch)).backward()
    x2 = torch.randn(2, 1, 8, 8, 8, generator=g)
    batch2 = (x2, masks, torch.ones(2, 9))
    (0.75 * m.training_step(batch2, 0)).backward()          # accumulates into the same p.grad
    (0.75 * om.training_step(batch2)).backward()
    for (k, p), q in zip(om.named_parameters(), m.parameters()):
        np.testing.assert_allclose(q.grad.numpy(), p.grad.numpy(), err_msg=k, **_tol(k, p.grad.numpy()))
    opt.step()
    oopt.step()
    if fused == "1":   # a second backward on the same step's graph is refused (its buffers were consumed)
        loss = m.training_step(batch, 0)
        loss.backward()
        with pytest.raises(RuntimeError):
            loss.backward()


def test_epoch_means_and_overwritten_activation_guard(emu):
    """log(on_epoch=True) accumulates the mean over the steps of an epoch (Lightning 1.0's reduction of what the reference logs,
    volumetric/base_trainer.py:106-109,125-131); a backward on activations a later forward overwrote raises."""
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(4)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 1, 8, 8, 8, generator=g)
    masks = (torch.rand(1, 9, 8, 8, 8, generator=g) < 0.1).to(torch.uint8)
    batch = (x, masks, torch.ones(1, 9))
    m = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"])
    losses, dices = [], []
    for _ in range(3):
        losses.append(float(m.fit_step(batch)))
        dices.append(float(m.logged["Mean Dice Score (train)"]))
    means = m.epoch_means()
    np.testing.assert_allclose(float(means["CrossEntropy Loss (train)"]), np.mean(losses), rtol=1e-6)
    np.testing.assert_allclose(float(means["Mean Dice Score (train)"]), np.mean(dices), rtol=1e-6, atol=1e-8)
    assert means["Dice per class (train)"].shape == (9,) and m.epoch_means() == {}
    vals = []
    for _ in range(2):
        vals.append(float(m.training_step(batch).detach()))
    np.testing.assert_allclose(float(m.epoch_means()["CrossEntropy Loss (train)"]), np.mean(vals), rtol=1e-6)
    l1 = m.training_step(batch)
    m.training_step(batch)                       # same shape: overwrites the activations l1's graph points at
    with pytest.raises(RuntimeError, match="overwritten"):
        l1.backward()


def test_2d_downsample_conv1x1_trains_through_the_input_gradient(emu):
    """--downsample (capstone/training/base_trainer.py:53,81-85): a trainable 3 -> 1 convolution in front of the 2-D U-Net.  The
    engine records an input-gradient pass for the stem; conv1x1's weight and bias gradients must equal the oracle's (nn.Conv2d(3,1,1)
    followed by the oracle U-Net)."""
    from capstone_amd.training.base_trainer import BaseUNet2D
    torch.manual_seed(11)
    filters = [4, 8, 12, 16, 24]
    ref = OracleUNet(2, 1, 10, filters, (2, 2, 2, 2), num_res_units=2)
    m = BaseUNet2D(filters=list(filters), use_res_units=True, downsample=True, loss_fx=["CrossEntropy"], transform_degree=1)
    m.unet.load_state_dict(ref.state_dict())
    c1 = torch.nn.Conv2d(3, 1, 1)
    c1.load_state_dict(m.conv1x1.state_dict())
    g = torch.Generator().manual_seed(12)
    images = torch.randn(2, 3, 32, 32, generator=g)
    masks = (torch.rand(2, 9, 32, 32, generator=g) < 0.1).to(torch.uint8)
    ind = torch.ones(2, 9)
    labels = OM.squash_masks(masks, 10)
    lref = OL.MultipleLoss(["CrossEntropy"])(ref(c1(images)), labels, ind)["CrossEntropy"]
    lref.backward()
    loss = m.training_step((images, masks, ind))
    loss.backward()
    np.testing.assert_allclose(loss.item(), lref.item(), rtol=2e-4)
    np.testing.assert_allclose(m.conv1x1.weight.grad.numpy(), c1.weight.grad.numpy(), rtol=5e-3, atol=1e-6)
    np.testing.assert_allclose(m.conv1x1.bias.grad.numpy(), c1.bias.grad.numpy(), rtol=5e-3, atol=1e-6)
    k, p = next(iter(ref.named_parameters()))
    np.testing.assert_allclose(dict(m.unet.named_parameters())[k].grad.numpy(), p.grad.numpy(), **_tol(k, p.grad.numpy()))


def test_identity_residual_bottom_under_a_dense_skip_gradient(emu):
    """equal channel counts at the bottom (ResidualUnit with an identity residual) under the accumulated skip gradient: the
    input gradient is g + dgrad(dy) PLUS the accumulated term (one extra elementwise pass)."""
    case = (3, 1, 10, (4, 8, 8), (2, 2), 2, (1, 1, 8, 8, 8))
    dims, cin, cout, chans, strides, nres, shape = case
    ref, net = _pair(dims, cin, cout, chans, strides, nres)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    y_ref = ref(x)
    eng = net.engine()
    eng.forward(x)
    np.testing.assert_allclose(eng.logits_view().numpy(), y_ref.detach().numpy(), rtol=2e-4, atol=2e-5)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy)
    pl = eng.last_plan
    pl.dlogits.t[..., :cout].copy_(gy.permute(0, 2, 3, 4, 1))
    eng.backward()
    for (k, p), q in zip(ref.named_parameters(), net.parameters()):
        np.testing.assert_allclose(eng.store.grad_view(q).numpy(), p.grad.numpy(), err_msg=k, **_tol(k, p.grad.numpy()))


@pytest.mark.parametrize("exclude_missing", [False, True])
def test_loss_module_dict_entries_match_the_oracle(emu, exclude_missing):
    """``MultipleLossWrapper.losses`` (reference capstone/models/losses.py:177-180): an nn.ModuleDict keyed by loss name whose
    entries are called as ``fx(input, target)`` — scalar, or the unreduced (B, C-1) / (B, C) table under ``reduction="none"`` — with
    a gradient w.r.t. the logits.  Host logic on the C-ABI emulator against the oracle's formulas."""
    from capstone_amd.volumetric.losses import MultipleLossWrapper3D
    names = ["CrossEntropy", "Dice", "Focal", "GeneralizedDice", "WeightedCrossEntropy"]
    w = MultipleLossWrapper3D(losses=names, exclude_missing=exclude_missing)
    assert isinstance(w.losses, torch.nn.ModuleDict) and list(w.losses.keys()) == names and list(w.state_dict()) == []
    assert all(fx.reduction == ("none" if exclude_missing else "mean") for fx in w.losses.values())
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(2, 10, 12, 10, 8, generator=g)
    target = torch.randint(0, 10, (2, 12, 10, 8), generator=g)
    for name, fx in w.losses.items():
        x, xr = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
        v = fx(x, target)
        if exclude_missing and name in ("Dice", "Focal", "GeneralizedDice"):
            ref = OL._TABLE[name](xr, target, "none")
            assert v.shape == ref.shape == ((2, 10) if name == "Focal" else (2, 9))
            np.testing.assert_allclose(v.detach().numpy(), ref.detach().numpy(), rtol=2e-5, atol=1e-7)
            coefs = torch.linspace(0.5, 1.5, v.numel()).reshape(v.shape)
            (v * coefs).sum().backward()
            (ref * coefs).sum().backward()
        else:
            ref = OL._TABLE[name](xr, target, "mean")
            np.testing.assert_allclose(v.item(), ref.item(), rtol=2e-5)
            v.backward()
            ref.backward()
        np.testing.assert_allclose(x.grad.numpy(), xr.grad.numpy(), rtol=2e-3, atol=1e-7)



def test_backward_statistics_come_from_the_producing_pass_where_it_offers_them(emu):
    """ctseg_conv_desc::bst_* (VERDICT r2 item 2): every InstanceNorm whose output gradient is WRITTEN by a convolution pass gets its
    backward statistics from that pass's epilogue — no ctseg_instnorm_prelu_bwd_reduce for it — and the gradients are the oracle's
    (the emulator offers the feature for every pass; the library decides per kernel).  With CTSEG_BST=0 every norm has its reduce."""
    import os
    counts = {}
    for on in ("1", "0"):
        os.environ["CTSEG_BST"] = on
        try:
            ref, net = _pair(3, 1, 10, (4, 8, 16), (2, 2), 2, seed=3)
            g = torch.Generator().manual_seed(2)
            x = torch.randn(2, 1, 8, 8, 4, generator=g)
            gy = torch.randn(2, 10, 8, 8, 4, generator=g)
            ref(x).backward(gy)
            eng = net.engine()
            eng.forward(x)
            pl = eng.last_plan
            pl.dlogits.t[..., :10].copy_(gy.permute(0, 2, 3, 4, 1))
            eng.backward(pl)
            for (k, p), q in zip(ref.named_parameters(), net.parameters()):
                np.testing.assert_allclose(eng.store.grad_view(q).numpy(), p.grad.numpy(), err_msg=k, **_tol(k, p.grad.numpy()))
            counts[on] = (sum(1 for nm, *_ in pl.bwd if nm == "ctseg_instnorm_prelu_bwd_reduce"), [f for _, f in pl.norm_bwd])
        finally:
            os.environ.pop("CTSEG_BST", None)
    n_norms = len(counts["0"][1])
    assert n_norms >= 8 and counts["0"][0] == n_norms and not any(counts["0"][1])
    fused = sum(counts["1"][1])
    assert fused == n_norms and counts["1"][0] == 0, counts      # every norm's gradient is written by a convolution pass here


def test_first_layer_weight_gradient_forms_its_upper_columns_on_load(emu):
    """ctseg_wgrad_desc::dyn_* (round 3): the first layer of the network wants no input gradient, so the weight-gradient pass of its
    fused [residual | unit0] convolution reads d_res where it lies and forms d_y0 from (g, y) of unit0's norm on load — that norm has
    no apply pass, nobody copies g into a fused operand, and its slope gradient comes from ctseg_instnorm_prelu_dalpha.  The
    gradients are torch's either way (the emulator offers the feature for fp32 plans; the library for the bf16 first layer)."""
    import os
    seen = {}
    for on in ("1", "0"):
        os.environ["CTSEG_EMU_WGRAD_DYN"] = on
        try:
            ref, net = _pair(3, 1, 10, (4, 8, 16), (2, 2), 2, seed=5)
            g = torch.Generator().manual_seed(4)
            x = torch.randn(2, 1, 8, 8, 4, generator=g)
            gy = torch.randn(2, 10, 8, 8, 4, generator=g)
            ref(x).backward(gy)
            eng = net.engine()
            eng.forward(x)
            pl = eng.last_plan
            pl.dlogits.t[..., :10].copy_(gy.permute(0, 2, 3, 4, 1))
            eng.backward(pl)
            for (k, p), q in zip(ref.named_parameters(), net.parameters()):
                np.testing.assert_allclose(eng.store.grad_view(q).numpy(), p.grad.numpy(), err_msg=k, **_tol(k, p.grad.numpy()))
            names = [nm for nm, *_ in pl.bwd]
            dyn = [a[0] for nm, _, a in pl.bwd if nm == "ctseg_conv_wgrad" and a[0].dyn_g]
            seen[on] = (sum(1 for nm in names if nm.startswith("ctseg_instnorm_prelu_bwd_apply")), names.count("ctseg_instnorm_prelu_dalpha"),
                        len(dyn), eng.store.flat_g.clone())
            if on == "1":
                assert len(dyn) == 1 and dyn[0].dyn_col0 * 2 == dyn[0].Cn and dyn[0].d_ld >= dyn[0].dyn_col0
        finally:
            os.environ.pop("CTSEG_EMU_WGRAD_DYN", None)
    assert seen["0"][2] == 0 and seen["0"][1] == 0
    assert seen["1"][0] == seen["0"][0] - 1 and seen["1"][1] == 1, seen        # one apply pass fewer, one slope-gradient launch instead
    np.testing.assert_allclose(seen["1"][3].numpy(), seen["0"][3].numpy(), rtol=1e-5, atol=1e-7)


def test_a_fused_loss_that_is_never_backpropagated_does_not_leak_its_gradient_into_the_next_backward(emu):
    """the fused training_step leaves d loss / d logits in the plan and a flag saying so; if that loss is dropped
    (skipped step, inspection under grad mode) the next forward on the plan must clear the flag, or ``model(x) + custom loss``
    would backpropagate the PREVIOUS batch's cross-entropy gradient instead of its own upstream gradient."""
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(11)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 1, 8, 8, 8, generator=g)
    masks = (torch.rand(1, 9, 8, 8, 8, generator=g) < 0.1).to(torch.uint8)
    m = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"])
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    dropped = m.training_step((x, masks, torch.ones(1, 9)), 0)      # fused route; never backpropagated
    assert dropped.requires_grad
    x2 = torch.randn(1, 1, 8, 8, 8, generator=g)
    w = torch.randn(1, 10, 8, 8, 8, generator=g)
    (m(x2) * w).sum().backward()
    fresh = BaseUNet3D(filters=[4, 8, 16], loss_fx=["CrossEntropy"])
    fresh.load_state_dict(sd)
    (fresh(x2) * w).sum().backward()
    for p, q in zip(m.parameters(), fresh.parameters()):
        assert torch.equal(p.grad, q.grad)
