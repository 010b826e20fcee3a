"""GPU: the Boundary loss on volumes — MultipleLossWrapper3D(..., device_boundary=True), LossEntry("Boundary") on 5-D input and one
BaseUNet3D step fed by compute_distance_map(spatial_dims=3).

The kernels are those of the 2-D route (ctseg_boundary_stats / ctseg_boundary_grad see B x S x C rows and [B][C-1][S] planes, whatever
the spatial rank), so the comparison target (boundary64 of reference_ops.py, any rank) and the bounds are those of
tests/test_gpu_boundary_loss.py, restated for a volume:
    p = softmax(x, 1);  T[b, c] = mean over the volume of p[b, c + 1] D[b, c];  "mean": T.mean();  exclude_missing: the non-Focal
    branch of apply_missing_mask
  * a scalar loss value: 2^-18 * sum_bc w_bc mean |p D|                                   (test_gpu_boundary_loss.py:16-17, :255)
  * its gradient beside label losses: 2^-19 * sum_j |g_j| p_j + 2^-22 * |d64| + 2^-23 * |total|          (:12-13, :260)
  * its gradient alone (the storing variant): 2^-19 * sum_j |g_j| p_j + 2^-22 * |d64|                    (:270)
  * the unreduced table: 2^-20 * mean |p D| + 2^-24 * |T64|; its mean: 2^-18 * mean of those             (:287, :292)
S = 6 * 5 * 4 = 120 voxels per sample here against 2115 there: fewer terms per sum, the same bounds.
The trainer step compares ``training_step`` + ``backward`` + Adam with ``fit_step`` by the tolerances of
tests/test_gpu_parity.py::test_autograd_drop_in_path_equals_native_step (:367 loss rtol 1e-6, :378 atol 2e-5 where the gradient is
not rounding noise, :379 atol 2.1e-3 everywhere)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capstone_amd.data import utils as DU  # noqa: E402
from reference_ops import boundary64, boundary_weights64  # noqa: E402

DEV = "cuda:0"
B, C, SP = 2, 10, (6, 5, 4)


def _inputs(seed=7):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, *SP, generator=g) * 2
    target = torch.randint(0, C, (B,) + SP, generator=g)
    D = torch.rand(B, C - 1, *SP, generator=g) * 2 - 1                      # random maps in [-1, 1]
    return logits, target, D


@pytest.mark.parametrize("exclude_missing", [False, True])
def test_wrapper_value_and_gradient_on_a_volume(exclude_missing):
    from capstone_amd.volumetric.losses import MultipleLossWrapper3D
    logits, target, D = _inputs()
    ind = torch.ones(B, 9)
    ind[1, 3] = 0
    ind[:, 6] = 0                                # a zero column: 1 / 0 -> the isinf branch (used under exclude_missing only)
    Wt = boundary_weights64(ind, exclude_missing, B, 9)
    val, mag, gb, gabs = boundary64(logits, [(D, Wt)])
    old = MultipleLossWrapper3D(["Dice", "Focal"], exclude_missing=exclude_missing)
    xo = logits.to(DEV).requires_grad_(True)
    vo = old(xo, target.to(DEV), mask_indicator=ind.to(DEV))
    torch.stack(list(vo.values())).sum().backward()
    wrap = MultipleLossWrapper3D(["Boundary", "Dice", "Focal"], exclude_missing=exclude_missing, device_boundary=True)
    x = logits.to(DEV).requires_grad_(True)
    v = wrap(x, target.to(DEV), mask_indicator=ind.to(DEV), dist_maps=D.to(DEV))
    assert list(v) == ["Boundary", "Dice", "Focal"]
    print(f"Boundary value {v['Boundary'].item():.9g} vs {val:.9g}, magnitude {mag:.3e}")
    assert abs(v["Boundary"].item() - val) <= 2.0 ** -18 * mag
    assert v["Dice"].item() == vo["Dice"].item() and v["Focal"].item() == vo["Focal"].item()
    torch.stack(list(v.values())).sum().backward()
    total = xo.grad.cpu().double() + gb
    err = (x.grad.cpu().double() - total).abs()
    bound = 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs() + 2.0 ** -23 * total.abs()
    print(f"wrapper gradient: worst error / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()) and float(gb.abs().max()) > 0
    # Boundary alone: the storing variant, no label pass
    x1 = logits.to(DEV).requires_grad_(True)
    only = MultipleLossWrapper3D(["Boundary"], exclude_missing=exclude_missing, device_boundary=True)
    v1 = only(x1, target.to(DEV), mask_indicator=ind.to(DEV), dist_maps=D.to(DEV))["Boundary"]
    assert v1.item() == v["Boundary"].item()
    v1.backward()
    err = (x1.grad.cpu().double() - gb).abs()
    print(f"Boundary alone, gradient: worst error / bound = {float((err / (2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs())).max()):.3e}")
    assert bool((err <= 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs()).all())
    with pytest.raises(ValueError):
        only(x1, target.to(DEV), dist_maps=D.to(DEV)[:, :, :3])                           # maps of another volume


def test_the_boundary_entry_on_5d_input():
    from capstone_amd.models.losses import LossEntry
    logits, _, D = _inputs(seed=8)
    gT = torch.randn(B, 9, generator=torch.Generator().manual_seed(9))
    _, _, gb, gabs = boundary64(logits, [(D, gT.double())])
    x = logits.to(DEV).requires_grad_(True)
    T = LossEntry("Boundary", "none")(x, D.to(DEV))
    assert T.shape == (B, 9) and T.dtype == torch.float32
    p = torch.softmax(logits.double(), dim=1)[:, 1:] * D.double()
    T64, Tabs = p.mean(dim=(2, 3, 4)), p.abs().mean(dim=(2, 3, 4))
    assert bool(((T.cpu().double() - T64).abs() <= 2.0 ** -20 * Tabs + 2.0 ** -24 * T64.abs()).all())
    (T * gT.to(DEV)).sum().backward()
    err = (x.grad.cpu().double() - gb).abs()
    assert bool((err <= 2.0 ** -19 * gabs + 2.0 ** -22 * gb.abs()).all())
    m = LossEntry("Boundary", "mean")(logits.to(DEV), D.to(DEV))
    assert abs(m.item() - T64.mean().item()) <= 2.0 ** -18 * Tabs.mean().item()
    with pytest.raises(AssertionError, match="rank"):
        LossEntry("Boundary", "mean")(logits.to(DEV), D.to(DEV).flatten(3))               # 5-D logits need 5-D maps


def _batch():
    g = torch.Generator().manual_seed(12)
    images = torch.randn(2, 1, 16, 16, 16, generator=g)
    masks = torch.zeros(2, 9, 16, 16, 16, dtype=torch.uint8)
    for b in range(2):
        for k in range(9):
            masks[b, k, k + 1:k + 6, 3 + b:12, 2:9 + k % 3] = 1             # overlapping boxes
    masks[1, 4] = 0                                                         # an absent class
    masks = masks.to(DEV)
    maps = DU.compute_distance_map(masks, spatial_dims=3)
    return images.to(DEV), masks, torch.ones(2, 9, device=DEV), maps


def _model(names, sd=None, **kw):
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(5)
    m = BaseUNet3D(filters=[4, 8, 8, 8, 8], loss_fx=list(names), **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def test_one_training_step_with_the_boundary_loss():
    batch = _batch()
    assert batch[3].shape == (2, 9, 16, 16, 16) and bool(batch[3].any()) and not bool(batch[3][1, 4].any())
    m1 = _model(["Boundary", "CrossEntropy"], device_boundary=True)
    sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    m2 = _model(["Boundary", "CrossEntropy"], sd, device_boundary=True)
    opt = m1.configure_optimizers()
    opt.zero_grad()
    loss = m1.training_step(batch, 0)
    loss.backward()
    opt.step()
    loss2 = m2.fit_step(batch)
    torch.cuda.synchronize()
    for name in ("Boundary", "CrossEntropy"):
        a, b = m1.logged[f"{name} Loss (train)"].item(), m2.logged[f"{name} Loss (train)"].item()
        print(f"{name}: training_step {a:.9g}, fit_step {b:.9g}")
        np.testing.assert_allclose(a, b, rtol=1e-6)
    np.testing.assert_allclose(loss.item(), loss2.item(), rtol=1e-6)
    np.testing.assert_allclose(m1.logged["Mean Dice Score (train)"].item(), m2.logged["Mean Dice Score (train)"].item(), rtol=1e-6)
    # the Boundary value itself against float64, from the logits the native step kept (bound: test_gpu_boundary_loss.py:365)
    y = m2.unet.engine().logits_view().detach().float().cpu()
    val, mag, _, _ = boundary64(y, [(batch[3].cpu(), torch.full((2, 9), 1.0 / 18, dtype=torch.float64))])
    assert abs(m2.logged["Boundary Loss (train)"].item() - val) <= 2.0 ** -18 * mag and mag > 0
    store = m2.unet.engine().store
    grads = {k: store.grad_view(q).detach().cpu().clone() for k, q in m2.named_parameters()}
    worst = 0.0
    for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
        wa, wn, gref = p.detach().cpu().numpy(), q.detach().cpu().numpy(), grads[k].numpy()
        real = np.abs(gref) > 1e-4 * max(float(np.abs(gref).max()), 1e-6)
        if k.endswith(".bias") and "residual" not in k:
            real &= False
        worst = max(worst, float(np.abs(wa - wn)[real].max()) if real.any() else 0.0)
        np.testing.assert_allclose(wa[real], wn[real], rtol=0, atol=2e-5, err_msg=k)
        np.testing.assert_allclose(wa, wn, rtol=0, atol=2.1e-3, err_msg=k)
        if real.any():
            assert np.abs(wn - sd[k].numpy())[real].max() > 0.5e-3, k       # and a step was taken at all (lr = 1e-3, :382)
    print(f"parameters after one Adam step, drop-in vs native: worst difference {worst:.3e}")
    # the same network under ["CrossEntropy"] alone (the fused route, which ignores the fourth element when the flag is on)
    m3 = _model(["CrossEntropy"], sd, device_boundary=True)
    m3.fit_step(batch)
    torch.cuda.synchronize()
    other = {k: m3.unet.engine().store.grad_view(q).detach().cpu() for k, q in m3.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert sum(not torch.equal(grads[k], other[k]) for k in grads) >= len(grads) // 2
    with torch.no_grad():
        m1.validation_step(batch)
    assert "Boundary Loss (val)" in m1.logged
    off = _model(["CrossEntropy"], sd)
    with pytest.raises(NotImplementedError, match="device_boundary=True"):
        off.fit_step(batch)


def test_boundary_alone_stores_its_gradient_and_still_counts_dice():
    batch = _batch()
    m1 = _model(["Boundary"], device_boundary=True)
    sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    m2 = _model(["Boundary"], sd, device_boundary=True)
    ref = _model(["Boundary", "Dice"], sd, device_boundary=True)
    loss = m1.training_step(batch, 0)
    loss.backward()
    loss2 = m2.fit_step(batch)
    ref.fit_step(batch)
    torch.cuda.synchronize()
    np.testing.assert_allclose(loss.item(), loss2.item(), rtol=1e-6)
    np.testing.assert_allclose(loss2.item(), ref.logged["Boundary Loss (train)"].item(), rtol=1e-6)
    for m in (m1, m2):          # the Dice metric comes from the label pass, which a Boundary-only step runs for it
        np.testing.assert_allclose(m.logged["Mean Dice Score (train)"].item(), ref.logged["Mean Dice Score (train)"].item(), rtol=1e-6)
    g1 = [m1.unet.engine().store.grad_view(q).detach().cpu() for q in m1.parameters()]
    g2 = [m2.unet.engine().store.grad_view(q).detach().cpu() for q in m2.parameters()]
    assert any(float(a.abs().max()) > 0 for a in g1)
    for a, b in zip(g1, g2):    # the same recorded programs behind the same loss gradient: equal to reduction-order rounding
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-4, atol=1e-6 * max(float(b.abs().max()), 1e-12))
