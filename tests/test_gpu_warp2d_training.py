"""GPU: the reference's default 2-D recipe end to end — MiccaiDataModule2D(transform_degree=0, device_warps=True) over a synthetic
.npz tree feeds BaseUNet2D and, through a squashing pipeline, MixupUNet2D."""
import numpy as np
import pytest
import torch

from capstone_amd.data import data_module as DM
from capstone_amd.transforms import ElasticTransform, GridDistortion, WarpPipeline2D, predefined
from plane_oracles import DEV, MEAN3, SOFT, STD3, make_raw


def _write_tree(root, split, n, seed):
    d = root / "miccai_2d" / split
    d.mkdir(parents=True)
    rng = np.random.default_rng(seed)
    for i in range(n):
        shape = (int(rng.integers(40, 56)), int(rng.integers(40, 56)))
        m = np.zeros((9,) + shape, np.uint8)
        for k in range(9):                                  # blocks of structures, some overlapping
            m[k, 3 * k + 2:3 * k + 10, 6 + i:34] = (k + i) % 4 != 0
        np.savez(d / f"case{i:03d}.npz", image=make_raw(shape, np.int16, seed + i)[None], masks=m, mask_indicator=np.ones(9))


@pytest.mark.gpu
def test_gpu_default_recipe_trains_base_and_mixup(tmp_path, monkeypatch):
    from capstone_amd.training.base_trainer import BaseUNet2D
    from capstone_amd.training.mixup_trainer import MixupUNet2D
    _write_tree(tmp_path, "train", 8, 3)
    _write_tree(tmp_path, "valid", 2, 50)
    ref = predefined.warped["degree_0"]["train"]
    small = WarpPipeline2D(SOFT, (32, 32), MEAN3[1], STD3[1], warps=[ElasticTransform(), GridDistortion()], oneof=ref.oneof, rot_flip=ref.rot_flip)
    monkeypatch.setitem(DM.WARPED_DEGREE, 0, {"train": small, "test": predefined.warped["degree_0"]["test"]})
    dm = DM.MiccaiDataModule2D(4, transform_degree=0, device_warps=True, root=str(tmp_path), device=DEV, generator=np.random.default_rng(9))
    dm.setup("fit")
    assert dm.train_dataset.transform is small
    batches = list(dm.train_dataloader())
    assert len(batches) == 2 and batches[0][0].shape == (4, 1, 32, 32) and batches[0][1].shape == (4, 9, 32, 32)
    assert all(torch.isfinite(b[0]).all() for b in batches)
    torch.manual_seed(5)
    model = BaseUNet2D(filters=[8, 16, 32, 64, 128], use_res_units=True, loss_fx=["Focal", "Dice"], transform_degree=0)
    model.to(DEV)
    opt = model.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, tuple) else opt["optimizer"] if isinstance(opt, dict) else opt
    before = [p.detach().clone() for p in model.parameters()]
    for batch in batches:
        loss = model.training_step(batch)
        assert np.isfinite(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    # MixupUNet2D on the pre-squashed label maps of the same recipe
    dm.train_dataset.transform = small.squashing()
    images, labels, ind = next(iter(dm.train_dataloader()))
    assert labels.shape == (4, 32, 32) and labels.dtype == torch.uint8 and len(labels._ctseg_labels) == 2
    torch.manual_seed(5)
    mix = MixupUNet2D(filters=[8, 16, 32, 64, 128], use_res_units=True, loss_fx=["Focal", "Dice"], transform_degree=0)
    mix.to(DEV)
    loss = mix.training_step((images, labels, ind))
    loss.backward()
    assert np.isfinite(loss.item())
