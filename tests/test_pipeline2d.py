"""The 2-D device input pipeline: capstone_amd.transforms / capstone_amd.data and ctseg_pipeline2d_batch.

Held to the ``o_*`` oracle of tests/plane_oracles.py.  CPU tests route the C ABI through an emulator whose pipeline entry IS the
oracle; GPU tests compare the HIP kernel with the oracle by array_equal.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import _native as nat
from capstone_amd.data import data_module as DM
from capstone_amd.data import datasets as DS
from capstone_amd.transforms import BatchPipeline2D, SliceStore2D, predefined
from capstone_amd.transforms import transforms_2d as T2
from feature_emulators import MixupEntries, Pipeline2dEntries
from helpers import check_bit_exact
from plane_oracles import DEV, MEAN3, SOFT, STD3, WINDOWS3, _write_npz, make_masks, make_raw, o_normalize, o_window, oracle_batch

class E(Pipeline2dEntries, MixupEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E()) as e:
        yield e


def run_pipeline(raws, masks, rows, mode, size, windows, shift, normalize, device):
    store = SliceStore2D(raws, masks, device=device)
    mean, std = (None, None) if not normalize else ((MEAN3, STD3) if len(windows) == 3 else (MEAN3[1], STD3[1]))
    pipe = BatchPipeline2D(windows, mode, size, mean, std, shift=shift)
    rows = np.asarray(rows)
    params = rows[:, 1:] if mode == "crop" else None
    img_a, m_a, pres_a = pipe(store, rows[:, 0], params=params)
    img_b, lab_b, pres_b = pipe.squashing()(store, rows[:, 0], params=params)
    ref = oracle_batch([np.asarray(r) for r in raws], [np.asarray(m).astype(np.uint8) for m in masks], rows.tolist(), mode, size, windows,
                       shift, None if not normalize else pipe.mean, None if not normalize else pipe.denom)
    got = dict(image=img_a.cpu().numpy(), image_sq=img_b.cpu().numpy(), masks=m_a.cpu().numpy(), labels=lab_b.cpu().numpy(),
               present=pres_a.cpu().numpy(), present_sq=pres_b.cpu().numpy(), hist=lab_b._ctseg_labels[1].cpu().numpy(),
               flat=lab_b._ctseg_labels[0].cpu().numpy())
    return got, ref


CROP_SHAPES = [(37, 29), (20, 20), (21, 40)]


def crop_rows(size, ks):
    """every slice x {four corners, one interior origin} x k x flip"""
    Ho, Wo = size
    rows = []
    for i, (H, W) in enumerate(CROP_SHAPES):
        origins = sorted({(0, 0), (0, W - Wo), (H - Ho, 0), (H - Ho, W - Wo), ((H - Ho) // 2, (W - Wo + 1) // 2)})
        rows += [(i, y0, x0, k, f) for (y0, x0), k, f in itertools.product(origins, ks, (0, 1))]
    return rows


# ---- CPU tests ---------------------------------------------------------------------------------------------------------------
def test_presets_are_the_reference_presets():
    assert T2.WINDOWING_CONFIG == {"brain": (80, 40), "soft_tissue": (350, 20), "bone": (2800, 600)}
    p1, p2 = predefined.windowed_degree_1, predefined.windowed_degree_2
    assert p1["train"] is p1["test"] and p2["test"] is p1["test"]
    for p, mode in ((p1["test"], 1), (p2["train"], 0)):
        assert p.windows == WINDOWS3 and p.mode == mode and p.size == (256, 256) and p.shift and not p.squash
        assert p.mean.dtype == np.float32 and np.array_equal(p.mean, np.float32(MEAN3))
        assert np.array_equal(p.denom, np.reciprocal(np.float32(STD3))) and p.denom.dtype == np.float32
    t0 = predefined.degree_0["test"]
    assert t0.windows == SOFT and t0.mode == 1 and t0.size == (256, 256)
    assert np.array_equal(t0.mean, np.float32([MEAN3[1]])) and np.array_equal(t0.denom, np.reciprocal(np.float32([STD3[1]])))
    for name in ("windowed_degree_3", "windowed_degree_4"):
        assert getattr(predefined, name)["test"] is p1["test"]
    assert T2.BrainWindowing().window_width == 80 and T2.BoneWindowing().window_level == 600
    assert T2.SoftTissueWindowing(shift=False).shift is False
    assert T2.WindowingBase(5, 6).get_transform_init_args_names() == ("window_width", "window_level")


def test_refusals(tmp_path):
    for name in ("degree_0", "windowed_degree_3", "windowed_degree_4"):
        with pytest.raises(NotImplementedError):
            getattr(predefined, name)["train"]
    with pytest.raises(NotImplementedError):
        DS.get_miccai_2d("train", transform=predefined.windowed_degree_1["train"], enhanced=True, root=str(tmp_path))
    with pytest.raises(AssertionError):
        DM.MiccaiDataModule2D(4, transform_degree=7)
    # CPU tensors: no fallback
    store = SliceStore2D([make_raw((12, 12), np.int16, 0)], [make_masks((12, 12), 0)], device="cpu")
    pipe = BatchPipeline2D(WINDOWS3, "crop", (8, 8), MEAN3, STD3)
    with pytest.raises(nat.NativeError):
        pipe(store, [0], params=[(0, 0, 0, 0)])
    with pytest.raises(nat.NativeError):
        T2.apply_window(torch.zeros(4, 4), 80, 40)
    with pytest.raises(nat.NativeError):
        T2.WindowedChannels().apply(torch.zeros(4, 4, 1))


def test_out_of_range_crops_are_refused_on_the_host(emu):
    store = SliceStore2D([make_raw((12, 15), np.int16, 0)], [make_masks((12, 15), 0)], device="cpu")
    pipe = BatchPipeline2D(WINDOWS3, "crop", (8, 8), MEAN3, STD3)
    pipe(store, [0], params=[(4, 7, 3, 1)])                                 # the last valid origin
    for bad in ((5, 0, 0, 0), (0, 8, 0, 0), (-1, 0, 0, 0), (0, -1, 0, 0)):
        with pytest.raises(nat.NativeError):
            pipe(store, [0], params=[bad])
    with pytest.raises(nat.NativeError):
        BatchPipeline2D(WINDOWS3, "crop", (16, 8)).draw_params([(12, 15)])   # a crop larger than the slice
    with pytest.raises(IndexError):
        pipe(store, [1], params=[(0, 0, 0, 0)])
    with pytest.raises(nat.NativeError):                                    # odd k, 6 x 8 output
        BatchPipeline2D(WINDOWS3, "crop", (6, 8))(store, [0], params=[(0, 0, 1, 0)])


def test_the_library_validates_the_host_table_before_any_launch():
    """ctseg_pipeline2d_batch itself (no device is touched: every case fails validation): odd k with a non-square output, a crop
    outside its slice, a slice outside its store"""
    L = nat.lib()
    i32x3, f32x3 = ctypes.c_int32 * 3, ctypes.c_float * 3
    lo, hi, mean, den = i32x3(0, -155, -800), i32x3(80, 195, 2000), f32x3(*MEAN3), f32x3(*STD3)

    def call(row, Ho, Wo, mode=0, elems=400):
        t = np.array([row], dtype=np.int64)
        return L.ctseg_pipeline2d_batch(4096, nat.I16, elems, 8192, 9 * elems, 16384, t.ctypes.data, 1, 9, mode, Ho, Wo, 3, lo, hi, 1,
                                        mean, den, 32768, 65536, None, None, None, None)
    assert call([0, 0, 20, 20, 0, 0, 1, 0], 6, 8) < 0 and b"odd k" in L.ctseg_last_error()
    assert call([0, 0, 20, 20, 0, 0, 3, 1], 6, 8) < 0 and b"odd k" in L.ctseg_last_error()
    assert call([0, 0, 20, 20, 15, 0, 0, 0], 6, 8) < 0 and b"leaves" in L.ctseg_last_error()
    assert call([0, 0, 20, 20, 0, 13, 2, 0], 6, 8) < 0 and b"leaves" in L.ctseg_last_error()
    assert call([0, 0, 20, 20, 0, 0, 4, 0], 8, 8) < 0
    assert call([1, 0, 20, 20, 0, 0, 0, 0], 8, 8) < 0 and b"outside" in L.ctseg_last_error()
    assert call([0, 0, 20, 21, 0, 0, 0, 0], 8, 8, mode=1) < 0 and b"outside" in L.ctseg_last_error()
    assert call([0, 0, 20, 20, 0, 0, 0, 0], 8, 8, mode=2) < 0


def test_drawn_params_stay_in_range_and_follow_the_reference_probabilities():
    pipe = BatchPipeline2D(WINDOWS3, "crop", (20, 20))
    sizes = np.array([CROP_SHAPES[i % 3] for i in range(3000)])
    p = pipe.draw_params(sizes, np.random.default_rng(7))
    assert p.shape == (3000, 4) and p.dtype == np.int64
    assert (p[:, 0] >= 0).all() and (p[:, 0] + 20 <= sizes[:, 0]).all() and (p[:, 1] >= 0).all() and (p[:, 1] + 20 <= sizes[:, 1]).all()
    assert (p[sizes[:, 0] == 20, :2] == 0).all()
    assert set(p[:, 2]) == {0, 1, 2, 3} and set(p[:, 3]) == {0, 1}
    assert p[sizes[:, 0] == 37, 0].max() == 17 and p[sizes[:, 1] == 40, 1].max() == 20       # the valid range is reached
    # rot90 applies with p = 0.5 and then draws k uniformly from 0..3: k == 0 has probability 5/8; flip 1/2 (3000 draws: 5 sigma)
    assert abs((p[:, 2] == 0).mean() - 0.625) < 0.045 and abs(p[:, 3].mean() - 0.5) < 0.046
    assert np.array_equal(p, pipe.draw_params(sizes, np.random.default_rng(7)))
    q = BatchPipeline2D(WINDOWS3, "crop", (7, 9)).draw_params(sizes, np.random.default_rng(7))
    assert set(q[:, 2]) == {0, 2}                                           # a non-square size is never turned by an odd k


def test_dataset_store_and_items(emu, tmp_path):
    raws, masks, inds = _write_npz(tmp_path, "train", 5, 3, bool_masks=True)
    pipe = BatchPipeline2D(WINDOWS3, "resize", (8, 8), MEAN3, STD3)
    ds = DS.get_miccai_2d("train", transform=pipe, root=str(tmp_path), device="cpu")
    assert len(ds) == 5 and [p[-11:] for p in ds.instance_paths] == [f"case{i:03d}.npz" for i in range(5)]
    st = ds.store
    assert st.K == 9 and st.images.dtype == torch.int16 and st.masks.dtype == torch.uint8
    npix = np.array([r.size for r in raws])
    assert np.array_equal(st.table[:, 0], np.concatenate(([0], np.cumsum(npix)[:-1]))) and np.array_equal(st.table[:, 1], 9 * st.table[:, 0])
    assert np.array_equal(st.table[:, 2:], [r.shape for r in raws]) and st.images.numel() == npix.sum() and st.masks.numel() == 9 * npix.sum()
    for i in (0, 3):
        im, m = st.raw(i)
        assert np.array_equal(im.numpy(), raws[i]) and np.array_equal(m.numpy(), masks[i].astype(np.uint8))
    assert ds.mask_indicator.shape == (5, 9) and np.array_equal(ds.mask_indicator.numpy(), np.stack(inds))
    image, m, ind = ds[2]
    ref = oracle_batch(raws, [x.astype(np.uint8) for x in masks], [(2, 0, 0, 0, 0)], "resize", (8, 8), WINDOWS3, True, pipe.mean, pipe.denom)
    assert image.shape == (3, 8, 8) and m.shape == (9, 8, 8) and m.dtype == torch.uint8 and ind.shape == (9,)
    assert np.array_equal(image.numpy(), ref["image"][0]) and np.array_equal(m.numpy(), ref["masks"][0])
    assert np.array_equal(ind.numpy(), inds[2])
    images, mb, indb = ds.batch([4, 0, 4])
    assert images.shape == (3, 3, 8, 8) and mb.shape == (3, 9, 8, 8) and torch.equal(images[0], images[2])
    assert np.array_equal(indb.numpy(), np.stack([inds[4], inds[0], inds[4]]))
    raw_ds = DS.MiccaiDataset2D(str(tmp_path / "miccai_2d" / "train"), transform=None, device="cpu")
    image, m, ind = raw_ds[1]
    assert image.shape == raws[1].shape + (1,) and np.array_equal(m.numpy(), masks[1].astype(np.uint8))
    # the reference's asserts
    bad = tmp_path / "bad"
    bad.mkdir()
    np.savez(bad / "x.npz", image=raws[0][None], masks=masks[0][:8], mask_indicator=inds[0])
    with pytest.raises(AssertionError):
        DS.MiccaiDataset2D(str(bad), transform=pipe, device="cpu")


def test_data_module_batches_and_shuffling(emu, tmp_path, monkeypatch):
    for split, n, seed in (("train", 7, 10), ("valid", 3, 20), ("test", 2, 30)):
        _write_npz(tmp_path, split, n, seed, bool_masks=False)
    small = BatchPipeline2D(WINDOWS3, "crop", (8, 8), MEAN3, STD3)
    test_side = BatchPipeline2D(WINDOWS3, "resize", (8, 8), MEAN3, STD3)
    monkeypatch.setitem(DM.DEGREE, 2, {"train": small, "test": test_side})
    dm = DM.MiccaiDataModule2D(3, transform_degree=2, root=str(tmp_path), device="cpu", generator=np.random.default_rng(5))
    dm.setup("fit")
    assert not hasattr(dm, "test_dataset") and dm.train_dataset.transform is small and dm.val_dataset.transform is test_side
    loader = dm.train_dataloader()
    assert len(loader) == 3
    first = loader.order()
    assert sorted(first) == list(range(7)) and list(first) != list(range(7))
    assert list(DM.DeviceBatches([dm.train_dataset], 3, True, np.random.default_rng(5)).order()) == list(
        DM.DeviceBatches([dm.train_dataset], 3, True, np.random.default_rng(5)).order())
    shapes = [(tuple(i.shape), tuple(m.shape), tuple(ind.shape)) for i, m, ind in loader]
    assert shapes == [((3, 3, 8, 8), (3, 9, 8, 8), (3, 9))] * 2 + [((1, 3, 8, 8), (1, 9, 8, 8), (1, 9))]
    val = list(dm.val_dataloader())
    assert len(val) == 1 and val[0][0].shape == (3, 3, 8, 8)
    assert np.array_equal(val[0][2].cpu().numpy(), dm.val_dataset.mask_indicator.numpy())      # sequential order
    dm.setup("test")
    assert [b[0].shape[0] for b in dm.test_dataloader()] == [2]
    full = DM.FullMiccaiDataModule2D(4, transform_degree=2, root=str(tmp_path), device="cpu", generator=np.random.default_rng(6))
    full.setup(None)
    batches = list(full.train_dataloader())
    assert [b[0].shape[0] for b in batches] == [4, 4, 2] and all(b[1].shape[1:] == (9, 8, 8) for b in batches)
    assert all(b[1]._ctseg_present.shape == (b[0].shape[0], 9) for b in batches)


def test_weighted_mixup_takes_the_stashed_present(emu):
    from capstone_amd.training import utils as U
    raws = [make_raw((12, 12), np.int16, s) for s in range(4)]
    masks = [make_masks((12, 12), s) for s in range(4)]
    masks[3][:] = 0                                                         # a slice that holds nothing
    store = SliceStore2D(raws, masks, device="cpu")
    pipe = BatchPipeline2D(WINDOWS3, "crop", (8, 8), MEAN3, STD3)
    params = [(0, 0, 0, 0), (4, 4, 1, 1), (2, 1, 2, 0), (1, 3, 3, 1)]
    images, m9, present = pipe(store, [0, 1, 2, 3], params=params)
    images_sq, labels, present_sq = pipe.squashing()(store, [0, 1, 2, 3], params=params)
    assert torch.equal(present, present_sq) and labels._ctseg_present is present_sq and len(labels._ctseg_labels) == 2
    assert torch.equal(present.bool(), (m9 == 1).flatten(2).any(2))
    assert present[:3, 1].all() and (labels._ctseg_labels[1][:3, 2] == 0).all() and present[3].sum() == 0
    assert torch.equal(U.mixup_probability(present_sq), U.mixup_probability((m9 == 1).flatten(2).any(2).int()))
    raw9 = m9.clone()                                                       # raw masks without any stash
    forced = torch.tensor([2, 0, 3, 1])
    a = U.weighted_mixup(images, raw9, index=forced, lambda_=0.3)
    b = U.weighted_mixup(images_sq, labels, index=forced, lambda_=0.3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert len(labels._ctseg_labels) == 2                                   # the stash was used, not rebuilt
    torch.manual_seed(3)
    a = U.weighted_mixup(images, m9.clone(), lambda_=0.3)
    torch.manual_seed(3)
    b = U.weighted_mixup(images_sq, labels, lambda_=0.3)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    # the step's _squash_masks is a lookup on either kind of batch
    assert torch.equal(U._squash_masks(labels, 10), U._squash_masks(raw9, 10))


def test_window_transforms_through_the_emulator(emu):
    raw = make_raw((9, 7), np.int16, 1)
    t = torch.from_numpy(raw)
    out = T2.WindowedChannels().apply(t[:, :, None])
    assert out.shape == (9, 7, 3) and out.dtype == torch.float32
    for c, (w, l) in enumerate(WINDOWS3):
        assert np.array_equal(out[:, :, c].numpy(), o_window(raw, w, l, True).astype(np.float32))
    assert np.array_equal(T2.SoftTissueWindowing(shift=False).apply(t).numpy()[:, :, 0], np.clip(raw, -155, 195).astype(np.float32))


# ---- GPU tests: the kernel against the oracle, bit for bit -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int16, np.uint8, np.float32])
@pytest.mark.parametrize("windows,shift", [(WINDOWS3, True), (WINDOWS3, False), (SOFT, True), (SOFT, False)])
def test_gpu_crop_rot90_flip_is_bit_exact(dtype, windows, shift):
    raws = [make_raw(s, dtype, 11 + i) for i, s in enumerate(CROP_SHAPES)]
    masks = [make_masks(s, 21 + i) for i, s in enumerate(CROP_SHAPES)]
    got, ref = run_pipeline(raws, masks, crop_rows((20, 20), (0, 1, 2, 3)), "crop", (20, 20), windows, shift, True, DEV)
    check_bit_exact(got, ref)
    assert (ref["present"][:, 1] == 1).all() and (ref["hist"][:, 2] == 0).all()         # covered: present, not in the histogram
    assert (ref["present"][:, 4] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_gpu_crop_of_a_non_square_unaligned_size(dtype):
    raws = [make_raw(s, dtype, 31 + i) for i, s in enumerate(CROP_SHAPES)]
    masks = [make_masks(s, 41 + i) for i, s in enumerate(CROP_SHAPES)]
    got, ref = run_pipeline(raws, masks, crop_rows((7, 9), (0, 2)), "crop", (7, 9), WINDOWS3, True, True, DEV)
    check_bit_exact(got, ref)
    got, ref = run_pipeline(raws, masks, crop_rows((7, 9), (0, 2)), "crop", (7, 9), SOFT, True, False, DEV)      # no normalization
    check_bit_exact(got, ref)


RESIZES = [((13, 17), (8, 8)), ((5, 6), (20, 12)), ((16, 16), (8, 8)), ((9, 9), (9, 9))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int16, np.uint8, np.float32])
@pytest.mark.parametrize("src,dst", RESIZES)
def test_gpu_resize_is_bit_exact(dtype, src, dst):
    raws = [make_raw(src, dtype, 51 + i) for i in range(3)]
    masks = [make_masks(src, 61 + i) for i in range(3)]
    rows = [(i, 0, 0, 0, 0) for i in (2, 0, 1, 0)]
    for windows, shift in ((WINDOWS3, True), (SOFT, False)):
        got, ref = run_pipeline(raws, masks, rows, "resize", dst, windows, shift, True, DEV)
        check_bit_exact(got, ref)
    if src == dst:                                          # identity: the windowed, normalized slice itself
        same = oracle_batch(raws, masks, rows, "crop", dst, SOFT, False, [np.float32(MEAN3[1])], [np.reciprocal(np.float32(STD3[1]))])
        assert np.array_equal(got["image"], same["image"]) and np.array_equal(got["masks"], same["masks"])
    if src == (16, 16):                                     # exact 2:1: the float64 mean of each 2 x 2 block, pairs first
        w = o_window(raws[2], *SOFT[0], False)
        mean22 = ((w[0::2, 0::2] + w[0::2, 1::2]) / 2 + (w[1::2, 0::2] + w[1::2, 1::2]) / 2) / 2
        assert np.array_equal(got["image"][0, 0], o_normalize(mean22, MEAN3[1], np.reciprocal(np.float32(STD3[1]))))


@pytest.mark.gpu
def test_gpu_trainers_take_the_pre_squashed_batch():
    """BaseUNet2D on a 9-mask batch and on the pre-squashed batch of the same slices: the same loss; MixupUNet2D steps on the
    pre-squashed batch (64 x 64, the smallest slice of the 2-D trainer tests)."""
    from capstone_amd.training.base_trainer import BaseUNet2D
    from capstone_amd.training.mixup_trainer import MixupUNet2D
    shapes = [(70, 81), (64, 64), (90, 66)]
    raws = [make_raw(s, np.int16, 71 + i) for i, s in enumerate(shapes)]
    masks = []
    for i, s in enumerate(shapes):                          # blocks of structures, some overlapping
        m = np.zeros((9,) + s, np.uint8)
        for k in range(9):
            m[k, 6 * k + 3:6 * k + 12, 8 + 4 * i:56] = (k + i) % 4 != 0
        masks.append(m)
    store = SliceStore2D(raws, masks, device=DEV)
    pipe = BatchPipeline2D(WINDOWS3, "crop", (64, 64), MEAN3, STD3)
    params = [(3, 9, 1, 0), (0, 0, 2, 1), (26, 2, 0, 1)]
    images, m9, _ = pipe(store, [0, 1, 2], params=params)
    images_sq, labels, present = pipe.squashing()(store, [0, 1, 2], params=params)
    assert torch.equal(images, images_sq) and labels.shape == (3, 64, 64) and labels.dtype == torch.uint8
    ind = torch.ones(3, 9, device=DEV)
    torch.manual_seed(5)
    model = BaseUNet2D(filters=[8, 16, 32, 64, 128], use_res_units=True, loss_fx=["Focal", "Dice"], transform_degree=1)
    model.to(DEV)
    loss_a = model.training_step((images, m9, ind)).item()
    loss_b = model.training_step((images_sq, labels, ind)).item()
    assert np.isfinite(loss_a) and loss_a == loss_b, (loss_a, loss_b)
    torch.manual_seed(5)
    mix = MixupUNet2D(filters=[8, 16, 32, 64, 128], use_res_units=True, loss_fx=["Focal", "Dice"], transform_degree=1)
    mix.to(DEV)
    loss = mix.training_step((images_sq, labels, ind))
    loss.backward()
    assert np.isfinite(loss.item()) and len(labels._ctseg_labels) == 2 and labels._ctseg_present is present
