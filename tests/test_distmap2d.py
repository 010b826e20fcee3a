"""Device distance maps of the 2-D pipeline: ctseg_distmap2d_batch, capstone_amd.data.utils.compute_distance_map,
EnhancedMiccaiDataset2D and the data modules with ``enhanced=True, device_maps=True``.

Held to ``distance_oracles.oracle`` on planes (nd = 2) and, through it, to tests/golden/distmap2d_reference.npz.  CPU tests route the
entry through an emulator whose ctseg_distmap2d_batch IS the oracle; GPU tests hold the kernel to the oracle by array_equal.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import distance_oracles as DO
from abi_emulator import Emulator, emulated
from capstone_amd import _native as nat
from capstone_amd.data import data_module as DM
from capstone_amd.data import datasets as DS
from capstone_amd.data import utils as DU
from capstone_amd.transforms import BatchPipeline2D, ElasticTransform, GridDistortion, SliceStore2D, WarpPipeline2D, predefined
from distance_oracles import DEV, isqrt, pattern_planes, separable_d2_to
from distance_oracles import blobs as discs
from feature_emulators import Distmap2dEntries, MixupEntries, Pipeline2dEntries, Warp2dEntries
from plane_oracles import MEAN3, STD3, WINDOWS3, _write_npz, make_masks, make_raw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distmap2d_reference.npz")
STACKS = ("discs", "discs_small", "long", "patterns")


class E(Distmap2dEntries, Warp2dEntries, Pipeline2dEntries, MixupEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E()) as e:
        yield e


def oracle(planes, d2_to=None):
    return DO.oracle(planes, 2, d2_to)


def check_reference_mode(planes, d2_to=None):
    return DO.check_reference_mode(planes, 2, d2_to)


signed_map = functools.partial(DO.signed_map, nd=2)
run_gpu = functools.partial(DO.run_gpu, nd=2)


# ---- CPU tests ---------------------------------------------------------------------------------------------------------------
def test_the_oracle_equals_the_reference_fixture_exactly():
    fx = np.load(GOLDEN, allow_pickle=False)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    seen_wrap = False
    for name in STACKS:
        m, ref = fx[f"{name}_masks"], fx[f"{name}_maps"]
        assert m.dtype == np.uint8 and m.shape[0] == 9 and ref.dtype == np.float64 and ref.shape == m.shape
        assert not (m != 0).all(axis=(1, 2)).any()                          # no all-foreground plane
        d2f, _, got = oracle(m)
        assert got.dtype == np.float64 and np.array_equal(got, ref), name
        seen_wrap |= bool((d2f > 255 * 255).any())
    m = fx["discs_masks"]
    assert not m[4].any() and not fx["discs_maps"][4].any()                 # an absent class
    assert ((m[1] != 0) <= (m[5] != 0)).all() and m[1].any()                # overlapping structures
    assert set(np.unique(m)) - {0, 1}                                       # mask values other than 1
    assert fx["long_masks"].shape == (9, 40, 330) and seen_wrap             # distances pass 255
    # inside a structure the bytes run 0, 255, 254, ...: the uint8 wrap of -(d - 1)
    inside = fx["long_maps"][2][fx["long_masks"][2] != 0]
    assert {0.0, 1.0, 254 / 255.0} <= set(inside.tolist())


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 7), (12, 19)])
def test_the_separable_oracle_equals_brute_force(shape):
    planes = pattern_planes(shape)
    a, b = oracle(planes), oracle(planes, separable_d2_to)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_compute_distance_map_through_the_emulator(emu):
    m = np.stack([pattern_planes((5, 7))[:9], make_masks((5, 7), 3) * 5])
    d2f, d2b, ref = oracle(m)
    t = torch.from_numpy(m)
    out = DU.compute_distance_map(t)
    assert out.shape == (2, 9, 5, 7) and out.dtype == torch.float32 and np.array_equal(out.numpy(), ref.astype(np.float32))
    out3, a, b = DU.compute_distance_map(t[1], return_d2=True)
    assert out3.shape == (9, 5, 7) and torch.equal(out3, out[1]) and a.dtype == torch.int32 and b.dtype == torch.int32
    assert np.array_equal(a.numpy(), d2f[1]) and np.array_equal(b.numpy(), d2b[1])
    assert torch.equal(DU.compute_distance_map(t != 0), out)                # bool masks
    assert torch.equal(DU.compute_distance_map(t.transpose(2, 3)), DU.compute_distance_map(t.transpose(2, 3).contiguous()))
    s = DU.compute_distance_map(t, signed=True)
    assert np.array_equal(s.numpy(), signed_map(m, d2f, d2b).astype(np.float32)) and (s < 0).any()
    for bad in (t.float(), t[0, 0], torch.zeros(9, 0, 4, dtype=torch.uint8), torch.zeros(1, 2, 1025, dtype=torch.uint8)):
        with pytest.raises((ValueError, nat.NativeError)):
            DU.compute_distance_map(bad)


def test_a_cpu_tensor_is_refused():
    with pytest.raises(nat.NativeError):
        DU.compute_distance_map(torch.zeros(9, 8, 8, dtype=torch.uint8))


def test_the_library_validates_before_any_launch():
    """ctseg_distmap2d_batch itself; no device is touched: every case fails validation"""
    L = nat.lib()
    err = L.ctseg_last_error

    def call(masks=4096, P=9, H=8, W=8, mode=0, table=8192, ws=16384, ws_bytes=None, out=32768, d2f=None, d2b=None):
        return L.ctseg_distmap2d_batch(masks, P, H, W, mode, table, ws, 4 * P * H * W if ws_bytes is None else ws_bytes, out, d2f, d2b, None)
    for kw in (dict(masks=None), dict(table=None), dict(ws=None), dict(out=None)):
        assert call(**kw) < 0 and b"null pointer" in err()
    for kw in (dict(P=0), dict(H=0), dict(W=0), dict(P=-1)):
        assert call(**kw) < 0 and b">= 1" in err()
    assert call(H=1025) < 0 and b"sides up to 1024" in err()
    assert call(W=1025) < 0 and b"sides up to 1024" in err()
    assert call(mode=2) < 0 and b"mode 2" in err()
    assert call(mode=-1) < 0 and b"mode" in err()
    assert call(ws_bytes=4 * 9 * 64 - 1) < 0 and b"workspace" in err()
    assert call(out=32770) < 0 and b"unaligned" in err()


def _pipes():
    return (BatchPipeline2D(WINDOWS3, "crop", (8, 8), MEAN3, STD3), BatchPipeline2D(WINDOWS3, "resize", (8, 8), MEAN3, STD3),
            WarpPipeline2D(WINDOWS3, (8, 8), MEAN3, STD3, warps=[GridDistortion(3)]))


def test_enhanced_dataset_returns_the_maps_of_the_transformed_masks(emu, tmp_path):
    _write_npz(tmp_path, "train", 5, 3, bool_masks=True)
    for pipe in _pipes():
        ds = DS.get_miccai_2d("train", transform=pipe, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu", generator=np.random.default_rng(4))
        assert isinstance(ds, DS.EnhancedMiccaiDataset2D) and isinstance(ds, DS.MiccaiDataset2D)
        images, masks, ind, maps = ds.batch([4, 0, 2])
        assert images.shape == (3, 3, 8, 8) and masks.shape == (3, 9, 8, 8) and masks.dtype == torch.uint8 and ind.shape == (3, 9)
        assert maps.shape == (3, 9, 8, 8) and maps.dtype == torch.float32
        assert np.array_equal(maps.numpy(), oracle(masks.numpy())[2].astype(np.float32)) and maps.any()
        item = ds[1]
        assert len(item) == 4 and item[0].shape == (3, 8, 8) and item[1].shape == (9, 8, 8) and item[2].shape == (9,)
        assert np.array_equal(item[3].numpy(), oracle(item[1].numpy())[2].astype(np.float32))
    signed = DS.EnhancedMiccaiDataset2D(str(tmp_path / "miccai_2d" / "train"), transform=_pipes()[1], device="cpu", signed=True)
    _, masks, _, maps = signed.batch([0, 1])
    assert np.array_equal(maps.numpy(), signed_map(masks.numpy(), *oracle(masks.numpy())[:2]).astype(np.float32))
    raw = DS.EnhancedMiccaiDataset2D(str(tmp_path / "miccai_2d" / "train"), transform=None, device="cpu")
    image, m, ind, maps = raw[3]
    assert maps.shape == m.shape and np.array_equal(maps.numpy(), oracle(m.numpy())[2].astype(np.float32))


def test_enhanced_dataset_with_a_squashing_pipeline_keeps_the_label_map_and_its_stashes(emu, tmp_path):
    _write_npz(tmp_path, "train", 4, 7, bool_masks=False)
    params = [(2, 1, 1, 0), (0, 3, 2, 1), (4, 4, 3, 1)]
    for pipe, p in ((_pipes()[0], params), (_pipes()[1], None),
                    (_pipes()[2], {"crop": params, "kind": [2, 0, 2], "xsteps": 1 + np.linspace(-0.2, 0.2, 12).reshape(3, 4),
                                   "ysteps": 1 + np.linspace(0.2, -0.2, 12).reshape(3, 4)})):
        nine = DS.get_miccai_2d("train", transform=pipe, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu").batch([3, 0, 1], params=p)
        sq = pipe.squashing()
        plain = DS.get_miccai_2d("train", transform=sq, root=str(tmp_path), device="cpu").batch([3, 0, 1], params=p)
        images, labels, ind, maps = DS.get_miccai_2d("train", transform=sq, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu").batch([3, 0, 1], params=p)
        # the maps are those of the nine unsquashed masks (structures overlap: labels alone would not give them back)
        assert torch.equal(maps, nine[3]) and np.array_equal(maps.numpy(), oracle(nine[1].numpy())[2].astype(np.float32))
        relabelled = np.stack([(labels.numpy() == k + 1) for k in range(9)], axis=1).astype(np.uint8)
        assert not np.array_equal(relabelled, nine[1].numpy())
        # the label map and its stashes are those of the plain dataset
        assert labels.shape == (3, 8, 8) and torch.equal(labels, plain[1]) and torch.equal(images, plain[0]) and torch.equal(ind, plain[2])
        assert torch.equal(labels._ctseg_present, plain[1]._ctseg_present) and len(labels._ctseg_labels) == 2
        assert torch.equal(labels._ctseg_labels[0], plain[1]._ctseg_labels[0]) and torch.equal(labels._ctseg_labels[1], plain[1]._ctseg_labels[1])
        assert torch.equal(labels._ctseg_masks, nine[1]) and not hasattr(plain[1], "_ctseg_masks")


def test_enhanced_false_is_unchanged(emu, tmp_path):
    _write_npz(tmp_path, "train", 4, 9, bool_masks=False)
    params = [(2, 1, 1, 0), (0, 3, 2, 1)]
    pipe = _pipes()[0]
    ds = DS.get_miccai_2d("train", transform=pipe, root=str(tmp_path), device="cpu")
    assert type(ds) is DS.MiccaiDataset2D
    out = ds.batch([1, 2], params=params)
    direct = pipe(ds.store, [1, 2], params=params)
    assert len(out) == 3 and torch.equal(out[0], direct[0]) and torch.equal(out[1], direct[1])
    assert torch.equal(out[2], ds.mask_indicator[[1, 2]]) and not hasattr(out[1], "_ctseg_masks") and emu.distmap2d_calls == 0
    assert len(ds[0]) == 3
    enhanced = DS.get_miccai_2d("train", transform=pipe, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu").batch([1, 2], params=params)
    assert all(torch.equal(a, b) for a, b in zip(out, enhanced[:3])) and emu.distmap2d_calls == 1


def test_data_modules_yield_four_tuples(emu, tmp_path, monkeypatch):
    for split, n, seed in (("train", 7, 10), ("valid", 3, 20), ("test", 2, 30)):
        _write_npz(tmp_path, split, n, seed, bool_masks=False)
    crop, resize, _ = _pipes()
    monkeypatch.setitem(DM.DEGREE, 2, {"train": crop, "test": resize})
    dm = DM.MiccaiDataModule2D(3, transform_degree=2, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu", generator=np.random.default_rng(5))
    dm.setup(None)
    assert all(isinstance(d, DS.EnhancedMiccaiDataset2D) for d in (dm.train_dataset, dm.val_dataset, dm.test_dataset))
    for loader, sizes in ((dm.train_dataloader(), [3, 3, 1]), (dm.val_dataloader(), [3]), (dm.test_dataloader(), [2])):
        batches = list(loader)
        assert [len(b) for b in batches] == [4] * len(sizes) and [b[3].shape[0] for b in batches] == sizes
        for images, masks, ind, maps in batches:
            assert maps.shape == masks.shape == (images.shape[0], 9, 8, 8) and maps.dtype == torch.float32
            assert np.array_equal(maps.numpy(), oracle(masks.numpy())[2].astype(np.float32))
    # a batch that spans two datasets: one launch per dataset, the parts concatenated
    full = DM.FullMiccaiDataModule2D(4, transform_degree=2, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu", generator=np.random.default_rng(6))
    full.setup("fit")
    loader = full.train_dataloader()
    order = loader.order()
    loader.order = lambda: order
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [4, 4, 2] and all(len(b) == 4 for b in batches)
    spans = [bool((order[i:i + 4] < 7).any() and (order[i:i + 4] >= 7).any()) for i in range(0, 10, 4)]
    assert any(spans)
    for images, masks, ind, maps in batches:
        assert maps.shape == masks.shape and np.array_equal(maps.numpy(), oracle(masks.numpy())[2].astype(np.float32))
        assert masks._ctseg_present.shape == (images.shape[0], 9)
    # squashed parts of two datasets: labels, stashes and maps all arrive
    monkeypatch.setitem(DM.DEGREE, 2, {"train": crop.squashing(), "test": resize.squashing()})
    full = DM.FullMiccaiDataModule2D(4, transform_degree=2, enhanced=True, device_maps=True, root=str(tmp_path), device="cpu", generator=np.random.default_rng(6))
    full.setup("fit")
    for images, labels, ind, maps in full.train_dataloader():
        assert labels.shape == (images.shape[0], 8, 8) and maps.shape == (images.shape[0], 9, 8, 8) and len(labels._ctseg_labels) == 2
    plain = DM.MiccaiDataModule2D(3, transform_degree=2, root=str(tmp_path), device="cpu", generator=np.random.default_rng(5))
    plain.setup("fit")
    assert all(len(b) == 3 for b in plain.train_dataloader())


def test_enhanced_without_the_opt_in_keeps_the_old_refusal(tmp_path):
    _write_npz(tmp_path, "train", 2, 3, bool_masks=False)
    _write_npz(tmp_path, "valid", 2, 4, bool_masks=False)
    with pytest.raises(NotImplementedError, match="device_maps=True"):
        DS.get_miccai_2d("train", transform=_pipes()[0], enhanced=True, root=str(tmp_path), device="cpu")
    dm = DM.MiccaiDataModule2D(2, transform_degree=2, enhanced=True, root=str(tmp_path), device="cpu")
    with pytest.raises(NotImplementedError, match="device_maps=True"):
        dm.setup("fit")
    assert type(DS.get_miccai_2d("train", transform=_pipes()[0], device_maps=True, root=str(tmp_path), device="cpu")) is DS.MiccaiDataset2D


def test_the_trainers_still_refuse_the_boundary_loss():
    from capstone_amd.models.losses import MultipleLossWrapper
    with pytest.raises(NotImplementedError):
        MultipleLossWrapper(["Focal", "Dice", "Boundary"])


# ---- GPU tests: the kernel against the oracle, bit for bit -------------------------------------------------------------------
GPU_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (33, 65), (40, 330)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=[f"{h}x{w}" for h, w in GPU_SHAPES])
def test_gpu_patterns_are_bit_exact(shape):
    planes = pattern_planes(shape)
    check_reference_mode(planes)
    got = run_gpu(planes)[0]
    empty, full = 7, 8                                                      # in the same launch, both all zero
    assert not planes[empty].any() and (planes[full] != 0).all() and not got[empty].any() and not got[full].any()
    if shape == (40, 330):
        assert oracle(planes)[0].max() > 255 * 255                          # the byte wraps


@pytest.mark.gpu
def test_gpu_nine_planes_of_three_samples_in_one_launch():
    m = np.stack([np.stack([discs((64, 64), 10 * b + c, n=1 + c % 3, value=1 + c) for c in range(9)]) for b in range(3)])
    m[1, 4] = 0                                                             # an absent class
    m[2, 1] = m[2, 5] * (discs((64, 64), 99) > 0)                           # a structure inside another
    assert m.shape == (3, 9, 64, 64)
    check_reference_mode(m)


@pytest.mark.gpu
def test_gpu_256_planes_against_the_separable_oracle():
    m = np.stack([discs((256, 256), 40 + c, n=1 + c % 4) for c in range(9)])
    m[3] = 0
    m[6] = 0
    m[6, 255, 0] = 1                                                        # every outward search runs the whole row
    m[7, 100:140, 60:200] |= 1
    check_reference_mode(m, separable_d2_to)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(33, 65), (40, 330)], ids=["33x65", "40x330"])
def test_gpu_signed_maps(shape):
    """3 fp32 ulp of the value: one square root, one subtraction and one division, each at most 1 ulp; a perfect square has an
    exact root, an exact subtraction and a correctly rounded division: equality with the float32 of the float64 value"""
    planes = pattern_planes(shape)
    got, d2f, d2b = run_gpu(planes, signed=True)
    ref_f, ref_b, _ = oracle(planes)
    assert np.array_equal(d2f, ref_f) and np.array_equal(d2b, ref_b)
    ref = signed_map(planes, ref_f, ref_b)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 3 * ulp).all(), float((err / ulp).max())
    used = np.where(planes != 0, ref_b, ref_f)
    square = isqrt(np.maximum(used, 0)) ** 2 == used
    assert square.any() and not square.all() and np.array_equal(got[square], ref.astype(np.float32)[square])
    assert (got < 0).any() and not got[7].any() and not got[8].any()


def _gpu_store(shapes, seed):
    raws = [make_raw(s, np.int16, seed + i) for i, s in enumerate(shapes)]
    masks = []
    for i, s in enumerate(shapes):                                          # overlapping discs; one absent class
        m = np.stack([discs(s, seed + 10 * i + c, n=2, value=1) for c in range(9)])
        m[4] = 0
        masks.append(m)
    return raws, masks


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["crop", "warped"])
def test_gpu_enhanced_dataset_through_the_presets(preset, tmp_path):
    shapes = [(262, 270), (300, 257)]
    raws, masks = _gpu_store(shapes, 5)
    d = tmp_path / "miccai_2d" / "train"
    d.mkdir(parents=True)
    for i, (r, m) in enumerate(zip(raws, masks)):
        np.savez(d / f"case{i:03d}.npz", image=r[None], masks=m, mask_indicator=np.ones(9))
    pipe = predefined.windowed_degree_2["train"] if preset == "crop" else predefined.warped["windowed_degree_4"]["train"]
    assert isinstance(pipe, WarpPipeline2D) == (preset == "warped") and pipe.size == (256, 256)
    ds = DS.get_miccai_2d("train", transform=pipe, enhanced=True, device_maps=True, root=str(tmp_path), device=DEV, generator=np.random.default_rng(3))
    if preset == "warped":                                                  # one elastic and one grid sample
        params = pipe.draw_params(ds.store.table[[1, 0], 2:4], np.random.default_rng(8))
        params["kind"][:] = [1, 2]
        params["matrix"][0] = [[1.02, 0.03, -2.0], [-0.02, 0.98, 3.0]]
        params["seed"][0] = 11
    else:
        params = [(20, 1, 1, 1), (3, 10, 2, 0)]
    images, m9, ind, maps = ds.batch([1, 0], params=params)
    torch.cuda.synchronize()
    assert images.shape == (2, 3, 256, 256) and m9.shape == (2, 9, 256, 256) and maps.shape == (2, 9, 256, 256) and maps.dtype == torch.float32
    ref = oracle(m9.cpu().numpy()[:, :6], separable_d2_to)[2]               # six planes per sample (one of them absent) keep this quick
    assert np.array_equal(maps.cpu().numpy()[:, :6], ref.astype(np.float32)) and m9[:, :6].any() and bool(maps.any())
    # the squashing side of the same preset: the labels of the same launch, the maps of the nine masks
    sq = DS.EnhancedMiccaiDataset2D(str(d), transform=pipe.squashing(), device=DEV)
    images_sq, labels, _, maps_sq = sq.batch([1, 0], params=params)
    assert labels.shape == (2, 256, 256) and torch.equal(maps_sq, maps) and torch.equal(labels._ctseg_masks, m9) and torch.equal(images_sq, images)
