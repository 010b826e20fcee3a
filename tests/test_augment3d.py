"""3-D augmentation on the device: ctseg_augment3d_to_hwd, capstone_amd.volumetric.transforms (augment3d_to_hwd, Augment3D,
InstancePipeline3D(augment=...), augmented_degree_1), MiccaiDataset3D(generator=...) and volumetric.data_module.MiccaiDataModule3D.

Held to the affine ``oracle`` of tests/resample_oracles.py; every comparison but one is ``array_equal``.  CPU tests route the entry
through an emulator that IS the oracle; GPU tests hold the kernel to the oracle.

The kernel's tile is the resize kernel's: one h, 64 along w, 32 along d.  Output (D', H', W') = (33, 6, 70) is one full tile plus
a ragged remainder on both tiled axes, (32, 4, 64) is exact tiles, (9, 33, 33) has the square h-w plane a quarter turn needs.
The sources resize up, down and mixed.  Every output has fewer than 1e5 voxels.
"""
import ctypes

import numpy as np
import pytest
import torch

from abi_emulator import Emulator, emulated
from capstone_amd import _native as nat
from capstone_amd.data.utils import compute_distance_map
from capstone_amd.volumetric import datasets as DS
from capstone_amd.volumetric import transforms as T
from feature_emulators import Augment3dEntries, Distmap3dEntries
from helpers import as_numpy
from resample_oracles import (GENERAL, K, SHAPES, SWAPPED, assert_same, cached_oracle, flip_matrix, general_matrix, identity, inputs, oracle,
                              quarter_turn, write_instances)
from resample_oracles import inputs_on_device as on_device

DEV = "cuda:0"


class E(Augment3dEntries, Distmap3dEntries, Emulator):
    pass


@pytest.fixture()
def emu():
    with emulated(E(), plan_run=False) as e:
        yield e


@pytest.fixture()
def calls(emu):
    """the names of the entries called, in order (a spy on nat.call, on top of the emulator)"""
    seen, inner = [], nat.call

    def spy(name, *args):
        seen.append(name)
        return inner(name, *args)
    nat.call = spy
    yield seen
    nat.call = inner


def resize_reference(shape, code, size, window=0, lo=0.0, hi=1.0):
    """the plain nearest resize by the ABI emulator's own, separate restatement"""
    image, masks = inputs(shape, code)
    n = int(np.prod(size))
    img, m, lab, hist = np.empty(n, np.float32), np.empty(K * n, np.uint8), np.empty(n, np.uint8), np.zeros(K + 1, np.int64)
    Emulator().resize3d_to_hwd(image.ctypes.data, code, masks.ctypes.data, K, *shape, *size, window, lo, hi, img.ctypes.data,
                               m.ctypes.data, lab.ctypes.data, hist.ctypes.data)
    Ho, Wo, Do = size[1], size[2], size[0]
    return img.reshape(Ho, Wo, Do), m.reshape(K, Ho, Wo, Do), lab.reshape(Ho, Wo, Do), hist


# ---- CPU: the oracle itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,size", SHAPES)
@pytest.mark.parametrize("interp", [0, 1])
def test_oracle_identity_is_the_nearest_resize(shape, size, interp):
    for code, window in ((nat.I16, 0), (nat.F32, 2), (nat.U8, 1)):
        want = resize_reference(shape, code, size, window, 40.0, 200.0)
        got = oracle(*inputs(shape, code), size, identity(), interp=interp, window=window, lo=40.0, hi=200.0)[:4]
        assert_same(got, want)


@pytest.mark.parametrize("shape,size", SHAPES)
@pytest.mark.parametrize("interp", [0, 1])
def test_oracle_integer_matrices_are_flip_and_rot90(shape, size, interp):
    want = resize_reference(shape, nat.I16, size)
    image, masks = inputs(shape, nat.I16)
    cases = [(flip_matrix(a, size), lambda x, ax, a=a: np.flip(x, ax[a])) for a in range(3)]
    if size[1] == size[2]:
        cases.append((quarter_turn(size), lambda x, ax: np.rot90(x, 1, axes=(ax[1], ax[2]))))
    for A, turn in cases:
        for border in (0, 1):
            img, m, lab, hist, outside = oracle(image, masks, size, A, interp=interp, border=border, cval=-7.0)
            assert outside == 0.0
            # outputs are (H', W', D'): the d, h, w axes of the volume are axes 2, 0, 1 (masks: one more in front)
            assert np.array_equal(img, turn(want[0], (2, 0, 1))) and np.array_equal(lab, turn(want[2], (2, 0, 1)))
            assert np.array_equal(m, turn(want[1], (3, 1, 2))) and np.array_equal(hist, want[3])


def test_oracle_general_matrix_samples_both_sides_of_the_border():
    shape, size = SHAPES[1]
    outside = cached_oracle(shape, nat.I16, size, general_matrix(size), interp=0, border=0, cval=-1000.0)[4]
    assert 0.05 < outside < 0.5, outside


# ---- CPU: Augment3D ----------------------------------------------------------------------------------------------------------
def test_matrix_identity_flip_and_composition_order():
    ident = T.Augment3D.identity_params()
    for size in ((33, 6, 70), (9, 33, 33), (96, 256, 256)):
        A = T.Augment3D.matrix(size, ident)
        assert A.dtype == np.float32 and A.shape == (3, 4) and np.array_equal(A, identity())
        A = T.Augment3D.matrix(size, dict(ident, flips=(False, False, True)))
        assert np.array_equal(A, flip_matrix(2, size))
        A = T.Augment3D.matrix(size, dict(ident, flips=(True, True, False)))
        assert np.array_equal(A, flip_matrix(0, size) @ np.vstack([flip_matrix(1, size), [0, 0, 0, 1]]))
    # by hand, on a 5 x 5 x 5 grid (c = 2): quarter turns about d and about w, zoom (1, 2, 4), w mirror, shift (1, 2, 3)
    #   diag(1/s) . F = diag(1, .5, -.25);  R_d . that = [[1,0,0],[0,0,.25],[0,.5,0]];  R_w . that = [[0,0,-.25],[1,0,0],[0,.5,0]]
    #   L c = (-.5, 2, 1);  offset = c - L c + t = (3.5, 2, 4)
    p = dict(ident, angles=(np.pi / 2, 0.0, np.pi / 2), scales=(1.0, 2.0, 4.0), flips=(False, False, True), shifts=(1.0, 2.0, 3.0))
    want = np.array([[0, 0, -0.25, 3.5], [1, 0, 0, 2], [0, 0.5, 0, 4]], dtype=np.float32)
    got = T.Augment3D.matrix((5, 5, 5), p)
    assert np.abs(got - want).max() < 1e-6, got
    # the turn about h alone: R_h = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    got = T.Augment3D.matrix((5, 5, 5), dict(ident, angles=(0.0, np.pi / 2, 0.0)))
    assert np.abs(got - np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 4]], dtype=np.float32)).max() < 1e-6, got


def test_channel_src_swaps_the_pairs_only_under_the_w_flip():
    aug = T.Augment3D()
    ident = T.Augment3D.identity_params()
    for flips in ((False, False, False), (True, False, False), (False, True, False), (True, True, False)):
        assert aug.channel_src(dict(ident, flips=flips), K) == list(range(K))
    for flips in ((False, False, True), (True, True, True)):
        assert aug.channel_src(dict(ident, flips=flips), K) == SWAPPED
    assert T.Augment3D(swap_pairs=((0, 1),)).channel_src(dict(ident, flips=(False, False, True)), 3) == [1, 0, 2]


def test_draw_is_reproducible_and_inside_the_ranges():
    aug = T.Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), translate=(2, 8, 8), flip_prob=(0, 0, 0.5), gain=(0.9, 1.1),
                      bias=(-20.0, 30.0))
    a = [aug.draw(np.random.default_rng(11)) for _ in range(2)]
    assert a[0] == a[1]
    g = np.random.default_rng(5)
    draws = [aug.draw(g) for _ in range(200)]
    assert draws[0] != draws[1]
    for p in draws:
        assert all(abs(v) <= h for v, h in zip(p["angles"], (0.26, 0.05, 0.05)))
        assert all(0.9 <= v <= 1.1 for v in p["scales"]) and all(abs(v) <= h for v, h in zip(p["shifts"], (2, 8, 8)))
        assert p["flips"][:2] == (False, False) and 0.9 <= p["gain"] <= 1.1 and -20.0 <= p["bias"] <= 30.0
    assert 60 < sum(p["flips"][2] for p in draws) < 140
    assert len({p["angles"][0] for p in draws}) == 200 and len({p["scales"] for p in draws}) == 200
    per_axis = T.Augment3D(scale=((1, 1), (0.5, 0.6), (2, 3))).draw(g)["scales"]
    assert per_axis[0] == 1.0 and 0.5 <= per_axis[1] <= 0.6 and 2 <= per_axis[2] <= 3
    off = T.Augment3D(rotate=(1, 1, 1), p=0.0).draw(g)
    assert off == T.Augment3D.identity_params()
    preset = T.augmented_degree_1["train"].augment.draw(g)
    assert (preset["gain"], preset["bias"]) == (1.0, 0.0) and T.augmented_degree_1["test"].augment is None


# ---- CPU: pipeline, dataset, data module (emulated) ----------------------------------------------------------------------------
def test_pipeline_calls_one_entry(calls):
    shape, size = SHAPES[1]
    image, masks = (torch.from_numpy(np.array(a)) for a in inputs(shape))
    plain = T.InstancePipeline3D(size)(image=image, masks=masks)
    assert calls == ["ctseg_resize3d_to_hwd"] and "channel_src" not in plain and "params" not in plain
    del calls[:]
    aug = T.Augment3D(rotate=(0.26, 0.05, 0.05), flip_prob=(0, 0, 1.0))
    out = T.InstancePipeline3D(size, squash=True, augment=aug)(image=image, masks=masks, generator=np.random.default_rng(3))
    assert calls == ["ctseg_augment3d_to_hwd"]
    assert out["channel_src"] == SWAPPED and out["params"] == aug.draw(np.random.default_rng(3))
    want = oracle(*inputs(shape), size, aug.matrix(size, out["params"]), interp=1, mask_src=SWAPPED)
    assert np.array_equal(out["image"][0].numpy(), want[0]) and np.array_equal(out["masks"].numpy(), want[2])
    assert np.array_equal(out["hist"].numpy(), want[3])
    # explicit parameters: identity parameters are the plain resize
    same = T.InstancePipeline3D(size, augment=aug)(image=image, masks=masks, params=T.Augment3D.identity_params())
    assert torch.equal(same["image"], plain["image"]) and torch.equal(same["masks"], plain["masks"])
    assert same["channel_src"] == list(range(K))


def test_dataset_permutes_the_indicator_with_the_channels(emu, tmp_path):
    shape, size = SHAPES[1]
    write_instances(tmp_path, shape, ("train",), 1)
    mirror = T.InstancePipeline3D(size, augment=T.Augment3D(flip_prob=(0, 0, 1.0)))
    ds = DS.get_miccai_3d("train", mirror, root=str(tmp_path), device="cpu", generator=np.random.default_rng(0))
    image, masks, ind = ds[0]
    assert ind.tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 0] and ind.dtype == torch.float64
    plain = DS.get_miccai_3d("train", T.InstancePipeline3D(size), root=str(tmp_path), device="cpu")[0]
    assert plain[2].tolist() == [1, 1, 0, 1, 0, 1, 1, 0, 1]
    # (H', W', D') storage: the w mirror is a flip of axis 1; channel 3 now holds what was channel 4
    assert torch.equal(image, plain[0].flip(2)) and torch.equal(masks, plain[1][SWAPPED].flip(2))
    assert not torch.equal(plain[1][3], plain[1][4])
    never = T.InstancePipeline3D(size, augment=T.Augment3D(flip_prob=(1.0, 0, 0)))
    assert DS.MiccaiDataset3D(str(tmp_path / "miccai_3d" / "train"), never, device="cpu")[0][2].tolist() == plain[2].tolist()


def test_data_module_degrees_batches_maps_and_seed(emu, tmp_path):
    from capstone_amd.volumetric import MiccaiDataModule3D
    from capstone_amd.volumetric import data_module as DM
    assert DM.MiccaiDataModule3D is MiccaiDataModule3D
    assert DM.DEGREE[0] is T.windowed_degree_0 and DM.DEGREE[1] is T.augmented_degree_1
    with pytest.raises(AssertionError):
        MiccaiDataModule3D(2, transform_degree=2)
    shape, size = (13, 40, 37), (8, 16, 12)
    write_instances(tmp_path, shape)
    Ho, Wo, Do = size[1], size[2], size[0]

    def batches(loader):
        return [tuple(t.clone() for t in b) for b in loader]
    dm0 = MiccaiDataModule3D(2, transform_degree=0, root=str(tmp_path), device="cpu", size=size)
    dm0.setup()
    assert dm0.train_dataset.transform.augment is None
    plain = batches(dm0.val_dataloader())
    assert [b[0].shape[0] for b in plain] == [2, 1] and len(dm0.val_dataloader()) == 2
    assert plain[0][0].shape == (2, 1, Ho, Wo, Do) and plain[0][1].shape == (2, K, Ho, Wo, Do) and plain[0][2].shape == (2, K)
    assert all(len(b) == 3 for b in plain)

    def degree1(seed, **kw):
        dm = MiccaiDataModule3D(2, transform_degree=1, root=str(tmp_path), device="cpu", seed=seed, size=size, **kw)
        dm.setup()
        return dm
    dm1 = degree1(7)
    assert dm1.train_dataset.transform.augment is T.augmented_degree_1["train"].augment and dm1.val_dataset.transform.augment is None
    first = batches(dm1.train_dataloader())
    again = batches(degree1(7).train_dataloader())
    other = batches(degree1(8).train_dataloader())
    assert all(torch.equal(x, y) for a, b in zip(first, again) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for a, b in zip(first, other) for x, y in zip(a, b))
    assert first[0][0].shape == (2, 1, Ho, Wo, Do) and first[0][1].shape == (2, K, Ho, Wo, Do) and first[1][0].shape[0] == 1
    for b in first:          # the train indicator is one fixed vector: either as written or with the pairs swapped
        for row in b[2].tolist():
            assert row in ([1, 1, 0, 1, 0, 1, 1, 0, 1], [1, 1, 0, 0, 1, 1, 1, 1, 0])
    # the sides that do not augment are the degree-0 batches
    for a, b in zip(batches(dm1.val_dataloader()) + batches(dm1.test_dataloader()), plain + batches(dm0.test_dataloader())):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the fourth batch element: the distance maps of the augmented masks
    dmm = degree1(7, dist_maps=True)
    with_maps = batches(dmm.train_dataloader())
    assert all(len(b) == 4 for b in with_maps) and with_maps[0][3].shape == (2, K, Ho, Wo, Do) and with_maps[0][3].dtype == torch.float32
    for b, a in zip(with_maps, first):
        assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[1]) and torch.equal(b[2], a[2])
        assert torch.equal(b[3], compute_distance_map(b[1], spatial_dims=3))
    assert bool((with_maps[0][3] != 0).any())


# ---- CPU: the entry's own validation (runs before any launch) ------------------------------------------------------------------
def test_entry_rejects_bad_arguments_without_a_device():
    L = nat.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def call(matrix=None, interp=1, border=0, mask_src=None, gain=1.0, bias=0.0, Kn=K):
        A = (ctypes.c_float * 12)(*(identity().reshape(-1).tolist() if matrix is None else matrix))
        held = (ctypes.c_int32 * Kn)(*(mask_src if mask_src is not None else range(Kn)))
        src = None if mask_src is None else ctypes.addressof(held)
        rc = L.ctseg_augment3d_to_hwd(p, nat.F32, p, Kn, 2, 2, 2, 2, 2, 2, ctypes.addressof(A), interp, border, 0.0, src, 0, 0.0, 1.0,
                                      gain, bias, p, p, p, None, None)
        return rc, L.ctseg_last_error().decode()
    for bad in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 7, 11):
            A = identity().reshape(-1).tolist()
            A[at] = bad
            rc, msg = call(matrix=A)
            assert rc < 0 and "matrix" in msg and "finite" in msg, msg
    for src in ([0, 1, 2, 3, 4, 5, 6, 7, 7], [0, 1, 2, 3, 4, 5, 6, 7, 9], [-1, 1, 2, 3, 4, 5, 6, 7, 8]):
        rc, msg = call(mask_src=src)
        assert rc < 0 and "permutation" in msg, msg
    for kw, word in (({"interp": 2}, "interp"), ({"interp": -1}, "interp"), ({"border": 2}, "border"), ({"border": -1}, "border"),
                     ({"gain": float("nan")}, "gain"), ({"bias": float("inf")}, "bias")):
        rc, msg = call(**kw)
        assert rc < 0 and word in msg, msg
    rc, msg = call(Kn=16, mask_src=list(range(16)))
    assert rc < 0 and "K <= 15" in msg, msg


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", SHAPES)
@pytest.mark.parametrize("code", [nat.F32, nat.I16, nat.U8])
def test_gpu_identity_equals_the_resize_kernel(shape, size, code):
    image, masks = on_device(shape, code)
    for window in (None, (160, 120, False), (160, 120, True)):
        want = as_numpy(T.resize3d_to_hwd(image, masks, size, window, want_masks=True, want_labels=True))
        for interp in (0, 1):
            for border in ("constant", "edge"):
                got = as_numpy(T.augment3d_to_hwd(image, masks, size, identity(), interp, border, cval=-3.0, window=window,
                                                  want_masks=True, want_labels=True))
                assert_same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", SHAPES)
def test_gpu_flips_and_quarter_turn_equal_torch_flip_and_rot90(shape, size):
    image, masks = on_device(shape, nat.I16)
    img, m, lab, hist = T.resize3d_to_hwd(image, masks, size, want_masks=True, want_labels=True)
    axis = (2, 0, 1)          # the d, h, w axes of the (H', W', D') outputs
    cases = [(flip_matrix(a, size), lambda x, lead, a=a: torch.flip(x, [lead + axis[a]])) for a in range(3)]
    if size[1] == size[2]:
        cases.append((quarter_turn(size), lambda x, lead: torch.rot90(x, 1, (lead, lead + 1))))
    for A, turn in cases:
        for interp in (0, 1):
            got = T.augment3d_to_hwd(image, masks, size, A, interp, "constant", cval=-7.0, want_masks=True, want_labels=True)
            assert torch.equal(got[0], turn(img, 0)) and torch.equal(got[1], turn(m, 1)) and torch.equal(got[2], turn(lab, 0))
            assert torch.equal(got[3], hist)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", SHAPES)
@pytest.mark.parametrize("interp", [0, 1])
def test_gpu_general_matrix_equals_the_oracle(shape, size, interp):
    image, masks = on_device(shape, nat.I16)
    A = general_matrix(size)
    if (shape, size) == SHAPES[1]:
        outside = cached_oracle(shape, nat.I16, size, A, interp=0, border=0, cval=-1000.0)[4]
        assert 0.05 < outside < 0.5, outside
    for border, cval in ((0, -1000.0), (1, 0.0)):
        for src in (None, SWAPPED):
            for window, lo, hi, gain, bias in ((None, 0.0, 1.0, 1.0, 0.0), ((2000, 0, True), -1000.0, 1000.0, 1.07, -0.02),
                                               (None, 0.0, 1.0, 0.93, 11.5)):
                want = cached_oracle(shape, nat.I16, size, A, interp=interp, border=border, cval=cval, mask_src=src,
                                     window=2 if window else 0, lo=lo, hi=hi, gain=gain, bias=bias)
                got = as_numpy(T.augment3d_to_hwd(image, masks, size, A, interp, border, cval, src, window, gain, bias,
                                                  want_masks=True, want_labels=True))
                assert_same(got, want[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", SHAPES)
def test_gpu_trilinear_within_the_derived_bound_of_float64(shape, size):
    """the one comparison with a tolerance: the kernel's float32 trilinear image against the same formula in float64 on the same
    float32 matrix entries.  Bound: six float32 operations per coordinate at magnitudes up to 2 * side, three axes, a slope of at
    most R (the input's value range, cval inside it) per voxel, plus the lerps' own roundings."""
    for code in (nat.I16, nat.F32):
        image, masks = inputs(shape, code)
        A = general_matrix(size)
        R = float(image.max()) - float(image.min())
        assert image.min() <= -1000.0 <= image.max()
        tol = R * (3 * 6 * 2.0 ** -24 * 2 * max(size) + 8 * 2.0 ** -24)
        for border in (0, 1):
            want = oracle(image, None, size, A, interp=1, border=border, cval=-1000.0, dtype=np.float64)[0]
            got = T.augment3d_to_hwd(on_device(shape, code)[0], None, size, A, 1, border, -1000.0)[0].cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"trilinear {shape}->{size} dtype {code} border {border}: max error {err:.3e}, bound {tol:.3e}")
            assert err <= tol, (err, tol)


@pytest.mark.gpu
def test_gpu_pipeline_with_explicit_params():
    shape, size = SHAPES[1]
    image, masks = on_device(shape, nat.I16)
    aug = T.Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), translate=(2, 8, 8), flip_prob=(0, 0, 0.5))
    params = dict(GENERAL, flips=(False, False, True))
    pipe = T.InstancePipeline3D(size, squash=True, dist_maps=True, augment=aug)
    out = pipe(image=image, masks=masks, params=params)
    assert out["channel_src"] == SWAPPED and out["params"] == params
    img, m, lab, hist = T.augment3d_to_hwd(image, masks, size, aug.matrix(size, params), 1, "constant", 0.0, SWAPPED,
                                           want_masks=True, want_labels=True)
    assert torch.equal(out["image"][0], img) and torch.equal(out["masks"], lab) and torch.equal(out["hist"], hist)
    assert torch.equal(out["dist_maps"], compute_distance_map(m, spatial_dims=3))
    want = oracle(*inputs(shape), size, aug.matrix(size, params), interp=1, mask_src=SWAPPED)
    assert_same(as_numpy((img, m, lab, hist)), want[:4])
    again = pipe(image=image, masks=masks, params=params)
    for key in ("image", "masks", "hist", "dist_maps"):
        assert torch.equal(out[key], again[key])
    nine = T.InstancePipeline3D(size, augment=aug)(image=image, masks=masks, params=params)
    assert torch.equal(nine["masks"], m)


@pytest.mark.gpu
def test_gpu_fit_step_on_a_degree_1_batch(tmp_path):
    from capstone_amd.volumetric import MiccaiDataModule3D
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    write_instances(tmp_path, (13, 40, 37), ("train", "valid"), 2)
    dm = MiccaiDataModule3D(2, transform_degree=1, root=str(tmp_path), device=DEV, seed=3, size=(16, 32, 32))
    dm.setup("fit")
    batch = next(iter(dm.train_dataloader()))
    assert batch[0].shape == (2, 1, 32, 32, 16) and batch[1].shape == (2, K, 32, 32, 16) and batch[0].is_cuda
    torch.manual_seed(0)
    model = BaseUNet3D(filters=[8, 16, 32], loss_fx=["CrossEntropy", "Dice"]).cuda()
    loss = float(model.fit_step(batch))
    assert np.isfinite(loss)
