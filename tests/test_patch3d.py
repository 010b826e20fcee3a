"""Foreground-biased patch sampling: ctseg_patch_centres / ctseg_patch_centres_workspace / ctseg_patch3d_to_hwd,
capstone_amd.volumetric.transforms (patch_centres, patch3d_to_hwd, patch_matrix, PatchSampler3D), datasets.MiccaiPatchDataset3D /
collate_patches_3d, MiccaiDataModule3D(patch_size=...) and BaseUNet3D(val_inferer=...).

Held to tests/patch_oracles.py; every comparison of a kernel's output is ``array_equal``.  The centre pick is integer arithmetic,
the identity crop moves whole voxels, and the general matrix is held to the float32 restatement of "the affine pass with
t' = f32(t + f32(c))", which rounds where the kernel rounds.

Shapes.  The count pass counts blocks of 16384 voxels with 16-byte loads: (5, 37, 70) = 12950 voxels is one ragged block whose
classes start at odd addresses, (9, 40, 50) = 18000 spans two blocks, and (9, 81, 70) = 51030, this file's own, four.  The crop's
tile is one h, 64 along w, 32 along d: patch (33, 7, 70) is a full tile plus a ragged remainder on both tiled axes, (32, 4, 64) is
tile-exact.  Every volume has fewer than 1e5 voxels.
"""
import ctypes

import numpy as np
import pytest
import torch

import patch_oracles as PO
from capstone_amd import STRUCTURES
from capstone_amd import _native as nat
from capstone_amd.volumetric import datasets as DS
from capstone_amd.volumetric import transforms as T
from helpers import as_numpy, on_device
from resample_oracles import K, SWAPPED, assert_same, inputs, write_instances

DEV = "cuda:0"
EDGE = (0, 1, 2 ** 31, 2 ** 32 - 1)
VOLUMES = [(5, 37, 70), (9, 40, 50), (9, 81, 70)]
SRC = (40, 20, 90)                                  # the crop tests' volume


# ---- CPU: the library without a device ---------------------------------------------------------------------------------------
def _err():
    return nat.lib().ctseg_last_error().decode()


def test_patch_centres_rejects_bad_arguments_before_any_launch():
    L = nat.lib()
    draws = (ctypes.c_uint32 * 48)()
    d = ctypes.addressof(draws)
    fake = 1 << 20                                  # never dereferenced: every call below is refused on the host
    need = L.ctseg_patch_centres_workspace(4, 9, 40, 50)

    def call(masks=fake, K_=4, dims=(9, 40, 50), draws_=d, P=2, ws=fake, ws_bytes=need, centres=fake, patch=None):
        return L.ctseg_patch_centres(masks, K_, *dims, draws_, P, 15, patch, ws, ws_bytes, centres, None)
    for kw in (dict(masks=None), dict(draws_=None), dict(ws=None), dict(centres=None)):
        assert call(**kw) < 0 and "null pointer" in _err(), kw
    for P in (0, 17):
        assert call(P=P) < 0 and "patches" in _err()
    assert call(K_=16) < 0 and "masks" in _err()
    assert call(K_=0) < 0 and "masks" in _err()
    assert call(dims=(2048, 1024, 1024)) < 0 and "2^31" in _err()
    assert call(dims=(0, 4, 4)) < 0 and "geometry" in _err()
    assert call(ws_bytes=need - 4) < 0 and "workspace" in _err()
    bad_patch = (ctypes.c_int32 * 3)(4, 0, 4)
    assert call(patch=ctypes.addressof(bad_patch)) < 0 and "patch side" in _err()
    assert L.ctseg_patch_centres_workspace(16, 9, 40, 50) < 0 and L.ctseg_patch_centres_workspace(4, 2048, 1024, 1024) < 0


def test_patch3d_rejects_bad_arguments_before_any_launch():
    L = nat.lib()
    fake = 1 << 20
    ident = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)

    def call(matrix=ctypes.addressof(ident), centre=fake, image=fake, out=fake, dims=(8, 8, 8), interp=0, border=0):
        return L.ctseg_patch3d_to_hwd(image, nat.F32, None, 0, *dims, 4, 4, 4, matrix, centre, interp, border, 0.0, None, 0, 0.0, 1.0,
                                      1.0, 0.0, out, None, None, None, None)
    assert call(centre=None) < 0 and "centre" in _err()
    assert call(matrix=None) < 0 and "matrix" in _err()
    assert call(image=None) < 0 and call(out=None) < 0
    for bad in (float("nan"), float("inf")):
        m = (ctypes.c_float * 12)(*ident)
        m[7] = bad
        assert call(matrix=ctypes.addressof(m)) < 0 and "not finite" in _err()
    assert call(dims=(2048, 1024, 1024)) < 0 and "2^31" in _err()
    assert call(interp=2) < 0 and call(border=2) < 0


def test_workspace_query_is_monotone_and_matches_the_formula():
    L = nat.lib()
    last = 0
    for dims in ((1, 1, 1), (5, 37, 70), (1, 128, 128), (1, 128, 129), (9, 40, 50), (9, 81, 70), (140, 512, 512)):
        for k in (1, 4, 9, 15):
            got = L.ctseg_patch_centres_workspace(k, *dims)
            assert got == PO.workspace_bytes(k, *dims), (k, dims)
        assert got >= last
        last = got
    assert L.ctseg_patch_centres_workspace(1, 1, 128, 128) == 4 * (1 + 16)            # exactly one block
    assert L.ctseg_patch_centres_workspace(1, 1, 128, 129) == 4 * (2 + 16)


# ---- CPU: the sampler's host side --------------------------------------------------------------------------------------------
def _augment(**kw):
    return T.Augment3D(rotate=(0.26, 0.05, 0.05), scale=(0.9, 1.1), flip_prob=(0, 0, 0.5), gain=(0.9, 1.1), **kw)


def test_draw_contract_values_taken_per_patch():
    intensity = T.Intensity3D(value_range=(0, 1), noise_std=(0, 0.05))
    for aug in (None, _augment(), _augment(intensity=intensity)):
        s = T.PatchSampler3D((8, 16, 16), num_patches=3, augment=aug)
        g1, g2 = np.random.default_rng(5), np.random.default_rng(5)
        got = s.draw(g1)
        want = []
        for _ in range(3):
            chance, a, b = g2.random(), int(g2.integers(0, 2 ** 32)), int(g2.integers(0, 2 ** 32))
            want.append((chance < 2 / 3, a, b, aug.draw(g2) if aug is not None else None))
        assert got == want and g1.bit_generator.state == g2.bit_generator.state
        assert all(0 <= d[1] < 2 ** 32 and 0 <= d[2] < 2 ** 32 for d in got)
    # without an augment exactly three values a patch: the next uniform of both generators agrees after a manual skip
    g1, g2 = np.random.default_rng(9), np.random.default_rng(9)
    T.PatchSampler3D((8, 16, 16), num_patches=2).draw(g1)
    for _ in range(2):
        g2.random(), g2.integers(0, 2 ** 32), g2.integers(0, 2 ** 32)
    assert g1.random() == g2.random()


def test_identity_translation_and_matrix_composition():
    for patch in ((33, 7, 70), (32, 4, 64), (5, 7, 6)):
        A = T.PatchSampler3D(patch).matrix()
        assert A.dtype == np.float32 and np.array_equal(A[:, :3], np.eye(3)) and A[:, 3].tolist() == [-(p // 2) for p in patch]
        assert np.array_equal(A, T.patch_matrix(patch)) and np.array_equal(A, T.PatchSampler3D(patch).matrix(T.Augment3D.identity_params()))
    params = dict(T.Augment3D.identity_params(), applied=True, angles=(0.2, 0.0, -0.03), scales=(1.1, 0.9, 1.0), flips=(False, False, True))
    patch = (9, 20, 31)
    want = T.Augment3D.matrix(patch, params, np.float64)
    want[:, 3] -= [4, 10, 15]
    assert np.array_equal(T.PatchSampler3D(patch).matrix(params), want.astype(np.float32))


def test_sampler_refuses_translate_deform_and_bad_sizes():
    with pytest.raises(ValueError):
        T.PatchSampler3D((8, 16, 16), augment=T.Augment3D(translate=(0, 2, 0)))
    with pytest.raises(ValueError):
        T.PatchSampler3D((8, 16, 16), augment=T.Augment3D(deform=T.Deform3D()))
    for kw in (dict(patch=(8, 16)), dict(patch=(8, 0, 16)), dict(patch=(8, 16, 16), num_patches=17), dict(patch=(8, 16, 16), num_patches=0),
               dict(patch=(8, 16, 16), fg_prob=1.5)):
        with pytest.raises(ValueError):
            T.PatchSampler3D(**kw)
    with pytest.raises(nat.NativeError):
        T.patch_centres(torch.zeros(2, 4, 4, 4, dtype=torch.uint8), [(1, 0, 0)])            # a CPU tensor: no fallback
    from capstone_amd.volumetric.data_module import MiccaiDataModule3D
    with pytest.raises(ValueError):
        MiccaiDataModule3D(1, 1, patch_size=(8, 16, 16), dist_maps=True)
    s = MiccaiDataModule3D(1, 3, patch_size=(8, 16, 16), patches_per_volume=3, fg_prob=0.5).patch_sampler()
    assert (s.patch, s.num_patches, s.fg_prob, s.window) == ((8, 16, 16), 3, 0.5, T.augmented_degree_3["train"].window)
    assert s.augment.deform is None and not s.augment.translate.any() and s.augment.intensity is not None
    assert np.array_equal(s.augment.rotate, T.augmented_degree_3["train"].augment.rotate)


def test_seeded_fg_share_is_two_thirds():
    s = T.PatchSampler3D((8, 16, 16), num_patches=15, fg_prob=2 / 3)
    g = np.random.default_rng(12342)
    fg = [d[0] for _ in range(200) for d in s.draw(g)]
    n, p = len(fg), 2 / 3
    assert n == 3000
    share, sd = sum(fg) / n, (p * (1 - p) / n) ** 0.5
    print("fg share", share, "sd", sd)
    assert abs(share - p) <= 4 * sd


def test_oracles_agree_on_the_identity_crop():
    image, masks = inputs(SRC, nat.I16)
    for patch, centre in (((33, 7, 70), (20, 9, 44)), ((33, 25, 70), (3, 10, 88))):
        for border in (0, 1):
            want = PO.crop_oracle(image, masks, patch, centre, border, cval=-1000.0, window=2, lo=-160.0, hi=240.0)
            for interp in (0, 1):
                got = PO.patch_oracle(image, masks, patch, T.patch_matrix(patch), centre, interp, border, cval=-1000.0, window=2, lo=-160.0,
                                      hi=240.0)
                assert_same(got, want)


# ---- GPU: the centre pick ----------------------------------------------------------------------------------------------------
def _poisoned(masks):
    need = nat.lib().ctseg_patch_centres_workspace(*masks.shape)
    return torch.full((need // 4,), -1, dtype=torch.int32, device=masks.device)             # every byte 0xFF


def _pick(masks_d, draws, patch=None, class_mask=None):
    got = T.patch_centres(masks_d, draws, patch, class_mask, workspace=_poisoned(masks_d))
    again = T.patch_centres(masks_d, draws, patch, class_mask, workspace=_poisoned(masks_d))
    got, again = got.cpu().numpy(), again.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, again)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("dims", VOLUMES, ids=str)
def test_gpu_centres_are_the_rth_set_voxel(dims):
    masks = PO.centre_masks(dims)
    masks_d = on_device(masks)
    edge = [(1, a, b) for a in EDGE for b in EDGE]                                           # P = 16
    assert np.array_equal(_pick(masks_d, edge), PO.centres(masks, edge))
    assert {int(c) for c in PO.centres(masks, edge)[:, 3]} == {1, 2, 3}                      # never the empty class
    background = [(0, a, b) for a in EDGE[:2] for b in EDGE] + [(0, 7, 123456789 * i) for i in range(1, 9)]
    got = _pick(masks_d, background)
    assert np.array_equal(got, PO.centres(masks, background)) and (got[:, 3] == -1).all()
    # every rank of the ~300-voxel mask, 16 at a time; a = 2^32 - 1 is the last eligible class
    n = int(np.count_nonzero(masks[3]))
    ranks = [(1, 2 ** 32 - 1, PO.draw_for_rank(r, n)) for r in range(n)]
    want = PO.centres(masks, ranks)
    flat = np.flatnonzero(masks[3].reshape(-1))
    assert np.array_equal(np.ravel_multi_index(tuple(want[:, :3].T), dims), flat) and (want[:, 3] == 3).all()
    got = np.concatenate([_pick(masks_d, ranks[i:i + 16]) for i in range(0, n, 16)])
    assert np.array_equal(got, want)
    # the dense class dropped; one patch; the single voxel at the last index
    for cm in (0b1011, 0b0010, 0b0001):
        assert np.array_equal(_pick(masks_d, edge, class_mask=cm), PO.centres(masks, edge, cm))
    assert (_pick(masks_d, edge, class_mask=0b0001)[:, 3] == -1).all()                       # only the empty class: background
    assert _pick(masks_d, [(1, 0, 5)], class_mask=0b0010).tolist() == [[dims[0] - 1, dims[1] - 1, dims[2] - 1, 1]]
    one = [(1, 2 ** 31, 2 ** 31)]
    assert np.array_equal(_pick(masks_d, one), PO.centres(masks, one))
    # all masks empty
    empty = torch.zeros_like(masks_d)
    got = _pick(empty, edge)
    assert np.array_equal(got, PO.centres(np.zeros_like(masks), edge)) and (got[:, 3] == -1).all()
    # the cached workspace of the default call gives the same
    assert np.array_equal(T.patch_centres(masks_d, edge).cpu().numpy(), PO.centres(masks, edge))


@pytest.mark.gpu
def test_gpu_centres_are_clamped_to_the_patch():
    dims = (10, 12, 14)
    masks = np.zeros((8,) + dims, np.uint8)
    corners = [(d, h, w) for d in (0, 9) for h in (0, 11) for w in (0, 13)]
    for k, c in enumerate(corners):
        masks[k][c] = 1
    draws = [(1, k << 29, 0) for k in range(8)]                                              # a * 8 >> 32 = k
    masks_d = on_device(masks)
    raw = _pick(masks_d, draws)
    assert raw.tolist() == [list(c) + [k] for k, c in enumerate(corners)]
    for patch in ((4, 8, 6), (5, 7, 6), (3, 12, 1)):
        got = _pick(masks_d, draws, patch)
        assert np.array_equal(got, PO.centres(masks, draws, None, patch))
        for a in range(3):
            lo, hi = patch[a] // 2, dims[a] - (patch[a] - patch[a] // 2)
            assert set(got[:, a].tolist()) == {lo, hi}
            assert lo - patch[a] // 2 == 0 and hi - patch[a] // 2 + patch[a] == dims[a]      # the patch touches both ends
    assert _pick(masks_d, draws, (4, 8, 6))[:, :3].tolist()[0] == [2, 4, 3] and _pick(masks_d, draws, (4, 8, 6))[7, :3].tolist() == [8, 8, 11]
    # an axis shorter than the patch: its centre is dim // 2
    got = _pick(masks_d, draws, (11, 8, 15))
    assert np.array_equal(got, PO.centres(masks, draws, None, (11, 8, 15)))
    assert (got[:, 0] == 5).all() and (got[:, 2] == 7).all() and set(got[:, 1].tolist()) == {4, 8}


# ---- GPU: the crop -----------------------------------------------------------------------------------------------------------
def _device_centre(masks, masks_d, draw, patch):
    """a centre that a preceding patch_centres call wrote on the same stream, and what it holds"""
    table = T.patch_centres(masks_d, [(0, 0, 0), draw], patch)
    return table[1], PO.centres(masks, [draw], None, patch)[0]


CROPS = [((33, 7, 70), True), ((32, 4, 64), True), ((33, 25, 70), True), ((33, 7, 70), False)]     # (patch, centre clamped)


@pytest.mark.gpu
@pytest.mark.parametrize("patch,clamped", CROPS, ids=str)
@pytest.mark.parametrize("border", [0, 1])
def test_gpu_identity_crop_is_numpy_slicing(patch, clamped, border):
    A = T.patch_matrix(patch)
    for code, window, interp in ((nat.I16, None, 0), (nat.F32, (400, 40, True), 1), (nat.U8, (100, 120, False), 0)):
        image, masks = inputs(SRC, code)
        image_d, masks_d = on_device(image, masks)
        # an unclamped centre next to the volume's corner sends part of the patch outside: cval / 0, or the edge voxel
        draw = (1, 3 << 29, 2 ** 32 - 1) if clamped else (0, 0, 2 ** 32 - 1)
        centre_d, centre = _device_centre(masks, masks_d, draw, patch if clamped else None)
        wn, lo, hi = T._window_args(window)
        want = PO.crop_oracle(image, masks, patch, centre, border, -1000.0, wn, lo, hi)
        if patch[1] > SRC[1] and not border:
            assert (want[0] == PO.window_f32(np.float32(-1000.0), wn, lo, hi)).any() and want[3][0] > 0
        got = T.patch3d_to_hwd(image_d, masks_d, patch, A, centre_d, interp, border, -1000.0, None, window, want_masks=True, want_labels=True)
        assert_same(as_numpy(got), want)
        # K = 0: the image alone; the masks alone
        got = T.patch3d_to_hwd(image_d, None, patch, A, centre_d, interp, border, -1000.0, window=window)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and got[1] is None and got[2] is None
        got = T.patch3d_to_hwd(None, masks_d, patch, A, centre_d, 0, border)
        assert got[0] is None and np.array_equal(got[1].cpu().numpy(), want[1])


GENERAL = dict(T.Augment3D.identity_params(), applied=True, angles=(0.26, 0.05, -0.04), scales=(1.1, 0.9, 1.05), flips=(False, False, True),
               gain=1.07, bias=-0.02)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("border", [0, 1])
def test_gpu_general_matrix_is_the_translated_affine_pass(interp, border):
    patch = (33, 7, 70)
    image, masks = inputs(SRC, nat.I16)
    image_d, masks_d = on_device(image, masks)
    A = T.PatchSampler3D(patch).matrix(GENERAL)
    for draw, clamp in (((1, 5 << 29, 2 ** 31), patch), ((0, 0, 77), None)):                 # inside; at the corner: much lies outside
        centre_d, centre = _device_centre(masks, masks_d, draw, clamp)
        want = PO.patch_oracle(image, masks, patch, A, centre, interp, border, -1000.0, SWAPPED, 2, -160.0, 240.0, GENERAL["gain"],
                               GENERAL["bias"])
        got = T.patch3d_to_hwd(image_d, masks_d, patch, A, centre_d, interp, border, -1000.0, SWAPPED, (400, 40, True), GENERAL["gain"],
                               GENERAL["bias"], want_masks=True, want_labels=True)
        assert_same(as_numpy(got), want)
    # the identity through the same route equals the slicing of the test above
    centre_d, centre = _device_centre(masks, masks_d, (1, 5 << 29, 2 ** 31), patch)
    got = T.patch3d_to_hwd(image_d, masks_d, patch, T.patch_matrix(patch), centre_d, interp, border, want_masks=True, want_labels=True)
    assert_same(as_numpy(got), PO.crop_oracle(image, masks, patch, centre, border))


# ---- GPU: sampler, dataset, trainer ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_sampler_is_reproducible_and_follows_explicit_draws():
    image, masks = inputs(SRC, nat.I16)
    image_d, masks_d = on_device(image, masks)
    patch = (16, 8, 40)
    for squash in (False, True):
        s = T.PatchSampler3D(patch, num_patches=3, squash=squash, window=(400, 40, True), augment=_augment())
        a, b = s(image_d, masks_d, generator=np.random.default_rng(3)), s(image_d, masks_d, generator=np.random.default_rng(3))
        assert a["draws"] == b["draws"] and a["channel_src"] == b["channel_src"]
        for key in ("image", "masks", "centres") + (("hist",) if squash else ()):
            assert torch.equal(a[key], b[key]), key
        assert a["image"].shape == (3, 1, 8, 40, 16) and a["masks"].shape == ((3, 8, 40, 16) if squash else (3, K, 8, 40, 16))
        if squash:
            assert a["hist"].shape == (3, K + 1) and a["hist"].sum(1).tolist() == [16 * 8 * 40] * 3
    # explicit draws: the centres of the rule, and exact crops about them
    draws = [(1, a, b) for a in EDGE[1:3] for b in EDGE[1:3]]
    s = T.PatchSampler3D(patch, num_patches=4, squash=True)
    res = s(image_d.unsqueeze(0), masks_d, draws=draws)
    want_c = PO.centres(masks, draws, None, patch)
    assert np.array_equal(res["centres"].cpu().numpy(), want_c) and res["channel_src"] == [list(range(K))] * 4
    for i in range(4):
        want = PO.crop_oracle(image, masks, patch, want_c[i])
        assert np.array_equal(res["image"][i, 0].cpu().numpy(), want[0]) and np.array_equal(res["masks"][i].cpu().numpy(), want[2])
        assert np.array_equal(res["hist"][i].cpu().numpy(), want[3])


@pytest.mark.gpu
def test_gpu_patch_dataset_permutes_the_indicator_with_the_mirror(tmp_path):
    write_instances(tmp_path, (24, 40, 44), splits=("train",), n=2)
    mirror = T.Augment3D(flip_prob=(0, 0, 1.0))
    s = T.PatchSampler3D((16, 32, 32), num_patches=2, augment=mirror)
    ds = DS.get_miccai_3d("train", root=str(tmp_path), device=DEV, generator=np.random.default_rng(1), patches=s)
    assert isinstance(ds, DS.MiccaiPatchDataset3D) and len(ds) == 2
    items = [ds[0], ds[1]]
    ind = np.array([1, 1, 0, 1, 0, 1, 1, 0, 1.0])
    for item in items:
        assert len(item) == 2
        for image, masks, indicator in item:
            assert image.shape == (1, 32, 32, 16) and masks.shape == (K, 32, 32, 16) and masks.dtype == torch.uint8
            assert np.array_equal(indicator.cpu().numpy(), ind[SWAPPED])
    images, masks, indicator = DS.collate_patches_3d(items)
    assert images.shape == (4, 1, 32, 32, 16) and masks.shape == (4, K, 32, 32, 16) and indicator.shape == (4, K)
    assert torch.equal(images[1], items[0][1][0]) and torch.equal(images[2], items[1][0][0])
    # the mirrored patch itself: output channel k is the w-mirrored crop of input channel SWAPPED[k]
    inst = np.load(ds.instance_paths[0])
    res = s(torch.from_numpy(inst["image"]).to(DEV), torch.from_numpy(inst["masks"]).to(DEV), generator=np.random.default_rng(1))
    assert res["channel_src"] == [SWAPPED, SWAPPED]
    c = res["centres"].cpu().numpy()[0]
    plain = PO.crop_oracle(None, inst["masks"], (16, 32, 32), c)[1]                           # (K, h, w, d)
    assert np.array_equal(res["masks"][0].cpu().numpy(), plain[SWAPPED][:, :, ::-1, :])
    # a squashing sampler carries the label maps and their counts through the collate
    sq = DS.MiccaiPatchDataset3D(ds.path, T.PatchSampler3D((16, 32, 32), squash=True), device=DEV, generator=np.random.default_rng(2))
    images, labels, indicator = DS.collate_patches_3d([sq[0], sq[1]])
    assert labels.shape == (4, 32, 32, 16) and labels._ctseg_labels[0].shape == (4, 32 * 32 * 16) and labels._ctseg_labels[1].shape == (4, K + 1)
    assert np.array_equal(indicator.cpu().numpy(), np.tile(ind, (4, 1)))


def _model(**kw):
    from capstone_amd.volumetric.base_trainer import BaseUNet3D
    torch.manual_seed(7)
    return BaseUNet3D(filters=[4, 8, 8], loss_fx=["CrossEntropy"], **kw).to(DEV)


@pytest.mark.gpu
def test_gpu_fit_step_on_a_collated_patch_batch(tmp_path):
    from capstone_amd.volumetric.data_module import MiccaiDataModule3D
    write_instances(tmp_path, (24, 40, 44), n=2)
    dm = MiccaiDataModule3D(2, 1, root=str(tmp_path), device=DEV, seed=4, patch_size=(16, 32, 32), patches_per_volume=2)
    dm.setup("fit")
    assert isinstance(dm.train_dataset, DS.MiccaiPatchDataset3D) and isinstance(dm.val_dataset, DS.MiccaiDataset3D)
    batch = next(iter(dm.train_dataloader()))
    assert batch[0].shape == (4, 1, 32, 32, 16) and batch[1].shape == (4, K, 32, 32, 16) and batch[2].shape == (4, K)
    loss = _model().fit_step(batch)
    direct = _model().fit_step(tuple(t.clone() for t in batch))
    assert torch.isfinite(loss) and torch.equal(loss, direct)


@pytest.mark.gpu
def test_gpu_validation_through_the_sliding_window_inferer():
    from capstone_amd.inferers import SlidingWindowInferer, sliding_window_inference
    from capstone_amd.training.utils import _squash_predictions
    from capstone_amd.volumetric.metrics import DiceMetricWrapper3D
    from capstone_amd.volumetric.utils import _squash_masks_3D
    g = torch.Generator().manual_seed(3)
    masks = torch.zeros(2, 9, 24, 40, 36, dtype=torch.uint8)
    for c in range(9):
        masks[:, c, 2 * c:2 * c + 6, 4:30, 3:25] = 1
    batch = (torch.randn(2, 1, 24, 40, 36, generator=g).to(DEV), masks.to(DEV), torch.ones(2, 9).to(DEV))
    plain = _model()
    with torch.no_grad():
        plain.validation_step(batch)
    m = _model(val_inferer=SlidingWindowInferer((16, 32, 32), sw_batch_size=2, overlap=0.25))
    assert "val_inferer" not in m.hparams
    with torch.no_grad():
        m.validation_step(batch)
        logits = torch.cat([sliding_window_inference(batch[0][i:i + 1], (16, 32, 32), 2, m, 0.25).clone() for i in range(2)])
        want_mean, want_per_class = DiceMetricWrapper3D()(_squash_predictions(logits), _squash_masks_3D(batch[1], 10, DEV))
    assert set(m.logged) == set(plain.logged) >= {f"{s} Dice (val)" for s in STRUCTURES} | {"Mean Dice Score (val)", "CrossEntropy Loss (val)"}
    assert torch.equal(m.logged["Mean Dice Score (val)"], want_mean)
    for s, v in zip(STRUCTURES, want_per_class):
        assert torch.equal(m.logged[f"{s} Dice (val)"], v, ) or (torch.isnan(v) and torch.isnan(m.logged[f"{s} Dice (val)"]))
    assert torch.isfinite(m.logged["CrossEntropy Loss (val)"])
