"""Device-fed counterpart of reference capstone/volumetric/datasets.py.

``MiccaiDataset3D`` reads the same ``.npz`` instances (``image`` 1xDxHxW, ``masks`` 9xDxHxW, ``mask_indicator`` 9 — written by
capstone/data/process_miccai.py:96-131), uploads the raw arrays once and runs the transform on the MI355X
(``transforms.InstancePipeline3D``) instead of albumentations on the host.  ``__getitem__`` returns the reference's triple
``(image (1,H,W,D), masks (9,H,W,D), mask_indicator (9,))`` as device tensors, or — with a ``squash=True`` pipeline —
``masks`` already reduced to the (H,W,D) uint8 label map; ``collate_3d`` stacks either form into the batch ``BaseUNet3D``
takes (pre-squashed label maps are recognised by ``_squash_masks_3D`` / ``fit_step`` and skip the squash pass).
"""
from pathlib import Path

import numpy as np
import torch

from .. import STRUCTURES
from ..data.utils import compute_distance_map
from .transforms import InstancePipeline3D


class MiccaiDataset3D:
    def __init__(self, path: str, transform=None, device="cuda", dist_maps: bool = False, signed: bool = False, generator=None):
        """``dist_maps=True``: ``__getitem__`` returns a fourth element, the (9,H,W,D) fp32 distance maps of the transformed masks
        (the Boundary loss's input, ``BaseUNet3D(device_boundary=True)``); ``signed`` as ``data.utils.compute_distance_map``.
        ``generator`` (a ``numpy.random.Generator``) is handed to an augmenting transform (``InstancePipeline3D(augment=...)``) for
        its draws; when such a transform reports a channel permutation (``"channel_src"``: a left-right mirror swapped the paired
        structures), ``mask_indicator`` is permuted with it."""
        self.path = Path(path).absolute()
        self.transform = transform
        self.generator = generator
        self.dist_maps, self.signed = dist_maps, signed
        if dist_maps and transform is not None and not getattr(transform, "dist_maps", False):
            raise ValueError("MiccaiDataset3D(dist_maps=True) needs a transform that returns \"dist_maps\" "
                             "(InstancePipeline3D(dist_maps=True)) or no transform")
        self.device = torch.device(device)
        self.instance_paths = sorted(p.as_posix() for p in self.path.iterdir())      # same order on every platform (ref :16-18)

    def __len__(self) -> int:
        return len(self.instance_paths)

    def __getitem__(self, index: int):
        instance = np.load(self.instance_paths[index])
        image, masks, mask_indicator = instance["image"], instance["masks"], instance["mask_indicator"]
        assert len(mask_indicator) == len(STRUCTURES)
        assert masks.shape[0] == len(STRUCTURES)
        image = torch.from_numpy(np.ascontiguousarray(image)).to(self.device, non_blocking=True)
        masks = torch.from_numpy(np.ascontiguousarray(masks).view(np.uint8) if masks.dtype == np.bool_ else np.ascontiguousarray(masks))
        masks = masks.to(self.device, non_blocking=True)
        hist = maps = None
        if self.transform is not None:
            if getattr(self.transform, "augment", None) is not None:
                transformed = self.transform(image=image, masks=masks, generator=self.generator)
            else:
                transformed = self.transform(image=image, masks=masks)
            image, masks, hist = transformed["image"], transformed["masks"], transformed.get("hist")
            maps = transformed.get("dist_maps") if self.dist_maps else None
            if transformed.get("channel_src") is not None:
                mask_indicator = mask_indicator[np.asarray(transformed["channel_src"], dtype=np.int64)]
        elif self.dist_maps:
            maps = compute_distance_map(masks, signed=self.signed, spatial_dims=3)
        mask_indicator = torch.from_numpy(mask_indicator).to(self.device)
        if hist is not None:
            masks._ctseg_hist = hist
        if self.dist_maps:
            return image, masks, mask_indicator, maps
        return image, masks, mask_indicator


def collate_3d(samples):
    """list of ``__getitem__`` triples -> (images (B,1,H,W,D), masks, mask_indicator (B,9)); masks = (B,9,H,W,D) uint8, or the
    (B,H,W,D) uint8 label maps of a squashing pipeline carrying ``_ctseg_labels`` = (labels (B,S), per-class counts (B,10)).
    When every sample has a fourth element (``dist_maps=True``), the (B,9,H,W,D) fp32 maps follow as the batch's fourth."""
    images = torch.stack([s[0] for s in samples])
    indicator = torch.stack([s[2] for s in samples])
    masks = torch.stack([s[1] for s in samples])
    if all(hasattr(s[1], "_ctseg_hist") for s in samples):
        masks._ctseg_labels = (masks.reshape(len(samples), -1), torch.stack([s[1]._ctseg_hist for s in samples]))
    if all(len(s) == 4 for s in samples):
        return images, masks, indicator, torch.stack([s[3] for s in samples])
    return images, masks, indicator


class MiccaiPatchDataset3D:
    """The same ``.npz`` instances through a ``transforms.PatchSampler3D``: one item is the list of the sampler's P patches of
    one volume, each a ``MiccaiDataset3D`` triple at the patch's size: ``(image (1,h,w,d), masks (9,h,w,d), mask_indicator (9,))``,
    or, with a squashing sampler, ``masks`` = the (h,w,d) uint8 label map carrying its class counts.  ``mask_indicator`` is
    repeated per patch and permuted by that patch's ``channel_src`` (a left-right mirror swaps the paired structures).
    ``generator`` (a ``numpy.random.Generator``) feeds the sampler's draws.  ``collate_patches_3d`` makes the trainer's batch."""

    def __init__(self, path: str, sampler, device="cuda", generator=None):
        self.path = Path(path).absolute()
        self.sampler, self.generator = sampler, generator
        self.device = torch.device(device)
        self.instance_paths = sorted(p.as_posix() for p in self.path.iterdir())

    def __len__(self) -> int:
        return len(self.instance_paths)

    def __getitem__(self, index: int):
        instance = np.load(self.instance_paths[index])
        image, masks, mask_indicator = instance["image"], instance["masks"], instance["mask_indicator"]
        assert len(mask_indicator) == len(STRUCTURES)
        assert masks.shape[0] == len(STRUCTURES)
        image = torch.from_numpy(np.ascontiguousarray(image)).to(self.device, non_blocking=True)
        masks = torch.from_numpy(np.ascontiguousarray(masks).view(np.uint8) if masks.dtype == np.bool_ else np.ascontiguousarray(masks))
        masks = masks.to(self.device, non_blocking=True)
        res = self.sampler(image, masks, generator=self.generator)
        samples = []
        for i, src in enumerate(res["channel_src"]):
            m = res["masks"][i]
            if res.get("hist") is not None:
                m._ctseg_hist = res["hist"][i]
            indicator = torch.from_numpy(mask_indicator[np.asarray(src, dtype=np.int64)]).to(self.device)
            samples.append((res["image"][i], m, indicator))
        return samples


def collate_patches_3d(items):
    """list of ``MiccaiPatchDataset3D`` items (each the list of one volume's patches) -> ``collate_3d`` of all their patches, volume
    by volume: a batch of ``len(items) * P`` samples"""
    return collate_3d([s for item in items for s in item])


def get_miccai_3d(split: str = "train", transform=None, root: str = "storage", device="cuda", dist_maps: bool = False,
                  signed: bool = False, generator=None, patches=None):
    """``patches`` = a ``transforms.PatchSampler3D``: the split as a ``MiccaiPatchDataset3D`` (no ``transform``, no distance maps)"""
    assert split in ["train", "valid", "test"], "Invalid data split passed"
    if patches is not None:
        if transform is not None or dist_maps:
            raise ValueError("get_miccai_3d(patches=...) takes neither a transform nor dist_maps")
        return MiccaiPatchDataset3D(f"{root}/miccai_3d/{split}", patches, device=device, generator=generator)
    if transform is None:
        transform = InstancePipeline3D(dist_maps=dist_maps, signed=signed)
    return MiccaiDataset3D(f"{root}/miccai_3d/{split}", transform=transform, device=device, dist_maps=dist_maps, signed=signed,
                           generator=generator)
