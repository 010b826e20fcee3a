"""Device-fed counterpart of reference capstone/data/datasets.py.

``MiccaiDataset2D`` reads the same ``.npz`` instances (``image`` 1xHxW, ``masks`` 9xHxW, ``mask_indicator`` 9 — written by
capstone/data/process_miccai.py:60-94) in the same sorted order with the same asserts, and uploads every slice ONCE into a flat
device store (``transforms.pipeline2d.SliceStore2D``: raw image elements, mask bytes, a per-slice (offset, H, W) table) plus
``mask_indicator`` (N, 9).  ``transform`` is a ``BatchPipeline2D`` (capstone_amd/transforms/predefined.py) instead of an
albumentations Compose.  ``__getitem__`` returns the reference's triple ``(image (C,H',W'), masks (9,H',W'), mask_indicator (9,))``
as device tensors; ``batch(indices)`` is the route the data module takes: one launch for the whole batch.
``EnhancedMiccaiDataset2D`` (``enhanced=True`` together with the opt-in ``device_maps=True``) adds the per-class distance maps of the
transformed masks (data/utils.py) as a fourth element, computed on the device.  ``enhanced=True`` alone raises
``NotImplementedError`` as before, and the Boundary loss that would consume the maps still raises in the trainers.
"""
from pathlib import Path

import numpy as np
import torch

from .. import STRUCTURES
from ..transforms.pipeline2d import SliceStore2D
from .utils import compute_distance_map


class MiccaiDataset2D:
    def __init__(self, path: str, transform=None, device="cuda", generator=None) -> None:
        self.path = Path(path).absolute()
        self.transform = transform
        self.device = torch.device(device)
        self.generator = generator                 # numpy Generator of the random crop / rot90 / flip (None: the pipeline's own)
        self.instance_paths = sorted(p.as_posix() for p in self.path.iterdir())      # same order on every platform (ref :29-32)
        images, masks, indicator = [], [], []
        for p in self.instance_paths:
            instance = np.load(p)
            image, m, mask_indicator = instance["image"], instance["masks"], instance["mask_indicator"]
            assert len(mask_indicator) == len(STRUCTURES)
            assert m.shape[0] == len(STRUCTURES)
            images.append(image.reshape(image.shape[-2:]))
            masks.append(m)
            indicator.append(mask_indicator)
        self.store = SliceStore2D(images, masks, self.device)
        self.mask_indicator = torch.from_numpy(np.stack(indicator)).to(self.device)

    def __len__(self) -> int:
        return len(self.instance_paths)

    def batch(self, indices, params=None):
        """-> (images (B,C,H',W') fp32, masks (B,9,H',W') uint8 — or the (B,H',W') label maps of a squashing pipeline —,
        mask_indicator (B,9))"""
        if self.transform is None:
            raise ValueError("MiccaiDataset2D.batch needs a BatchPipeline2D transform (raw slices differ in size)")
        idx = torch.as_tensor(np.asarray(indices, dtype=np.int64))
        images, masks, _ = self.transform(self.store, idx, params=params, generator=self.generator)
        return images, masks, self.mask_indicator[idx.to(self.device)]

    def __getitem__(self, index: int):
        if self.transform is None:
            image, masks = self.store.raw(index)
            return image.unsqueeze(-1), masks, self.mask_indicator[index]
        images, masks, indicator = self.batch([index])
        return images[0], masks[0], indicator[0]


class EnhancedMiccaiDataset2D(MiccaiDataset2D):
    """reference datasets.py:58-69: the triple plus ``distance_maps`` (9, H', W') fp32 of the TRANSFORMED nine masks.  ``signed``:
    the float signed map instead of the reference's uint8-wrapped one (data/utils.py)."""

    def __init__(self, path: str, transform=None, device="cuda", generator=None, signed=False) -> None:
        super().__init__(path, transform=transform, device=device, generator=generator)
        self.signed = bool(signed)

    def batch(self, indices, params=None):
        """-> (images, masks — or the label maps of a squashing pipeline, stashes included —, mask_indicator,
        distance_maps (B,9,H',W') fp32).  A squashing pipeline writes the nine masks in the same launch as its labels: overlapping
        structures cannot be taken back from a label map."""
        if self.transform is None:
            raise ValueError("EnhancedMiccaiDataset2D.batch needs a BatchPipeline2D transform (raw slices differ in size)")
        idx = torch.as_tensor(np.asarray(indices, dtype=np.int64))
        images, masks, _ = self.transform(self.store, idx, params=params, generator=self.generator, with_masks=True)
        nine = masks._ctseg_masks if hasattr(masks, "_ctseg_masks") else masks
        return images, masks, self.mask_indicator[idx.to(self.device)], compute_distance_map(nine, signed=self.signed)

    def __getitem__(self, index: int):
        if self.transform is None:
            image, masks, indicator = super().__getitem__(index)
            return image, masks, indicator, compute_distance_map(masks, signed=self.signed)
        images, masks, indicator, maps = self.batch([index])
        return images[0], masks[0], indicator[0], maps[0]


def get_miccai_2d(split: str = "train", transform=None, enhanced=False, root: str = "storage", device="cuda", generator=None,
                  device_maps=False):
    assert split in ["train", "valid", "test"], "Invalid data split passed"
    if enhanced and not device_maps:
        raise NotImplementedError("distance maps (EnhancedMiccaiDataset2D) are computed on the device only on request: pass "
                                  "device_maps=True (the Boundary loss that consumes them is outside the MI355X hot path)")
    _dataset = EnhancedMiccaiDataset2D if enhanced else MiccaiDataset2D
    return _dataset(f"{root}/miccai_2d/{split}", transform=transform, device=device, generator=generator)
