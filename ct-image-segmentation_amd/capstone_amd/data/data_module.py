"""Drop-in for reference capstone/data/data_module.py: ``MiccaiDataModule2D`` / ``FullMiccaiDataModule2D`` over the device store.

The loaders are plain iterables of device batches ``(images, masks, mask_indicator)`` (``enhanced=True, device_maps=True``: plus
``distance_maps``): a shuffled (train) or sequential order cut into ``batch_size`` pieces, each piece one ``MiccaiDataset2D.batch``
launch.  No workers, no pinned memory: nothing crosses the host after ``setup``.  The classes derive from ``pl.LightningDataModule`` only when Lightning is importable.
"""
from typing import Optional

import numpy as np
import torch

from ..transforms import predefined
from ..volumetric.base_trainer import pl
from .datasets import get_miccai_2d

DEGREE = {
    0: predefined.degree_0,
    1: predefined.windowed_degree_1,
    2: predefined.windowed_degree_2,
    3: predefined.windowed_degree_3,
    4: predefined.windowed_degree_4,
}
# device_warps=True: the degrees whose "train" side warps take their device restatement
WARPED_DEGREE = {0: predefined.warped["degree_0"], 3: predefined.warped["windowed_degree_3"], 4: predefined.warped["windowed_degree_4"]}


def _cat_masks(parts):
    masks = torch.cat(parts)
    if all(hasattr(p, "_ctseg_present") for p in parts):
        masks._ctseg_present = torch.cat([p._ctseg_present for p in parts])
    if all(hasattr(p, "_ctseg_labels") for p in parts):
        masks._ctseg_labels = (masks.reshape(masks.shape[0], -1), torch.cat([p._ctseg_labels[1] for p in parts]))
    return masks


class DeviceBatches:
    """iterable over one or more datasets (ConcatDataset's index space): every dataset keeps its own transform, so a batch that
    spans two of them is one launch per dataset"""

    def __init__(self, datasets, batch_size: int, shuffle: bool, generator=None):
        self.datasets = list(datasets)
        self.batch_size, self.shuffle = int(batch_size), shuffle
        self.generator = generator if generator is not None else np.random.default_rng()
        self.bounds = np.cumsum([0] + [len(d) for d in self.datasets])

    def __len__(self):
        return (int(self.bounds[-1]) + self.batch_size - 1) // self.batch_size

    def order(self):
        n = int(self.bounds[-1])
        return self.generator.permutation(n) if self.shuffle else np.arange(n)

    def __iter__(self):
        order = self.order()
        for i in range(0, len(order), self.batch_size):
            idx = order[i:i + self.batch_size]
            parts = [d.batch(idx[(idx >= lo) & (idx < hi)] - lo) for d, lo, hi in zip(self.datasets, self.bounds[:-1], self.bounds[1:])
                     if ((idx >= lo) & (idx < hi)).any()]
            if len(parts) == 1:
                yield parts[0]
            else:
                # (an enhanced dataset's fourth element, the distance maps, is concatenated like the indicator)
                yield (torch.cat([p[0] for p in parts]), _cat_masks([p[1] for p in parts])) + tuple(
                    torch.cat([p[k] for p in parts]) for k in range(2, len(parts[0])))


class MiccaiDataModule2D(pl.LightningDataModule if pl is not None else object):
    def __init__(self, batch_size, transform_degree: int = None, enhanced=False, root: str = "storage", device="cuda",
                 generator=None, device_warps=False, device_maps=False, **kwargs):
        super().__init__()
        self.batch_size = batch_size
        assert transform_degree in DEGREE.keys(), "Invalid transform degree passed"
        self.transform = WARPED_DEGREE[transform_degree] if device_warps and transform_degree in WARPED_DEGREE else DEGREE[transform_degree]
        self.enhanced, self.device_maps = enhanced, device_maps      # enhanced without device_maps: the old refusal, at setup
        self.root, self.device = root, device
        self.generator = generator                 # numpy Generator: the shuffle and the random crop / rot90 / flip

    def _dataset(self, split, side):
        return get_miccai_2d(split=split, transform=self.transform[side], enhanced=self.enhanced, root=self.root, device=self.device,
                             generator=self.generator, device_maps=self.device_maps)

    def setup(self, stage: Optional[str] = None):
        if stage == "fit" or stage is None:
            self.train_dataset = self._dataset("train", "train")
            self.val_dataset = self._dataset("valid", "test")
        if stage == "test" or stage is None:
            self.test_dataset = self._dataset("test", "test")

    def train_dataloader(self):
        return DeviceBatches([self.train_dataset], self.batch_size, shuffle=True, generator=self.generator)

    def val_dataloader(self):
        return DeviceBatches([self.val_dataset], self.batch_size, shuffle=False)

    def test_dataloader(self):
        return DeviceBatches([self.test_dataset], self.batch_size, shuffle=False)


class FullMiccaiDataModule2D(MiccaiDataModule2D):
    def train_dataloader(self):
        return DeviceBatches([self.train_dataset, self.val_dataset], self.batch_size, shuffle=True, generator=self.generator)
