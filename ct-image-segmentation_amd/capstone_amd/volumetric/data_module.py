"""Drop-in for reference capstone/volumetric/data_module.py: ``MiccaiDataModule3D`` over the device-fed ``MiccaiDataset3D``.

``transform_degree`` 0 is the reference's only preset (resize + permute); 1 adds the device augmentation of
``transforms.augmented_degree_1`` on the "train" side; 3 is ``transforms.augmented_degree_3``: the soft-tissue window on both sides
and, on the "train" side, degree 1 plus the free-form deformation and the intensity stage (blur, noise, gamma).
``transforms.augmented_degree_2``, degree 1 plus the deformation on the unwindowed image, has no number here: it goes to
``get_miccai_3d`` / ``MiccaiDataset3D`` directly.  The loaders are plain iterables of device batches
``(images, masks, mask_indicator)`` (``dist_maps=True``: plus the distance maps): a shuffled (train) or sequential order cut into
``batch_size`` pieces, every instance one ``MiccaiDataset3D.__getitem__`` (one launch) and every piece one ``collate_3d``.  No
workers, no pinned memory.  The class derives from ``pl.LightningDataModule`` only when Lightning is importable.
``patch_size`` opts the train split into ``transforms.PatchSampler3D``: native-resolution patches, most of them centred on a
structure, ``patches_per_volume`` per instance, so that a train batch has ``batch_size * patches_per_volume`` samples; validation
and test stay whole volumes through the preset's "test" side (``BaseUNet3D(val_inferer=...)`` predicts them window by window).
"""
from typing import Optional

import numpy as np

from . import transforms
from .base_trainer import pl
from .datasets import collate_3d, collate_patches_3d, get_miccai_3d
from .transforms import Augment3D, InstancePipeline3D, PatchSampler3D

DEGREE = {0: transforms.windowed_degree_0, 1: transforms.augmented_degree_1, 3: transforms.augmented_degree_3}


class InstanceBatches:
    """iterable of ``collate`` (default ``collate_3d``) batches over one dataset"""

    def __init__(self, dataset, batch_size: int, shuffle: bool, generator=None, collate=collate_3d):
        self.dataset, self.batch_size, self.shuffle, self.collate = dataset, int(batch_size), shuffle, collate
        self.generator = generator if generator is not None else np.random.default_rng()

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        order = self.generator.permutation(n) if self.shuffle else np.arange(n)
        for i in range(0, n, self.batch_size):
            yield self.collate([self.dataset[int(j)] for j in order[i:i + self.batch_size]])


class MiccaiDataModule3D(pl.LightningDataModule if pl is not None else object):
    def __init__(self, batch_size, transform_degree: int = None, root: str = "storage", device="cuda", dist_maps: bool = False,
                 signed: bool = False, seed: Optional[int] = None, size=None, patch_size=None, patches_per_volume: int = 2,
                 fg_prob: float = 2 / 3, **kwargs):
        """``dist_maps`` / ``signed`` as ``MiccaiDataset3D``; ``seed`` seeds the one ``numpy.random.Generator`` behind the train
        shuffle and the augmentation's draws (None: fresh entropy); ``size`` = another (D', H', W') target than the preset's.
        ``patch_size`` = (D', H', W') switches the TRAIN split to ``PatchSampler3D(patch_size, patches_per_volume, fg_prob)`` with
        the preset's window and squash and its ``Augment3D`` minus translate and deform; not with ``dist_maps``"""
        super().__init__()
        self.batch_size = batch_size
        assert transform_degree in DEGREE.keys(), "Invalid transform degree passed"
        self.transform = DEGREE[transform_degree]
        self.root, self.device, self.dist_maps, self.signed = root, device, dist_maps, signed
        self.size = None if size is None else tuple(int(v) for v in size)
        self.generator = np.random.default_rng(seed)
        self.patch_size = None if patch_size is None else tuple(int(v) for v in patch_size)
        self.patches_per_volume, self.fg_prob = int(patches_per_volume), float(fg_prob)
        if self.patch_size is not None and dist_maps:
            raise ValueError("MiccaiDataModule3D: patch_size does not go with dist_maps")

    def patch_sampler(self):
        """the train split's ``PatchSampler3D``: the "train" preset's window and squash, and its augmentation about the patch centre
        (rotation, zoom, mirrors, gain / bias, intensity; the translation is the centre's, and a patch is not deformed)"""
        t = self.transform["train"]
        a = t.augment
        if a is not None:
            a = Augment3D(rotate=a.rotate, scale=a.scale, flip_prob=a.flip_prob, swap_pairs=a.swap_pairs, gain=a.gain, bias=a.bias,
                          interp=a.interp, border=a.border, cval=a.cval, p=a.p, intensity=a.intensity)
        return PatchSampler3D(self.patch_size, self.patches_per_volume, self.fg_prob, squash=t.squash, window=t.window, augment=a)

    def _dataset(self, split, side):
        t = self.transform[side]
        size = t.size if self.size is None else self.size
        maps, signed = (True, self.signed) if self.dist_maps else (t.dist_maps, t.signed)
        if (size, maps, signed) != (t.size, t.dist_maps, t.signed):      # the preset with the maps switched on / another target
            t = InstancePipeline3D(size, t.squash, t.window, maps, signed, t.augment)
        return get_miccai_3d(split=split, transform=t, root=self.root, device=self.device, dist_maps=self.dist_maps,
                             signed=self.signed, generator=self.generator)

    def setup(self, stage: Optional[str] = None):
        if stage == "fit" or stage is None:
            if self.patch_size is not None:
                self.train_dataset = get_miccai_3d(split="train", root=self.root, device=self.device, generator=self.generator,
                                                   patches=self.patch_sampler())
            else:
                self.train_dataset = self._dataset("train", "train")
            self.val_dataset = self._dataset("valid", "test")
        if stage == "test" or stage is None:
            self.test_dataset = self._dataset("test", "test")

    def train_dataloader(self):
        return InstanceBatches(self.train_dataset, self.batch_size, shuffle=True, generator=self.generator,
                               collate=collate_3d if self.patch_size is None else collate_patches_3d)

    def val_dataloader(self):
        return InstanceBatches(self.val_dataset, self.batch_size, shuffle=False)

    def test_dataloader(self):
        return InstanceBatches(self.test_dataset, self.batch_size, shuffle=False)
