"""Mirror of reference capstone/volumetric/losses.py:119-130 (the 3-D loss registry + wrapper)."""
from ..models.losses import LOSSES, WEIGHT, MultipleLossWrapper  # noqa: F401


class MultipleLossWrapper3D(MultipleLossWrapper):
    def __init__(self, losses, exclude_missing=False, device_boundary=False):
        """``device_boundary``: as ``MultipleLossWrapper``; ``forward`` then takes ``dist_maps`` (B, C-1, H, W, D), the fourth batch
        element of ``MiccaiDataset3D(dist_maps=True)``"""
        super(MultipleLossWrapper3D, self).__init__(losses, exclude_missing, device_boundary)
