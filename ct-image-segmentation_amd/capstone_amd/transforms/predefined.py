"""The presets of reference capstone/transforms/predefined.py that are per-pixel and index arithmetic, as ``BatchPipeline2D``
objects: ``windowed_degree_1``, ``windowed_degree_2`` and the ``"test"`` side of every degree.  The ``"train"`` sides of
``degree_0``, ``windowed_degree_3`` and ``windowed_degree_4`` warp the slice (``A.ElasticTransform`` / ``A.GridDistortion``): asking
for one raises ``NotImplementedError`` — it is not downgraded to a crop.  ``warped`` holds the device restatement of those three
presets (``WarpPipeline2D``; its parity with OpenCV is unpinned, which is why it is opted into: ``device_warps=True`` on the data
modules, or ``predefined.warped[name]`` directly).
"""
from .pipeline2d import BatchPipeline2D
from .warp2d import ElasticTransform, GridDistortion, WarpPipeline2D
from .transforms_2d import WINDOWING_CONFIG

_stacked_window_stats = {"mean": (0.107, 0.135, 0.085), "std": (0.271, 0.267, 0.152)}
_stacked_windows = [WINDOWING_CONFIG[w] for w in ("brain", "soft_tissue", "bone")]
_SIZE = (256, 256)

_minimal_windowed_transform = BatchPipeline2D(_stacked_windows, "resize", _SIZE, _stacked_window_stats["mean"],
                                              _stacked_window_stats["std"])
_minimal_transform = BatchPipeline2D([WINDOWING_CONFIG["soft_tissue"]], "resize", _SIZE, _stacked_window_stats["mean"][1],
                                     _stacked_window_stats["std"][1])


class _Preset(dict):
    """{"train": ..., "test": ...} whose refused sides raise when they are asked for"""

    def __init__(self, name, train, test):
        super().__init__(test=test)
        self.name = name
        if train is not None:
            self["train"] = train

    def __missing__(self, key):
        if key == "train":
            raise NotImplementedError(f"{self.name}['train'] warps the slice (ElasticTransform / GridDistortion): its device "
                                      f"restatement is opt-in (device_warps=True on the data modules, or predefined.warped['{self.name}']), "
                                      "and it is not replaced by a weaker augmentation")
        raise KeyError(key)


windowed_degree_1 = _Preset("windowed_degree_1", _minimal_windowed_transform, _minimal_windowed_transform)
windowed_degree_2 = _Preset("windowed_degree_2", BatchPipeline2D(_stacked_windows, "crop", _SIZE, _stacked_window_stats["mean"],
                                                                 _stacked_window_stats["std"]), _minimal_windowed_transform)
windowed_degree_3 = _Preset("windowed_degree_3", None, _minimal_windowed_transform)
windowed_degree_4 = _Preset("windowed_degree_4", None, _minimal_windowed_transform)
degree_0 = _Preset("degree_0", None, _minimal_transform)


def _warp(windows, mean, std, warps, oneof, rot_flip):
    return WarpPipeline2D(windows, _SIZE, mean, std, warps=warps, oneof=oneof, rot_flip=rot_flip)


_soft = [WINDOWING_CONFIG["soft_tissue"]]
# the "train" sides that warp, after RandomCrop(256, 256): degree 3 ElasticTransform() then RandomRotate90 and HorizontalFlip;
# degree 4 and degree 0 OneOf([ElasticTransform(), GridDistortion()]) and neither rotation nor flip
warped = {
    "degree_0": {"train": _warp(_soft, _stacked_window_stats["mean"][1], _stacked_window_stats["std"][1],
                                [ElasticTransform(), GridDistortion()], True, False), "test": _minimal_transform},
    "windowed_degree_3": {"train": _warp(_stacked_windows, _stacked_window_stats["mean"], _stacked_window_stats["std"],
                                         [ElasticTransform()], False, True), "test": _minimal_windowed_transform},
    "windowed_degree_4": {"train": _warp(_stacked_windows, _stacked_window_stats["mean"], _stacked_window_stats["std"],
                                         [ElasticTransform(), GridDistortion()], True, False), "test": _minimal_windowed_transform},
}
