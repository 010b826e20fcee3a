"""The presets of reference capstone/transforms/predefined.py that are per-pixel and index arithmetic, as ``BatchPipeline2D``
objects: ``windowed_degree_1``, ``windowed_degree_2`` and the ``"test"`` side of every degree.  The ``"train"`` sides of
``degree_0``, ``windowed_degree_3`` and ``windowed_degree_4`` warp the slice (``A.ElasticTransform`` / ``A.GridDistortion``): asking
for one raises ``NotImplementedError`` — it is not downgraded to a crop.
"""
from .pipeline2d import BatchPipeline2D
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
            raise NotImplementedError(f"{self.name}['train'] warps the slice (ElasticTransform / GridDistortion): not carried to the "
                                      "device pipeline, and not replaced by a weaker augmentation")
        raise KeyError(key)


windowed_degree_1 = _Preset("windowed_degree_1", _minimal_windowed_transform, _minimal_windowed_transform)
windowed_degree_2 = _Preset("windowed_degree_2", BatchPipeline2D(_stacked_windows, "crop", _SIZE, _stacked_window_stats["mean"],
                                                                 _stacked_window_stats["std"]), _minimal_windowed_transform)
windowed_degree_3 = _Preset("windowed_degree_3", None, _minimal_windowed_transform)
windowed_degree_4 = _Preset("windowed_degree_4", None, _minimal_windowed_transform)
degree_0 = _Preset("degree_0", None, _minimal_transform)
