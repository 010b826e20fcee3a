_TTA = ("TestTimeAugmenter3D", "tta_accumulate", "tta_finish", "view_to_target_matrix", "class_channel_src", "mirror_views")


def __getattr__(name):
    # resolved on first use: data_module imports the trainer, which the 2-D data module imports through this package
    if name == "MiccaiDataModule3D":
        from .data_module import MiccaiDataModule3D
        return MiccaiDataModule3D
    if name in _TTA:
        from . import tta
        return getattr(tta, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
