def __getattr__(name):
    # resolved on first use: data_module imports the trainer, which the 2-D data module imports through this package
    if name == "MiccaiDataModule3D":
        from .data_module import MiccaiDataModule3D
        return MiccaiDataModule3D
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
