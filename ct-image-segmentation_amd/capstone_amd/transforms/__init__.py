"""Device-side 2-D transforms: drop-in names of reference capstone/transforms (transforms_2d.py, predefined.py)."""
from .pipeline2d import BatchPipeline2D, SliceStore2D  # noqa: F401
from .warp2d import ElasticTransform, GridDistortion, WarpPipeline2D  # noqa: F401
