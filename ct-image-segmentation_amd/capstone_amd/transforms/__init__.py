"""Device-side 2-D transforms: drop-in names of reference capstone/transforms (transforms_2d.py, predefined.py); and the
post-processing transforms of label maps, under MONAI's names."""
from ..components import FillHoles, KeepLargestConnectedComponent  # noqa: F401
from .pipeline2d import BatchPipeline2D, SliceStore2D  # noqa: F401
from .warp2d import ElasticTransform, GridDistortion, WarpPipeline2D  # noqa: F401
