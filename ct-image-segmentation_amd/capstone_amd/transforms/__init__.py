"""Device-side 2-D transforms: drop-in names of reference capstone/transforms (transforms_2d.py, predefined.py); and the
post-processing transform of label maps, under MONAI's name."""
from ..components import KeepLargestConnectedComponent  # noqa: F401
from .pipeline2d import BatchPipeline2D, SliceStore2D  # noqa: F401
from .warp2d import ElasticTransform, GridDistortion, WarpPipeline2D  # noqa: F401
