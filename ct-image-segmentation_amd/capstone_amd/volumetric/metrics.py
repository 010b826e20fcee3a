"""Mirror of reference capstone/volumetric/metrics.py: the 3-D metric wrapper (rank-agnostic here)."""
from ..models.metrics import DiceMetricWrapper, SurfaceDiceMetricWrapper, SurfaceDistanceMetricWrapper


class DiceMetricWrapper3D(DiceMetricWrapper):
    pass


class SurfaceDistanceMetricWrapper3D(SurfaceDistanceMetricWrapper):
    pass


class SurfaceDiceMetricWrapper3D(SurfaceDiceMetricWrapper):
    pass
