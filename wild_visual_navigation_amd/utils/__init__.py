from .data import Data, Batch
from .confidence_generator import ConfidenceGenerator
from .loss import TraversabilityLoss, AnomalyLoss
from .meshes import make_plane, make_dense_plane, make_polygon_from_points
from .operation_modes import WVNMode
from .metrics import BinaryROC, BinaryAUROC, BinaryAccuracy
from .metric_logger import MetricLogger
from .image_io import compressed_image_to_torch, image_to_torch

__all__ = ["Data", "Batch", "ConfidenceGenerator", "TraversabilityLoss", "AnomalyLoss", "make_plane", "make_dense_plane",
           "make_polygon_from_points", "WVNMode", "BinaryROC", "BinaryAUROC", "BinaryAccuracy", "MetricLogger",
           "compressed_image_to_torch", "image_to_torch"]
