"""The pictures a user looks at (visu/ of the reference): traversability, confidence and segmentation overlays composed by one
fused HIP kernel (csrc/overlay.hip, ops.overlay / overlay_panels / image_to_u8), and the graph and flow views -- lines and ellipses,
bit for bit what PIL.ImageDraw paints -- by a vector rasteriser on the device (csrc/draw.hip, ops.draw).  Importing this package
needs neither PIL nor matplotlib: they are imported where a PNG is written or a colour map is looked up by a name that is not packaged."""
from .image_functionality import image_functionality
from .colormaps import colour_table, default_classification_table
from .visualizer import LearningVisualizer

__all__ = ["LearningVisualizer", "image_functionality", "colour_table", "default_classification_table"]
