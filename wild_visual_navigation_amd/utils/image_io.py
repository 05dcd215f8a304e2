"""Camera messages -> frames in device memory (the reference's wild_visual_navigation_ros/ros_converter.py: ros_image_to_torch)."""
import torch

from .. import ops


def compressed_image_to_torch(data, fmt: str = "", device="cuda", as_float: bool = False) -> torch.Tensor:
    """The CompressedImage branch of ros_image_to_torch (ros_converter.py:117-126) on the GPU: ``data`` is ``msg.data`` (the JPEG
    bytes), ``fmt`` is ``msg.format`` -> [3,H,W] on ``device``.

    The channel order is the reference's, quirk included: cv2.imdecode yields BGR, and the reference swaps to RGB only when
    "bgr" occurs in the format string.  So "bgr8; jpeg compressed bgr8" gives RGB, and "rgb8; jpeg compressed" (or an empty
    format) gives the decoded picture with R and B exchanged, exactly as the reference hands it on.

    uint8 by default (what FeatureExtractor takes); ``as_float=True`` gives the reference's ToTensor result: fp32, value / 255 as the
    CPU rounds it (a 256-entry table of the correctly rounded quotients: the GPU's own division differs in the last bit).
    Baseline JPEG only (ops.jpeg_decode); a PNG-compressed message or a refused stream raises WvnError."""
    rgb = ops.jpeg_decode(data, device, strict=True)[0][0]
    img = rgb if "bgr" in fmt else rgb.flip(0)
    if not as_float:
        return img.contiguous()
    return (torch.arange(256, dtype=torch.float32) / 255).to(img.device)[img.long()]
