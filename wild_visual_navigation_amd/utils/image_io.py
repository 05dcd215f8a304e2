"""Camera messages -> frames in device memory (the reference's wild_visual_navigation_ros/ros_converter.py: ros_image_to_torch)."""
import torch

from .. import _lib, ops

# sensor_msgs/image_encodings.h names that are NOT taken: 16-bit, alpha, float and the generic CvMat types
_REFUSED_HINT = "16-bit, alpha, float and generic (8UC1 ...) encodings are refused"
RAW_ENCODINGS = tuple(k for k in _lib.SRC_KINDS if k != "planar")
DESIRED_ENCODINGS = ("rgb8", "bgr8", "passthrough")


def image_plan(encoding: str, desired_encoding: str = "rgb8"):
    """(channels, bgr) of what image_to_torch returns for a message of ``encoding``; WvnError naming what is refused.  "rgb8" /
    "bgr8": three planes in that order (mono8: the plane three times, as cv_bridge's conversion gives).  "passthrough": the message's
    own form -- mono8 one plane, rgb8 R,G,B, bgr8 B,G,R; a mosaic has no colour order of its own and is demosaiced to R,G,B (cv_bridge
    would hand on the raw mosaic, which nothing downstream takes)."""
    if encoding not in RAW_ENCODINGS:
        raise _lib.WvnError(f"image_to_torch: encoding {encoding!r} is not supported ({_REFUSED_HINT}); "
                            f"the encodings are {', '.join(RAW_ENCODINGS)}")
    if desired_encoding not in DESIRED_ENCODINGS:
        raise _lib.WvnError(f"image_to_torch: desired_encoding {desired_encoding!r} is not one of {', '.join(DESIRED_ENCODINGS)}")
    if desired_encoding == "passthrough":
        return (1, False) if encoding == "mono8" else (3, encoding == "bgr8")
    return 3, desired_encoding == "bgr8"


def check_raw_geometry(encoding: str, height: int, width: int, step=None, rectify=None, who: str = "image_to_torch") -> int:
    """The host-side refusals of a raw frame's description -> step in bytes (default: width x bytes per pixel)."""
    if encoding not in RAW_ENCODINGS:
        raise _lib.WvnError(f"{who}: encoding {encoding!r} is not supported ({_REFUSED_HINT}); "
                            f"the encodings are {', '.join(RAW_ENCODINGS)}")
    bpp = 3 if encoding in ("rgb8", "bgr8") else 1
    least = 3 if encoding.startswith("bayer") else 1
    height, width = int(height), int(width)
    if not (least <= height <= _lib.FRAME_MAX_DIM and least <= width <= _lib.FRAME_MAX_DIM):
        raise _lib.WvnError(f"{who}: a {encoding} frame of {height} x {width}: each side must lie in [{least}, {_lib.FRAME_MAX_DIM}]")
    step = width * bpp if step is None else int(step)
    if step < width * bpp:
        raise _lib.WvnError(f"{who}: step={step} is smaller than a row of {width} pixels ({width * bpp} bytes)")
    if height * step >= 2 ** 31:
        raise _lib.WvnError(f"{who}: height * step = {height * step} bytes leaves 31 bits")
    if rectify is not None:
        if not isinstance(rectify, ops.RectifyMap):
            raise _lib.WvnError(f"{who}: rectify must be a RectifyMap (ops.rectify_map), got {type(rectify).__name__}")
        if rectify.src_size != (height, width):
            raise _lib.WvnError(f"{who}: the map is for {rectify.src_size[0]} x {rectify.src_size[1]} frames, "
                                f"the message is {height} x {width}")
    return step


def image_to_torch(data, encoding: str, height: int, width: int, step=None, device="cuda", desired_encoding: str = "rgb8",
                   rectify=None) -> torch.Tensor:
    """The sensor_msgs/Image branch of ros_image_to_torch (ros_converter.py:113-116: cv_bridge's imgmsg_to_cv2) on the GPU: ``data``
    is ``msg.data`` (bytes, bytearray or a 1-d uint8 CPU tensor), the other arguments are the message's fields -> uint8 [C,H,W] on
    ``device``.  One upload of height x step bytes, one launch: mono8, rgb8, bgr8 and the four 8-bit Bayer mosaics (bilinear
    demosaic), padded rows honoured.  ``rectify``: a RectifyMap (ops.rectify_map / rectify_map_from_camera_info) -- the frame comes
    out undistorted at the map's output size, demosaiced at the taps of the same launch.  Channel order and count: image_plan."""
    channels, bgr = image_plan(encoding, desired_encoding)
    step = check_raw_geometry(encoding, height, width, step, rectify)
    raw = ops.upload_raw_frames(data, height * step, device, "image_to_torch")
    if raw.shape[0] != 1:
        raise _lib.WvnError(f"image_to_torch: one message expected, got {raw.shape[0]} (FeatureExtractor.decode_raw takes a list)")
    raw = raw.view(1, height, step)
    if rectify is None:
        return ops.unpack_frames(raw, encoding, step=step, width=width, bgr=bgr, channels=channels)[0]
    return ops.rectify(raw, rectify, encoding, step=step, width=width, bgr=bgr, channels=channels)[0]


def compressed_image_to_torch(data, fmt: str = "", device="cuda", as_float: bool = False, rectify=None) -> torch.Tensor:
    """The CompressedImage branch of ros_image_to_torch (ros_converter.py:117-126) on the GPU: ``data`` is ``msg.data`` (the JPEG
    bytes), ``fmt`` is ``msg.format`` -> [3,H,W] on ``device``.

    The channel order is the reference's, quirk included: cv2.imdecode yields BGR, and the reference swaps to RGB only when
    "bgr" occurs in the format string.  So "bgr8; jpeg compressed bgr8" gives RGB, and "rgb8; jpeg compressed" (or an empty
    format) gives the decoded picture with R and B exchanged, exactly as the reference hands it on.

    uint8 by default (what FeatureExtractor takes); ``as_float=True`` gives the reference's ToTensor result: fp32, value / 255 as the
    CPU rounds it (a 256-entry table of the correctly rounded quotients: the GPU's own division differs in the last bit).
    Baseline JPEG only (ops.jpeg_decode); a PNG-compressed message or a refused stream raises WvnError.
    ``rectify``: a RectifyMap -- the decoded frame is undistorted (ops.rectify) in the same channel order, [3,h,w]."""
    rgb = ops.jpeg_decode(data, device, strict=True)[0][0]
    if rectify is None:
        img = (rgb if "bgr" in fmt else rgb.flip(0)).contiguous()
    else:
        img = ops.rectify(rgb, rectify, "planar", bgr="bgr" not in fmt)[0]
    if not as_float:
        return img
    return (torch.arange(256, dtype=torch.float32) / 255).to(img.device)[img.long()]
