"""TorchVisionInterface -- the constructor / ``inference`` contract of
wild_visual_navigation/feature_extractor/torchvision_interface.py (resnet18, return nodes ``layer{1,2,3,4}.1.relu_1`` as
``feat1`` .. ``feat4``), running on the fp32-input MFMA convolutions of csrc/resnet.hip.  tests/resnet_ref.py states the network in
float64; parity with the torchvision package and with a released checkpoint is unpinned (neither is present)."""
import warnings
from collections import OrderedDict
from typing import Dict, List, Tuple

import torch

from .. import _lib, ops

BN_EPS = 1e-5
STAGE_CHANNELS = ops.PYRAMID_CHANNELS


def resnet18_conv_names() -> List[Tuple[str, str]]:
    """(convolution, its BatchNorm) state-dict prefixes in the order the packed image holds them (include/wvn_hip.h)."""
    names = [("conv1", "bn1")]
    for L in range(1, 5):
        names += [(f"layer{L}.0.conv1", f"layer{L}.0.bn1"), (f"layer{L}.0.conv2", f"layer{L}.0.bn2")]
        if L > 1:
            names.append((f"layer{L}.0.downsample.0", f"layer{L}.0.downsample.1"))
        names += [(f"layer{L}.1.conv1", f"layer{L}.1.bn1"), (f"layer{L}.1.conv2", f"layer{L}.1.bn2")]
    return names


def resnet18_conv_shapes() -> Dict[str, Tuple[int, int, int, int]]:
    """conv prefix -> weight shape [Cout, Cin, k, k] of torchvision's resnet18."""
    shapes = {"conv1": (64, 3, 7, 7)}
    for L in range(1, 5):
        c = 64 << (L - 1)
        cin = 64 if L == 1 else c // 2
        shapes[f"layer{L}.0.conv1"] = (c, cin, 3, 3)
        if L > 1:
            shapes[f"layer{L}.0.downsample.0"] = (c, cin, 1, 1)
        for name in (f"layer{L}.0.conv2", f"layer{L}.1.conv1", f"layer{L}.1.conv2"):
            shapes[name] = (c, c, 3, 3)
    return shapes


def synthetic_resnet18_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a resnet18 checkpoint under torchvision's keys: He-scaled convolutions, and BatchNorm layers with non-trivial
    affine terms AND running statistics, so that the folded scale / shift arithmetic is exercised."""
    g = torch.Generator().manual_seed(seed)
    shapes = resnet18_conv_shapes()
    sd = OrderedDict()
    for conv, bn in resnet18_conv_names():
        co, ci, k, _ = shapes[conv]
        sd[conv + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[bn + ".weight"] = 0.5 + torch.rand(co, generator=g)
        sd[bn + ".bias"] = 0.1 * torch.randn(co, generator=g)
        sd[bn + ".running_mean"] = 0.1 * torch.randn(co, generator=g)
        sd[bn + ".running_var"] = 0.5 + torch.rand(co, generator=g)
    return sd


def load_resnet18_state_dict(pretrained_weights) -> Dict[str, torch.Tensor]:
    """A resnet18 state dict from a dict or a checkpoint path, reduced to the keys the network reads (``fc.*`` and
    ``num_batches_tracked`` are ignored).  A missing or mis-shaped key raises a WvnError that names it."""
    if isinstance(pretrained_weights, str):
        sd = torch.load(pretrained_weights, map_location="cpu")
        for key in ("state_dict", "model"):
            if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict):
                sd = sd[key]
    elif isinstance(pretrained_weights, dict):
        sd = pretrained_weights
    else:
        raise _lib.WvnError(f"pretrained_weights must be a path or a state dict, not {type(pretrained_weights).__name__}")
    sd = {k.replace("module.", "", 1) if k.startswith("module.") else k: v for k, v in sd.items()}
    shapes = resnet18_conv_shapes()
    out = OrderedDict()
    for conv, bn in resnet18_conv_names():
        want = {conv + ".weight": shapes[conv]}
        for p in ("weight", "bias", "running_mean", "running_var"):
            want[f"{bn}.{p}"] = (shapes[conv][0],)
        for key, shape in want.items():
            if key not in sd:
                raise _lib.WvnError(f"pretrained_weights: resnet18 key '{key}' is missing")
            if tuple(sd[key].shape) != shape:
                raise _lib.WvnError(f"pretrained_weights: '{key}' has shape {tuple(sd[key].shape)}, resnet18 needs {shape}")
            out[key] = sd[key].detach().to("cpu", torch.float32)
    return out


class TorchVisionInterface:
    def __init__(self, device: str, model_type: str, input_size: int = 448, pretrained: bool = True, pretrained_weights=None,
                 allow_synthetic: bool = False):
        # refusals first: nothing below them touches the GPU
        if model_type != "resnet18":
            raise _lib.WvnError(f"model_type '{model_type}' is not supported by the MI355X path: only 'resnet18' (resnet50, resnet50_dino "
                                f"and the EfficientNets need bottleneck or depthwise blocks)")
        if not isinstance(input_size, int) or input_size < 32 or input_size % 32:
            raise _lib.WvnError(f"input_size={input_size} must be a positive multiple of 32 (the stride of the last ResNet-18 stage)")
        self._device = torch.device(device)
        if self._device.type != "cuda":
            raise _lib.WvnError(f"device '{device}': TorchVisionInterface runs on a GPU; the HIP path has no CPU fallback")
        self._model_type = model_type
        self._input_size = input_size
        self._pretrained = pretrained
        if pretrained_weights is None:
            if not allow_synthetic:
                warnings.warn("TorchVisionInterface: no pretrained_weights given -- running with seeded SYNTHETIC resnet18 weights (the "
                              "reference downloads the released checkpoint; there is no network here): shapes and speed are real, the "
                              "features are meaningless.  Pass pretrained_weights=<path | state dict> or allow_synthetic=True to silence",
                              stacklevel=2)
            self._state_dict = synthetic_resnet18_state_dict()
        else:
            self._state_dict = load_resnet18_state_dict(pretrained_weights)
        self._packed = None       # the packed image on the GPU, built at the first frame (construction stays host-only)
        self._workspace = None    # level maps + temporaries of the last batch size
        self._workspace_batch = 0
        self._levels = None

    # ---------------------------------------------------------------------------------------------------------------------
    def _pack(self):
        sd = self._state_dict
        weights, scales, shifts = [], [], []
        for conv, bn in resnet18_conv_names():
            scale, shift = ops.bn_scale_shift(sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"], BN_EPS)
            weights.append(sd[conv + ".weight"].to(self._device))
            scales.append(scale.to(self._device))
            shifts.append(shift.to(self._device))
        self._packed = ops.resnet18_pack(weights, scales, shifts)

    def change_device(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.WvnError(f"device '{device}': TorchVisionInterface runs on a GPU; the HIP path has no CPU fallback")
        self._device = device
        self._packed = self._workspace = self._levels = None
        self._workspace_batch = 0

    def check_frames(self, img: torch.Tensor, who: str = "TorchVisionInterface"):
        """Frames must already have the network's size: the nodes' resize_image delivers it, the reference's bilinear T.Resize is not
        rebuilt.  Refused before any GPU work."""
        s = self._input_size
        if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != s or img.shape[3] != s:
            raise _lib.WvnError(f"{who}: img must be [B,3,{s},{s}] (input_size={s}; frames are not resized here), not {tuple(img.shape)}")

    @torch.no_grad()
    def forward_levels(self, img: torch.Tensor):
        """img [B,3,S,S] (fp32 in [0,1] or uint8) -> the four NHWC level maps [B,S/s,S/s,C], views of this object's workspace (valid until
        the next call)."""
        self.check_frames(img)
        img = img.to(self._device)
        if self._packed is None:
            self._pack()
        B = img.shape[0]
        if self._workspace is None or self._workspace_batch != B:
            self._workspace = ops.resnet18_workspace(B, self._input_size, self._input_size, self._device)
            self._workspace_batch = B
        self._levels, _ = ops.resnet18_forward(self._packed, img, self._workspace)
        return self._levels

    @torch.no_grad()
    def inference(self, img: torch.Tensor):
        """torchvision_interface.py of the reference: the ordered dict feat1 .. feat4 of NCHW fp32 maps (copies)."""
        levels = self.forward_levels(img)
        return OrderedDict((f"feat{i + 1}", m.permute(0, 3, 1, 2).contiguous()) for i, m in enumerate(levels))

    def forward(self, img: torch.Tensor):
        return self.inference(img)

    __call__ = forward

    @property
    def input_size(self):
        return self._input_size

    @property
    def model_type(self):
        return self._model_type

    @property
    def feature_dim(self):
        return ops.PYRAMID_DIM
