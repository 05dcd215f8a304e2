"""The definition the ResNet-18 pyramid kernels (csrc/resnet.hip, csrc/pyramid_pool.hip) are held to, in plain torch; float64 by default.

Network: torchvision's ``resnet18`` in eval mode written out with F.conv2d / F.batch_norm / F.max_pool2d / relu, on the frame normalised
with T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]); the outputs are the reference's return nodes ``layer{1,2,3,4}.1.relu_1``
(the outputs of the four stages) as ``feat1`` .. ``feat4`` [B, C, h, w].  State dict: torchvision's keys.

Pooling (feature_extractor.py:314-366 of the reference, the multi-scale branch), per level with stride s:
  seg_s = F.interpolate(seg, scale_factor=1/s) (nearest) = seg[::s, ::s]; row i = the mean of the level's vectors over the cells where
  seg_s == i.
  Fallback, where the published code cannot run (it calls ``.type`` on a Python float): no cell of the level carries id i -> the vector
  of the cell (min(cy // s, h - 1), min(cx // s, w - 1)), cy = floor(sum of the segment's pixel rows / its pixel count) at full
  resolution in integers, cx likewise.
  An id below S without a pixel: a NaN row in all four blocks.  Negative ids are ignored.

``dtype=torch.float32`` runs the same statements in fp32: the yardstick the GPU's error is measured against.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5
STRIDES = (4, 8, 16, 32)
CHANNELS = (64, 128, 256, 512)


def normalize(img: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[B,3,H,W] fp32 in [0,1] or uint8 (v / 255 first) -> the normalised frame."""
    x = img.to(dtype) / 255 if img.dtype == torch.uint8 else img.to(dtype)
    mean = torch.tensor(MEAN, dtype=dtype, device=img.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype, device=img.device).view(1, 3, 1, 1)
    return (x - mean) / std


def bn_scale_shift(weight, bias, running_mean, running_var, eps=BN_EPS):
    """Eval-mode BatchNorm as y = x * scale + shift, float64."""
    w, b, m, v = (t.to(torch.float64) for t in (weight, bias, running_mean, running_var))
    scale = w / torch.sqrt(v + eps)
    return scale, b - m * scale


def _bn(x, sd, name, dtype):
    return F.batch_norm(x, sd[name + ".running_mean"].to(dtype), sd[name + ".running_var"].to(dtype), sd[name + ".weight"].to(dtype),
                        sd[name + ".bias"].to(dtype), training=False, eps=BN_EPS)


def conv_bn_act(x, weight, bn, stride, pad, residual=None, relu=True, dtype=torch.float64):
    """x [B,Cin,H,W] -> relu(batch_norm(conv2d(x)) + residual); bn = (weight, bias, running_mean, running_var)."""
    y = F.conv2d(x.to(dtype), weight.to(dtype), stride=stride, padding=pad)
    y = F.batch_norm(y, bn[2].to(dtype), bn[3].to(dtype), bn[0].to(dtype), bn[1].to(dtype), training=False, eps=BN_EPS)
    if residual is not None:
        y = y + residual.to(dtype)
    return F.relu(y) if relu else y


def conv_affine_act(x, weight, scale, shift, stride, pad, residual=None, relu=True, dtype=torch.float64):
    """The same with the folded terms given as they are: relu(conv2d(x) * scale[c] + shift[c] + residual).  On integer inputs with
    scale in {0.5, 1, 2, -1} every intermediate is an integer or a half: exact in float64 and, below 2^24, in fp32 too."""
    y = F.conv2d(x.to(dtype), weight.to(dtype), stride=stride, padding=pad)
    y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.to(dtype)
    return F.relu(y) if relu else y


def _basic_block(x, sd, name, stride, dtype):
    out = F.relu(_bn(F.conv2d(x, sd[name + ".conv1.weight"].to(dtype), stride=stride, padding=1), sd, name + ".bn1", dtype))
    out = _bn(F.conv2d(out, sd[name + ".conv2.weight"].to(dtype), stride=1, padding=1), sd, name + ".bn2", dtype)
    if name + ".downsample.0.weight" in sd:
        x = _bn(F.conv2d(x, sd[name + ".downsample.0.weight"].to(dtype), stride=stride), sd, name + ".downsample.1", dtype)
    return F.relu(out + x)


def resnet18(sd, img: torch.Tensor, dtype=torch.float64) -> "OrderedDict[str, torch.Tensor]":
    x = normalize(img, dtype)
    x = F.relu(_bn(F.conv2d(x, sd["conv1.weight"].to(dtype), stride=2, padding=3), sd, "bn1", dtype))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    out = OrderedDict()
    for L in range(1, 5):
        x = _basic_block(x, sd, f"layer{L}.0", 1 if L == 1 else 2, dtype)
        x = _basic_block(x, sd, f"layer{L}.1", 1, dtype)
        out[f"feat{L}"] = x
    return out


def centroid(seg: torch.Tensor, i: int):
    """(cy, cx) of id i in seg [H,W]: floor(sum of pixel rows / pixel count), in integers; None for an id without a pixel."""
    ys, xs = torch.nonzero(seg == i, as_tuple=True)
    n = ys.numel()
    if n == 0:
        return None
    return int(ys.sum().item()) // n, int(xs.sum().item()) // n


def pyramid_pool(levels, seg: torch.Tensor, n_seg: int, dtype=torch.float64):
    """levels: four maps [C,h,w] of ONE frame (strides 4, 8, 16, 32), seg [H,W] integer -> (feat [n_seg, sum C] in ``dtype``,
    fallback [n_seg, 4] bool: the (segment, level) pairs that took the centroid cell)."""
    seg = seg.to(torch.int64)
    H, W = seg.shape
    blocks = []
    fallback = torch.zeros(n_seg, len(levels), dtype=torch.bool)
    for l, (m, s) in enumerate(zip(levels, STRIDES)):
        m = m.to(dtype)
        Cc, h, w = m.shape
        assert (h, w) == (H // s, W // s)
        seg_s = F.interpolate(seg[None, None].to(torch.float64), scale_factor=1 / s)[0, 0].to(torch.int64)
        assert torch.equal(seg_s, seg[::s, ::s])
        block = torch.full((n_seg, Cc), float("nan"), dtype=dtype)
        for i in range(n_seg):
            mask = seg_s == i
            if mask.any():
                block[i] = m[:, mask].sum(dim=1) / int(mask.sum())
                continue
            c = centroid(seg, i)
            if c is None:
                continue
            fallback[i, l] = True
            block[i] = m[:, min(c[0] // s, h - 1), min(c[1] // s, w - 1)]
        blocks.append(block)
    return torch.cat(blocks, dim=1), fallback
