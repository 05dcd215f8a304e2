"""Functional wrappers (torch tensors in / out) around the C-ABI kernels of libwvn_hip.so.
Allocation and stream selection happen here; arithmetic happens in HIP.  No fallbacks."""
import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib, ptr, require_cuda, stream


def _i32(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.int32 else t.to(torch.int32)


def upsample_bilinear(tokens: torch.Tensor, grid: int, out_size: int) -> torch.Tensor:
    """tokens [B,G*G,D] fp32 -> dense [B,D,H,H] (align_corners=True; dino_interface.py:87-90)."""
    require_cuda(tokens, "tokens")
    tokens = tokens.contiguous()
    B, P, D = tokens.shape
    out = torch.empty(B, D, out_size, out_size, dtype=torch.float32, device=tokens.device)
    check(lib().wvn_upsample_bilinear(ptr(tokens), ptr(out), B, grid, D, out_size, stream()), "wvn_upsample_bilinear")
    return out


def random_pixels(batch: int, H: int, W: int, nr: int, seed: int = 0, frame0: int = 0, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """segmentation_type "random" (feature_extractor.py:227-235) for a batch, without a permutation of the frame: image b draws
    ``nr`` distinct pixels from the key (seed, frame0 + b) (both taken modulo 2^32) -> (idx [B,nr] int32 row-major pixel indices,
    seg [B,H,W] int32: j at idx[b, j], -1 elsewhere).  A function of the key and H*W alone (tests/random_pixels_ref.py)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.WvnError(f"random_pixels: device must be a GPU (got {device}); the HIP path has no CPU fallback")
    if not (1 <= nr <= H * W):
        raise _lib.WvnError(f"random_pixels: n_random_pixels={nr} must lie in [1, H*W={H * W}]")
    idx = torch.empty(batch, nr, dtype=torch.int32, device=device)
    seg = torch.empty(batch, H, W, dtype=torch.int32, device=device)
    check(lib().wvn_random_pixels(int(seed) & 0xFFFFFFFF, int(frame0) & 0xFFFFFFFF, batch, H, W, nr, ptr(idx), ptr(seg), stream()),
          "wvn_random_pixels")
    return idx, seg


def gather_bilinear(tokens: torch.Tensor, idx: torch.Tensor, grid: int, out_size: int) -> torch.Tensor:
    """tokens [B,G*G,D] fp32, idx [B,nr] pixel indices y * H + x of the H x H map (any order, duplicates allowed) -> feat [B,nr,D]:
    ``upsample_bilinear(tokens, grid, out_size).reshape(B, D, H*H)[b, :, idx[b]].T`` bit for bit, from four token rows per sample
    (feature_extractor.py:96-111).  An index outside the map gives a NaN row."""
    require_cuda(tokens, "tokens")
    require_cuda(idx, "idx")
    if tokens.dim() != 3 or idx.dim() != 2 or idx.shape[0] != tokens.shape[0] or tokens.shape[1] != grid * grid or out_size < 1:
        raise _lib.WvnError(f"gather_bilinear: tokens [B,{grid}*{grid},D] and idx [B,nr] expected, got {tuple(tokens.shape)} and {tuple(idx.shape)}")
    if tokens.dtype != torch.float32:
        raise _lib.WvnError(f"gather_bilinear: fp32 tokens expected, got {tokens.dtype}")
    tokens = tokens.contiguous()
    idx = _i32(idx).contiguous()
    B, _, D = tokens.shape
    nr = idx.shape[1]
    feat = torch.empty(B, nr, D, dtype=torch.float32, device=tokens.device)
    check(lib().wvn_gather_bilinear(ptr(tokens), ptr(idx), ptr(feat), B, grid, out_size, D, nr, stream()), "wvn_gather_bilinear")
    return feat


DENSE_SIFT_DIM = 128              # descriptor length per image channel (8 angular x 4 x 4 spatial bins)


def _sift_frames(img: torch.Tensor, who: str) -> torch.Tensor:
    require_cuda(img, "img")
    if img.dim() != 4 or img.shape[1] not in (1, 3) or img.shape[2] < 4 or img.shape[3] < 4:
        raise _lib.WvnError(f"{who}: img must be [B,C,H,W] with C in (1, 3) and H, W >= 4, not {tuple(img.shape)}")
    return img.contiguous() if img.dtype == torch.uint8 else img.contiguous().float()


def dense_sift(img: torch.Tensor) -> torch.Tensor:
    """Dense SIFT descriptors (feature_type "sift"; feature_extractor.py:276-286 of the reference): img [B,C,H,W] fp32 in [0,1] or
    uint8 (x / 255 fused into the load), C in (1, 3), any H, W >= 4 -> [B, 128 C, H, W] fp32, channel c of the frame in columns
    [128 c, 128 c + 128).  The definition: include/wvn_hip.h, tests/dense_sift_ref.py."""
    img = _sift_frames(img, "dense_sift")
    B, Cc, H, W = img.shape
    out = torch.empty(B, DENSE_SIFT_DIM * Cc, H, W, dtype=torch.float32, device=img.device)
    check(lib().wvn_dense_sift(ptr(img), int(img.dtype == torch.uint8), ptr(out), B, Cc, H, W, stream()), "wvn_dense_sift")
    return out


def dense_sift_segpool(img: torch.Tensor, seg: torch.Tensor, n_seg: int, return_counts: bool = False):
    """Per-segment means of ``dense_sift(img)`` without the dense map: img [B,C,H,W], seg [B,H,W] int (ids outside [0, n_seg), -1
    included, are ignored) -> feat [B, n_seg, 128 C] fp32, NaN row for an id without a pixel.  feat is
    float32(sum trunc(dense * 2^32) / (count * 2^32)) over the very bits ``dense_sift`` returns, summed in 64-bit integers: the same
    result whatever the order of the atomics.  ``return_counts``: also the pixels per id, [B, n_seg] int32."""
    img = _sift_frames(img, "dense_sift_segpool")
    require_cuda(seg, "seg")
    B, Cc, H, W = img.shape
    if tuple(seg.shape) != (B, H, W):
        raise _lib.WvnError(f"dense_sift_segpool: seg must be [B,H,W] = {(B, H, W)}, not {tuple(seg.shape)}")
    if n_seg < 1:
        raise _lib.WvnError(f"dense_sift_segpool: n_seg={n_seg} must be >= 1")
    seg = _i32(seg).contiguous()
    D = DENSE_SIFT_DIM * Cc
    feat = torch.empty(B, n_seg, D, dtype=torch.float32, device=img.device)
    cnt = torch.empty(B, n_seg, dtype=torch.int32, device=img.device)
    ssum = torch.empty(B * n_seg * D, dtype=torch.int64, device=img.device)   # 2^-32 fixed-point sums (cleared by the call)
    check(lib().wvn_dense_sift_segpool(ptr(img), int(img.dtype == torch.uint8), ptr(seg), ptr(feat), ptr(cnt), ptr(ssum), B, Cc, H, W,
                                       int(n_seg), stream()), "wvn_dense_sift_segpool")
    return (feat, cnt) if return_counts else feat


CONV_IN_NHWC, CONV_IN_FRAME_F32, CONV_IN_FRAME_U8 = 0, 1, 2   # include/wvn_hip.h: WVN_CONV_IN_*
RESNET18_NCONV = 20
PYRAMID_CHANNELS = (64, 128, 256, 512)   # ResNet-18 stages at strides 4, 8, 16, 32
PYRAMID_DIM = sum(PYRAMID_CHANNELS)      # 960


def bn_scale_shift(weight, bias, running_mean, running_var, eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval-mode BatchNorm folded to y = x * scale + shift: formed in float64 on the host, then rounded to fp32 (CPU tensors)."""
    w, b, m, v = (t.detach().to("cpu", torch.float64) for t in (weight, bias, running_mean, running_var))
    scale = w / torch.sqrt(v + eps)
    return scale.float(), (b - m * scale).float()


def conv2d_pack(weight: torch.Tensor) -> torch.Tensor:
    """weight [Cout,Cin,k,k] fp32 on the GPU -> the packed [Kpad,Cout] image ``conv2d_bn_act`` reads (k = (ky, kx, cin) major)."""
    require_cuda(weight, "weight")
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.dtype != torch.float32:
        raise _lib.WvnError(f"conv2d_pack: weight must be fp32 [Cout,Cin,k,k], not {weight.dtype} {tuple(weight.shape)}")
    Cout, Cin, k, _ = weight.shape
    n = lib().wvn_conv2d_pack_floats(Cout, Cin, k)
    if n == 0:
        raise _lib.WvnError(f"conv2d_pack: unsupported shape {tuple(weight.shape)}")
    packed = torch.empty(n // Cout, Cout, dtype=torch.float32, device=weight.device)
    check(lib().wvn_conv2d_pack(ptr(weight.contiguous()), ptr(packed), Cout, Cin, k, stream()), "wvn_conv2d_pack")
    return packed


def conv2d_bn_act(x: torch.Tensor, packed: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, ksize: int, stride: int, pad: int,
                  residual: Optional[torch.Tensor] = None, relu: bool = True, frame: bool = False) -> torch.Tensor:
    """Convolution + folded BatchNorm (+ residual) (+ ReLU) on the fp32-input MFMA (csrc/resnet.hip).  x: an NHWC fp32 activation
    [B,H,W,Cin] (Cin % 32 == 0), or with ``frame=True`` an NCHW frame [B,3,H,W] (fp32 in [0,1] or uint8) that is normalised with the
    ImageNet mean / std on load (the stem).  packed: ``conv2d_pack(weight)``.  Returns NHWC [B,OH,OW,Cout]; residual has that shape."""
    for t, n in ((x, "x"), (packed, "packed"), (scale, "scale"), (shift, "shift")):
        require_cuda(t, n)
    if x.dim() != 4:
        raise _lib.WvnError(f"conv2d_bn_act: x must have four dimensions, not {tuple(x.shape)}")
    if frame:
        B, Cin, H, W = x.shape
        kind = CONV_IN_FRAME_U8 if x.dtype == torch.uint8 else CONV_IN_FRAME_F32
        x = x.contiguous() if x.dtype == torch.uint8 else x.contiguous().float()
    else:
        B, H, W, Cin = x.shape
        kind = CONV_IN_NHWC
        if x.dtype != torch.float32:
            raise _lib.WvnError(f"conv2d_bn_act: fp32 activations expected, got {x.dtype}")
        x = x.contiguous()
    Cout = packed.shape[1]
    if packed.shape[0] * Cout != lib().wvn_conv2d_pack_floats(Cout, Cin, ksize) or scale.numel() != Cout or shift.numel() != Cout:
        raise _lib.WvnError(f"conv2d_bn_act: packed {tuple(packed.shape)} / scale / shift do not fit Cin={Cin}, ksize={ksize}")
    if H + 2 * pad < ksize or W + 2 * pad < ksize or stride < 1:
        raise _lib.WvnError(f"conv2d_bn_act: ksize={ksize} does not fit {H} x {W} with pad={pad}")
    OH, OW = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    out = torch.empty(B, OH, OW, Cout, dtype=torch.float32, device=x.device)
    if residual is not None:
        require_cuda(residual, "residual")
        if tuple(residual.shape) != tuple(out.shape) or residual.dtype != torch.float32:
            raise _lib.WvnError(f"conv2d_bn_act: residual must be fp32 {tuple(out.shape)}, not {residual.dtype} {tuple(residual.shape)}")
        residual = residual.contiguous()
    check(lib().wvn_conv2d_bn_act(ptr(x), kind, ptr(packed.contiguous()), ptr(scale.contiguous().float()), ptr(shift.contiguous().float()),
                                  ptr(residual), int(bool(relu)), ptr(out), B, H, W, Cin, Cout, ksize, stride, pad, stream()),
          "wvn_conv2d_bn_act")
    return out


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    """F.max_pool2d(kernel 3, stride 2, padding 1) on an NHWC fp32 activation [B,H,W,C] (the padding is -inf)."""
    require_cuda(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise _lib.WvnError(f"maxpool3x3s2: fp32 [B,H,W,C] expected, got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    B, H, W, Cc = x.shape
    out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, dtype=torch.float32, device=x.device)
    check(lib().wvn_maxpool3x3s2(ptr(x), ptr(out), B, H, W, Cc, stream()), "wvn_maxpool3x3s2")
    return out


def resnet18_pack(weights, scales, shifts) -> torch.Tensor:
    """The packed image of ResNet-18 for ``resnet18_forward``: three lists of RESNET18_NCONV GPU tensors in the order of
    include/wvn_hip.h (weights [Cout,Cin,k,k], folded BatchNorm scale / shift [Cout])."""
    if not (len(weights) == len(scales) == len(shifts) == RESNET18_NCONV):
        raise _lib.WvnError(f"resnet18_pack: {RESNET18_NCONV} convolutions expected")
    keep = []
    arrays = []
    for ts in (weights, scales, shifts):
        arr = (C.c_void_p * RESNET18_NCONV)()
        for i, t in enumerate(ts):
            require_cuda(t, "resnet18 parameter")
            t = t.contiguous().float()
            keep.append(t)
            arr[i] = t.data_ptr()
        arrays.append(arr)
    nbytes = lib().wvn_resnet18_pack_bytes()
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=weights[0].device)
    check(lib().wvn_resnet18_pack(arrays[0], arrays[1], arrays[2], ptr(packed), nbytes, stream()), "wvn_resnet18_pack")
    torch.cuda.current_stream().synchronize()   # `keep` may be released after the copies have run
    return packed


def resnet18_workspace(B: int, H: int, W: int, device) -> torch.Tensor:
    nbytes = lib().wvn_resnet18_workspace_bytes(B, H, W)
    if nbytes == 0:
        raise _lib.WvnError(f"resnet18: frames [B={B},3,{H},{W}] are not supported (H and W must be multiples of 32)")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def resnet18_levels(workspace: torch.Tensor, B: int, H: int, W: int):
    """The four NHWC level maps [B,H/s,W/s,C] (s = 4, 8, 16, 32) as views of a ``resnet18_forward`` workspace."""
    out = []
    for l, Cc in enumerate(PYRAMID_CHANNELS, start=1):
        s = 2 << l
        off = lib().wvn_resnet18_level_offset(B, H, W, l) // 4
        out.append(workspace[off: off + B * (H // s) * (W // s) * Cc].view(B, H // s, W // s, Cc))
    return out


def resnet18_forward(packed: torch.Tensor, img: torch.Tensor, workspace: Optional[torch.Tensor] = None):
    """ResNet-18 (eval mode) on frames [B,3,H,W] (fp32 in [0,1] or uint8; H, W multiples of 32) -> (the four NHWC level maps as views of
    the workspace, the workspace).  A given workspace must be ``resnet18_workspace(B, H, W, device)`` or larger."""
    require_cuda(img, "img")
    require_cuda(packed, "packed")
    if img.dim() != 4 or img.shape[1] != 3:
        raise _lib.WvnError(f"resnet18_forward: img must be [B,3,H,W], not {tuple(img.shape)}")
    img = img.contiguous() if img.dtype == torch.uint8 else img.contiguous().float()
    B, _, H, W = img.shape
    if workspace is None:
        workspace = resnet18_workspace(B, H, W, img.device)
    check(lib().wvn_resnet18_forward(ptr(packed), ptr(img), int(img.dtype == torch.uint8), B, H, W, ptr(workspace),
                                     workspace.numel() * workspace.element_size(), stream()), "wvn_resnet18_forward")
    return resnet18_levels(workspace, B, H, W), workspace


def segpool_pyramid(levels, seg: torch.Tensor, n_seg: int) -> torch.Tensor:
    """The multi-scale segment pooling (feature_extractor.py:314-366 of the reference): levels = four NHWC maps [B,H/s,W/s,C] with
    C = 64, 128, 256, 512 at s = 4, 8, 16, 32, seg [B,H,W] int -> feat [B,n_seg,960].  Per level the mean over the cells of seg[::s, ::s]
    that carry the id; where none does, the cell holding the segment's centroid; NaN rows for ids without a pixel (include/wvn_hip.h)."""
    require_cuda(seg, "seg")
    if seg.dim() != 3:
        raise _lib.WvnError(f"segpool_pyramid: seg must be [B,H,W], not {tuple(seg.shape)}")
    B, H, W = seg.shape
    if len(levels) != 4 or H % 32 or W % 32:
        raise _lib.WvnError(f"segpool_pyramid: four level maps and H, W multiples of 32 expected (H={H}, W={W})")
    maps = []
    for l, (m, Cc) in enumerate(zip(levels, PYRAMID_CHANNELS)):
        s = 4 << l
        require_cuda(m, "level map")
        if tuple(m.shape) != (B, H // s, W // s, Cc) or m.dtype != torch.float32:
            raise _lib.WvnError(f"segpool_pyramid: level {l + 1} must be fp32 NHWC {(B, H // s, W // s, Cc)}, not {m.dtype} {tuple(m.shape)}")
        maps.append(m.contiguous())
    if n_seg < 1:
        raise _lib.WvnError(f"segpool_pyramid: n_seg={n_seg} must be >= 1")
    seg = _i32(seg).contiguous()
    nbytes = lib().wvn_segpool_pyramid_scratch_bytes(B, int(n_seg))
    if nbytes == 0:
        raise _lib.WvnError(f"segpool_pyramid: B={B}, n_seg={n_seg} not supported")
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=seg.device)
    feat = torch.empty(B, n_seg, PYRAMID_DIM, dtype=torch.float32, device=seg.device)
    check(lib().wvn_segpool_pyramid(ptr(maps[0]), ptr(maps[1]), ptr(maps[2]), ptr(maps[3]), ptr(seg), ptr(feat), ptr(scratch), nbytes, B, H,
                                    W, int(n_seg), stream()), "wvn_segpool_pyramid")
    return feat


def upsample_nearest_labels(labels: torch.Tensor, out_size: int) -> torch.Tensor:
    """labels [B,G,G] int32 -> [B,H,H] int32 (stego_interface.py:108-109)."""
    require_cuda(labels, "labels")
    labels = _i32(labels).contiguous()
    B, G, _ = labels.shape
    out = torch.empty(B, out_size, out_size, dtype=torch.int32, device=labels.device)
    check(lib().wvn_upsample_nearest_i32(ptr(labels), ptr(out), B, G, out_size, stream()), "wvn_upsample_nearest_i32")
    return out


def segpool_bilinear_mean(seg: torch.Tensor, tokens: torch.Tensor, grid: int, n_seg: int,
                          return_counts: bool = False):
    """Fused up-sample + per-segment mean (feature_extractor.py:390-396 on dino_interface.py:87-90).
    seg [B,H,H] int (-1 ignored), tokens [B,G*G,D] fp32 -> feat [B,S,D] fp32 (NaN row for an empty id).
    Square frames only: both axes are resampled with the reference's (G-1)/(H-1) tap scale."""
    require_cuda(tokens, "tokens")
    seg = _i32(seg).contiguous()
    B, H, W = seg.shape
    if H != W:
        raise _lib.WvnError(f"segpool_bilinear_mean: square frames only (seg is [B,H,H]); got H={H}, W={W}")
    tokens = tokens.contiguous()
    D = tokens.shape[-1]
    dev = tokens.device
    feat = torch.empty(B, n_seg, D, dtype=torch.float32, device=dev)
    wbuf = torch.empty(B * n_seg * grid * grid, dtype=torch.int64, device=dev)  # 2^-40 fixed-point tap weights
    cnt = torch.empty(B * n_seg, dtype=torch.int32, device=dev)
    check(lib().wvn_segpool_bilinear_mean(ptr(seg), ptr(tokens), D, ptr(feat), ptr(wbuf), ptr(cnt), B, H, W, grid,
                                          n_seg, D, stream()), "wvn_segpool_bilinear_mean")
    return (feat, cnt.reshape(B, n_seg)) if return_counts else feat


_STENCILS = {}


def patch_stencil_tables(grid: int, out_size: int, device):
    """[G][3] stencil weights (offsets -1, 0, +1) of the block-averaged align_corners=True bilinear
    up-sampling grid -> out_size for patch size P = out_size // grid; None when the geometry is not
    patch-aligned (out_size != grid * P) or a tap falls outside the 3-wide stencil."""
    key = (grid, out_size, str(device))
    if key not in _STENCILS:
        import numpy as np

        P = out_size // grid
        tab = None
        if P * grid == out_size and P >= 1:
            scale = np.float32(grid - 1) / np.float32(out_size - 1) if out_size > 1 else np.float32(0)
            tab = np.zeros((grid, 3), dtype=np.float32)
            for y in range(out_size):
                g = y // P
                src = np.float32(scale * np.float32(y))
                y0 = int(src)
                y1 = y0 + (1 if y0 < grid - 1 else 0)
                w1 = np.float32(src - np.float32(y0))
                for yy, ww in ((y0, np.float32(1) - w1), (y1, w1)):
                    if not -1 <= yy - g <= 1:
                        tab = None
                        break
                    tab[g, yy - g + 1] += ww
                if tab is None:
                    break
            if tab is not None:
                tab = torch.from_numpy(tab / np.float32(P)).to(device)
        _STENCILS[key] = tab
    return _STENCILS[key]


def segpool_patch_labels(labels: torch.Tensor, tokens: torch.Tensor, grid: int, out_size: int, n_seg: int):
    """Patch-aligned fast path of segpool_bilinear_mean: labels [B,G,G] (or [B,G*G]) int32 at patch
    resolution, tokens [B,G*G,D] -> feat [B,S,D].  Returns None if the geometry is not patch-aligned."""
    require_cuda(tokens, "tokens")
    tab = patch_stencil_tables(grid, out_size, tokens.device)
    if tab is None or n_seg * 65 * 4 > 60 * 1024:
        return None
    tokens = tokens.contiguous()
    B, P, D = tokens.shape
    labels = _i32(labels).reshape(B, P).contiguous()
    feat = torch.empty(B, n_seg, D, dtype=torch.float32, device=tokens.device)
    check(lib().wvn_segpool_patch_labels(ptr(labels), ptr(tokens), D, ptr(tab), ptr(tab), ptr(feat), B, grid, n_seg, D,
                                         stream()), "wvn_segpool_patch_labels")
    return feat


def segmean_tokens(seg: torch.Tensor, tokens: torch.Tensor, n_seg: int) -> torch.Tensor:
    """Plain per-segment mean of a pixel-resolution map: seg [B,H,W] / [B,P], tokens [B,P,D] -> [B,S,D]."""
    require_cuda(tokens, "tokens")
    tokens = tokens.contiguous().float()
    B, P, D = tokens.shape
    seg = _i32(seg).reshape(B, P).contiguous()
    out = torch.empty(B, n_seg, D, dtype=torch.float32, device=tokens.device)
    cnt = torch.empty(B * n_seg, dtype=torch.int32, device=tokens.device)
    scratch = torch.empty(lib().wvn_segmean_scratch_bytes(B, P, n_seg, D), dtype=torch.uint8, device=tokens.device)
    check(lib().wvn_segmean_tokens(ptr(seg), ptr(tokens), ptr(out), ptr(cnt), ptr(scratch), scratch.numel(), B, P, n_seg, D,
                                   stream()), "wvn_segmean_tokens")
    return out


def label_pool(mask: torch.Tensor, seg: torch.Tensor, n_seg: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """MissionNode.update_supervision_signal (nodes.py:400-440). mask [C,H,W] fp32 w/ NaN, seg [H,W]."""
    require_cuda(mask, "mask")
    mask = mask.contiguous().float()
    if mask.dim() == 2:
        mask = mask[None]
    seg = _i32(seg).contiguous()
    Cc, H, W = mask.shape
    dev = mask.device
    signal = torch.empty(n_seg, dtype=torch.float32, device=dev)
    valid = torch.empty(n_seg, dtype=torch.uint8, device=dev)
    ssum = torch.empty(n_seg, dtype=torch.int64, device=dev)   # 2^-32 fixed-point sums (deterministic integer atomics)
    scnt = torch.empty(n_seg, dtype=torch.int32, device=dev)
    check(lib().wvn_label_pool(ptr(mask), Cc, ptr(seg), ptr(signal), ptr(valid), ptr(ssum), ptr(scnt), H, W, n_seg,
                               stream()), "wvn_label_pool")
    return signal, valid.bool()


def _record_table(rows, dev) -> torch.Tensor:
    """Device array of C records whose fields are 8-byte words (pointers / int pairs), built from Python ints."""
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def label_pool_batched(masks, segs, n_segs):
    """``label_pool`` for a list of nodes in ONE launch pair.  masks: list of [C,H,W] fp32 CUDA tensors (same shape), segs:
    list of [H,W] int32 CUDA tensors, n_segs: list of ints -> list of (signal [S_i] fp32, valid [S_i] bool)."""
    n = len(masks)
    dev = masks[0].device
    Cc, H, W = masks[0].shape
    smax = max(n_segs)
    sig = [torch.empty(s, dtype=torch.float32, device=dev) for s in n_segs]
    val = [torch.empty(s, dtype=torch.uint8, device=dev) for s in n_segs]
    for m, sg in zip(masks, segs):
        require_cuda(m, "mask")
        if m.dtype != torch.float32 or not m.is_contiguous() or sg.dtype != torch.int32 or not sg.is_contiguous():
            raise _lib.WvnError("label_pool_batched: masks must be contiguous fp32 [C,H,W], segment maps contiguous int32 [H,W]")
    table = _record_table([[ptr(m), ptr(sg), ptr(a), ptr(b), s] for m, sg, a, b, s in zip(masks, segs, sig, val, n_segs)], dev)
    ssum = torch.empty(n * smax, dtype=torch.int64, device=dev)
    scnt = torch.empty(n * smax, dtype=torch.int32, device=dev)
    check(lib().wvn_label_pool_batched(ptr(table), n, Cc, H, W, smax, ptr(ssum), ptr(scnt), stream()), "wvn_label_pool_batched")
    return [(a, b.bool()) for a, b in zip(sig, val)]


def project_render_fmin(Ks, poses, masks, points: torch.Tensor, value, want_projected: bool = False):
    """ImageProjector.project_and_render + torch.fmin merge for n nodes in one launch (csrc/supervision.hip).
    Ks / poses: lists of [4,4] fp32 CUDA tensors (scaled camera matrix, pose_cam_in_world); masks: list of contiguous
    [C,H,W] fp32 CUDA tensors, UPDATED IN PLACE; points [N,3] (shared) or [n,N,3]; value: float or 1-element CUDA tensor
    (colour * traversability).  ``want_projected``: returns (projected [n,N,2] raw pinhole coordinates, depth [n,N] camera-frame z).
    Refused before anything is launched: no mask, a mask that is not [C,H,W] or lives on the CPU, len(Ks) or len(poses) != n, a K or
    pose that is not [4,4], points that are not [N,3] or [n,N,3] with N >= 2, a value tensor with more than one element."""
    who = "project_render_fmin"
    n = len(masks)
    if n < 1 or any(not isinstance(m, torch.Tensor) or m.dim() != 3 for m in masks):
        raise _lib.WvnError(f"{who}: masks must be a non-empty list of [C,H,W] tensors")
    if len(Ks) != n or len(poses) != n:
        raise _lib.WvnError(f"{who}: {len(Ks)} camera matrices and {len(poses)} poses for {n} masks")
    for name, ts in (("K", Ks), ("pose", poses)):
        for t in ts:
            if tuple(t.shape) != (4, 4):
                raise _lib.WvnError(f"{who}: every {name} must be [4,4], not {tuple(t.shape)}")
    if points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise _lib.WvnError(f"{who}: points must be [N,3] or [n,N,3], not {tuple(points.shape)}")
    if points.dim() == 3 and points.shape[0] != n:
        raise _lib.WvnError(f"{who}: batched points {tuple(points.shape)} for {n} masks: the leading dimension must be {n}")
    if points.shape[-2] < 2:
        raise _lib.WvnError(f"{who}: a polygon needs at least 2 points, not {points.shape[-2]}")
    if isinstance(value, torch.Tensor) and value.numel() != 1:
        raise _lib.WvnError(f"{who}: value must be a float or a 1-element tensor, not {tuple(value.shape)}")
    for m in masks:
        require_cuda(m, "mask")
    dev = masks[0].device
    Cc, H, W = masks[0].shape
    points = points.to(dev, torch.float32).contiguous()
    batched = points.dim() == 3
    N = points.shape[-2]
    proj = torch.empty(n, N, 2, dtype=torch.float32, device=dev) if want_projected else None
    depth = torch.empty(n, N, dtype=torch.float32, device=dev) if want_projected else None
    keep = []
    rows = []
    for i in range(n):
        K = Ks[i].to(dev, torch.float32).contiguous()
        T = poses[i].to(dev, torch.float32).contiguous()
        keep += [K, T]
        m = masks[i]
        if m.dtype != torch.float32 or not m.is_contiguous() or tuple(m.shape) != (Cc, H, W):
            raise _lib.WvnError("project_render_fmin: masks must be contiguous fp32 [C,H,W] of one shape")
        rows.append([ptr(K), ptr(T), ptr(m), ptr(proj[i]) if proj is not None else 0, ptr(depth[i]) if depth is not None else 0])
    table = _record_table(rows, dev)
    vdev = value if isinstance(value, torch.Tensor) else None
    if vdev is not None:
        vdev = vdev.to(dev, torch.float32).reshape(-1).contiguous()
    check(lib().wvn_project_render_fmin(ptr(table), n, ptr(points), int(batched), N, Cc, H, W, ptr(vdev),
                                        0.0 if vdev is not None else float(value), stream()), "wvn_project_render_fmin")
    return (proj, depth) if want_projected else None


_SLIC_TABLES = {}


def slic_tables(device):
    """sRGB -> linear (x 4095) and CIELAB f(t) (x 4096) lookup tables of the integer SLIC (csrc/slic.hip), built in double
    precision on the host."""
    key = str(device)
    if key not in _SLIC_TABLES:
        import numpy as np

        c = np.arange(256, dtype=np.float64) / 255.0
        lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
        t = np.arange(4096, dtype=np.float64) / 4095.0
        f = np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)
        _SLIC_TABLES[key] = (torch.from_numpy(np.rint(lin * 4095.0).astype(np.int32)).to(device),
                             torch.from_numpy(np.rint(f * 4096.0).astype(np.int32)).to(device))
    return _SLIC_TABLES[key]


def slic(img: torch.Tensor, num_components: int = 100, compactness: float = 10.0, iters: int = 10,
         enforce_connectivity: bool = False, min_size_factor: float = 0.25) -> torch.Tensor:
    """img [3,H,W] uint8 or float in [0,1] (CUDA) -> SLIC label map [H,W] int32 in [0, slic_num_clusters); [B,3,H,W] -> [B,H,W].
    ``enforce_connectivity``: the post-processing step of SLIC (fast_slic's default) as ONE batched pass over the B maps
    (``slic_enforce_connectivity`` with min_size = max(1, int(min_size_factor * H * W / slic_num_clusters))); off by default, and
    then the labels are the k-means result exactly as before."""
    require_cuda(img, "img")
    if img.dim() not in (3, 4) or img.shape[-3] != 3:
        raise _lib.WvnError(f"slic: img must be [3,H,W] or [B,3,H,W], not {tuple(img.shape)}")
    u8 = img.dtype == torch.uint8
    img = img.contiguous() if u8 else img.contiguous().float()
    single = img.dim() == 3
    frames = img[None] if single else img
    B, _, H, W = frames.shape
    lin, f = slic_tables(img.device)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=img.device)
    scratch = torch.empty(lib().wvn_slic_scratch_bytes(H, W, num_components), dtype=torch.uint8, device=img.device)
    for b in range(B):   # (launches only: the frames share the scratch buffer in stream order)
        check(lib().wvn_slic(ptr(frames[b]), int(u8), H, W, num_components, float(compactness), iters, ptr(lin), ptr(f), ptr(labels[b]),
                             ptr(scratch), scratch.numel(), stream()), "wvn_slic")
    if enforce_connectivity:
        K = slic_num_clusters(H, W, num_components)
        slic_enforce_connectivity(labels, K, slic_min_size(H, W, K, min_size_factor), out=labels)
    return labels[0] if single else labels


def slic_min_size(H: int, W: int, n_clusters: int, min_size_factor: float = 0.25) -> int:
    """Smallest fragment that connectivity enforcement leaves alone: a fraction (fast_slic's default: a quarter) of the mean superpixel."""
    return max(1, int(min_size_factor * H * W / n_clusters))


# tile of the component-labelling kernel (rows, columns): WVN_SLIC_CC_TILE_H / _W of include/wvn_hip.h (the tests pick sizes around it)
SLIC_CC_TILE = (8, 32)


def slic_enforce_connectivity(labels: torch.Tensor, n_clusters: int, min_size: int, out: Optional[torch.Tensor] = None,
                              return_waiting: bool = False):
    """Connectivity enforcement of label maps (csrc/slic_connectivity.hip; the definition is in include/wvn_hip.h): labels [H,W] or
    [B,H,W] int32 (CUDA) with ids in [0, n_clusters) -- SLIC's or any other -> the same shape, every 4-connected fragment below
    ``min_size`` pixels handed to the neighbouring label with the longest common border (lowest id on a tie), in rounds, until none is
    left.  One launch sequence for the whole batch and no host synchronisation.  ``out`` may be ``labels`` (in place).
    ``return_waiting``: also returns the kernels' per-image counters of components still waiting at the end, [B] int32 on the device --
    zero by construction (the tests assert it)."""
    require_cuda(labels, "labels")
    if labels.dtype != torch.int32 or labels.dim() not in (2, 3):
        raise _lib.WvnError("slic_enforce_connectivity: labels must be int32 [H,W] or [B,H,W]")
    labels = labels.contiguous()
    H, W = labels.shape[-2:]
    B = 1 if labels.dim() == 2 else labels.shape[0]
    if out is None:
        out = torch.empty_like(labels)
    elif out.dtype != torch.int32 or out.shape != labels.shape or not out.is_contiguous() or out.device != labels.device:
        raise _lib.WvnError("slic_enforce_connectivity: out must be a contiguous int32 tensor of labels' shape on labels' device")
    nbytes = lib().wvn_slic_connectivity_scratch_bytes(B, H, W, int(n_clusters))
    if nbytes == 0:
        raise _lib.WvnError(f"slic_enforce_connectivity: unsupported shape B={B} H={H} W={W} n_clusters={n_clusters}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=labels.device)
    check(lib().wvn_slic_connectivity(ptr(labels), ptr(out), B, H, W, int(n_clusters), int(min_size), ptr(scratch), scratch.numel(),
                                      stream()), "wvn_slic_connectivity")
    if return_waiting:
        return out, scratch[:16 * B].view(torch.int32)[::4].clone()
    return out


def slic_num_clusters(H: int, W: int, num_components: int) -> int:
    return int(lib().wvn_slic_num_clusters(H, W, num_components))


def seg_centers(seg: torch.Tensor, n_seg: int) -> torch.Tensor:
    require_cuda(seg, "seg")
    seg = _i32(seg).contiguous()
    H, W = seg.shape[-2:]
    out = torch.empty(n_seg, 2, dtype=torch.float32, device=seg.device)
    scratch = torch.empty(3 * n_seg, dtype=torch.int64, device=seg.device)
    check(lib().wvn_seg_centers(ptr(seg), ptr(out), ptr(scratch), H, W, n_seg, stream()), "wvn_seg_centers")
    return out


def seg_adjacency(seg: torch.Tensor, n_seg: int) -> torch.Tensor:
    require_cuda(seg, "seg")
    seg = _i32(seg).contiguous()
    H, W = seg.shape[-2:]
    dev = seg.device
    max_edges = n_seg * n_seg
    edges = torch.empty(max_edges, 2, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    bitmap = torch.empty(n_seg * n_seg, dtype=torch.uint8, device=dev)
    check(lib().wvn_seg_adjacency(ptr(seg), ptr(edges), ptr(count), ptr(bitmap), H, W, n_seg, max_edges, stream()),
          "wvn_seg_adjacency")
    return edges[: int(count.item())]  # the edge count fixes the output shape: one host sync, as in the reference


def seg_adjacency_batched(seg: torch.Tensor, n_seg: int) -> torch.Tensor:
    """seg [B,H,W] int32 -> adj [B,S,S] uint8 with adj[b, l, r] = 1 exactly for the (left, right) pairs ``seg_adjacency`` returns
    for frame b: the bitmap that call compacts, for every frame at once, without the edge count and so without a host
    synchronisation.  (The result is a transposed view: memory is target-major, [b][r][l].)"""
    require_cuda(seg, "seg")
    if seg.dim() != 3 or n_seg < 1:
        raise _lib.WvnError(f"seg_adjacency_batched: seg [B,H,W] and n_seg >= 1 expected, got {tuple(seg.shape)} and {n_seg}")
    seg = _i32(seg).contiguous()
    B, H, W = seg.shape
    adj = torch.empty(B, n_seg, n_seg, dtype=torch.uint8, device=seg.device)
    check(lib().wvn_seg_adjacency_batched(ptr(seg), ptr(adj), B, H, W, n_seg, stream()), "wvn_seg_adjacency_batched")
    return adj.transpose(1, 2)


def kmeans_cosine(code: torch.Tensor, K: int, iters: int = 10, relabel: bool = True, return_centroids: bool = False):
    """code [B,P,C] fp32 (any row stride) -> (labels [B,P] int32, n_segments [B] int32[, final centroids [B,K,C]])."""
    require_cuda(code, "code")
    B, P, Cc = code.shape
    if code.stride(2) != 1 or code.stride(0) != P * code.stride(1):
        code = code.contiguous()
    dev = code.device
    xn = torch.empty(B, P, Cc, dtype=torch.float32, device=dev)
    check(lib().wvn_normalize_rows(ptr(code), code.stride(1), ptr(xn), B * P, Cc, stream()), "wvn_normalize_rows")
    labels = torch.empty(B, P, dtype=torch.int32, device=dev)
    nseg = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib().wvn_kmeans_scratch_bytes(B, P, Cc, K), dtype=torch.uint8, device=dev)
    check(lib().wvn_kmeans_cosine(ptr(xn), ptr(labels), ptr(nseg), ptr(scratch), B, P, Cc, K, iters, int(relabel),
                                  stream()), "wvn_kmeans_cosine")
    if return_centroids:   # (the centroids are the first B*K*C floats of the scratch area, include/wvn_hip.h)
        return labels, nseg, scratch.view(torch.float32)[: B * K * Cc].reshape(B, K, Cc).clone()
    return labels, nseg


def kmeans_cosine_pixels_supported(G: int, H: int, C: int, K: int) -> bool:
    """Whether ``wvn_kmeans_cosine_pixels`` has an instantiation for this shape (csrc/stego.hip: code dimension 90 or 16, up to 64
    clusters, the two staged code rows within 96 KB of LDS); callers fall back to the dense rows + ``kmeans_cosine`` otherwise."""
    return C in (90, 16) and 0 < K <= 64 and 2 * G * C * 4 <= 96 * 1024 and G > 0 and H > 0


def kmeans_pixels_linear_supported(G: int, H: int, C: int, K: int) -> bool:
    """Whether the linear form of the pixel k-means (``wvn_kmeans_cosine_pixels_linear``, csrc/stego_linear.hip) has an instantiation
    for this shape (code dimension 90 or 16, up to 32 clusters, its per-band tables within the LDS)."""
    return bool(lib().wvn_kmeans_pixels_linear_supported_shape(G, H, C, K))


def kmeans_cosine_pixels(code: torch.Tensor, G: int, H: int, K: int, iters: int = 10, relabel: bool = True,
                         return_centroids: bool = False, form: str = "linear", align_corners: bool = True):
    """code [B, G*G, C] fp32 patch codes -> (labels [B, H*H] int32, n_segments [B] int32): the k-means of ``kmeans_cosine`` over
    the H x H bilinearly up-sampled, normalised code pixels (the [B, H*H, C] array is never built).
    form="linear" (default, oracle/kmeans_linear.py): assignment from a per-pass similarity table interpolated per pixel, centroid
    sums from summed tap weights times the patch codes -- the same clustering at ~1/20 of the arithmetic; form="direct"
    (oracle/interfaces.py::kmeans_cosine_labels_pixels): every row re-created and multiplied out in every pass.  Both are
    deterministic and bit-exact against their oracle; they differ from each other only where two similarities tie within fp32 rounding.
    align_corners=False (linear form only): the code pixels are the half-pixel (align_corners=False) bilinear interpolation of the patch codes --
    the other reading of the absent STEGO package (include/wvn_hip.h: wvn_kmeans_cosine_pixels_linear_ac)."""
    require_cuda(code, "code")
    if not align_corners and form != "linear":
        raise _lib.WvnError("kmeans_cosine_pixels: align_corners=False exists in the linear form only")
    B, P, Cc = code.shape
    if P != G * G:
        raise _lib.WvnError(f"kmeans_cosine_pixels: {P} code rows for a {G} x {G} grid")
    if form not in ("linear", "direct"):
        raise _lib.WvnError(f"kmeans_cosine_pixels: form must be 'linear' or 'direct', not {form!r}")
    code = code.contiguous()
    dev = code.device
    labels = torch.empty(B, H * H, dtype=torch.int32, device=dev)
    nseg = torch.empty(B, dtype=torch.int32, device=dev)
    if form == "linear":
        if not kmeans_pixels_linear_supported(G, H, Cc, K):
            raise _lib.WvnError(f"kmeans_cosine_pixels(form='linear'): no instantiation for G={G}, H={H}, C={Cc}, K={K} "
                                "(C in {16, 90}, K <= 32); use form='direct'")
        scratch = torch.empty(lib().wvn_kmeans_pixels_linear_scratch_bytes(B, G, H, Cc, K), dtype=torch.uint8, device=dev)
        check(lib().wvn_kmeans_cosine_pixels_linear_ac(ptr(code), ptr(labels), ptr(nseg), ptr(scratch), B, G, H, Cc, K, iters,
                                                       int(relabel), int(bool(align_corners)), stream()), "wvn_kmeans_cosine_pixels_linear_ac")
    else:
        scratch = torch.empty(lib().wvn_kmeans_pixels_scratch_bytes(B, G, H, Cc, K), dtype=torch.uint8, device=dev)
        check(lib().wvn_kmeans_cosine_pixels(ptr(code), ptr(labels), ptr(nseg), ptr(scratch), B, G, H, Cc, K, iters, int(relabel),
                                             stream()), "wvn_kmeans_cosine_pixels")
    if return_centroids:
        return labels, nseg, scratch.view(torch.float32)[: B * K * Cc].reshape(B, K, Cc).clone()
    return labels, nseg


def table_bilerp_argmax(table: torch.Tensor, G: int, H: int, align_corners: bool = True) -> torch.Tensor:
    """table [B, G*G, K] fp32 (K <= 32 scores per patch) -> labels [B, H, H] int32: per pixel the first-maximum argmax of the
    bilinearly interpolated (align_corners as given, fixed operation order) scores -- a linear probe at pixel resolution."""
    require_cuda(table, "table")
    B, P, K = table.shape
    if P != G * G:
        raise _lib.WvnError(f"table_bilerp_argmax: {P} rows for a {G} x {G} grid")
    KP = lib().wvn_table_argmax_slots(K)
    if KP <= 0:
        raise _lib.WvnError(f"table_bilerp_argmax: 1..32 scores per patch are supported, not {K}")
    t = table.float()
    t = torch.nn.functional.pad(t, (0, KP - K)).contiguous() if KP != K else t.contiguous()
    labels = torch.empty(B, H, H, dtype=torch.int32, device=table.device)
    check(lib().wvn_table_bilerp_argmax_ac(ptr(t), ptr(labels), B, G, H, K, int(bool(align_corners)), stream()), "wvn_table_bilerp_argmax_ac")
    return labels


def flip_average(code: torch.Tensor, mirrored: Optional[torch.Tensor], G: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """0.5 * (code + flip_x(mirrored)) on [B, G*G, C] fp32 patch maps (in place on ``code`` unless ``out`` is given).  The inputs may be
    views of rows with a padded stride (``buf[..., :C]`` of the [.., 128] code rows the fused STEGO head writes); ``out`` is then required
    and contiguous.  ``mirrored=None``: ``out = code`` (the padded rows narrowed, no mirror pass)."""
    require_cuda(code, "code")
    B, P, Cc = code.shape
    ld = code.stride(1)

    def rows_ok(t):
        return t.dtype == torch.float32 and t.stride(2) == 1 and t.stride(1) == ld and (t.shape[0] == 1 or t.stride(0) == P * ld)

    if P != G * G or ld < Cc or not rows_ok(code) or (mirrored is not None and (mirrored.shape != code.shape or not rows_ok(mirrored))):
        raise _lib.WvnError("flip_average: [B, G*G, C] fp32 pairs expected, contiguous or with one common padded row stride")
    if out is None and (ld != Cc or mirrored is None):
        raise _lib.WvnError("flip_average: padded rows / the no-mirror form need out=")
    dst = code if out is None else out
    if out is not None and (not out.is_contiguous() or out.shape != code.shape or out.dtype != torch.float32):
        raise _lib.WvnError("flip_average: out must be a contiguous fp32 tensor of the inputs' shape")
    check(lib().wvn_flip_average(ptr(code), ptr(mirrored), ptr(dst), B, G, Cc, ld, stream()), "wvn_flip_average")
    return dst


def cast_rows_bf16(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[r, :cols] = src[r, :] rounded to dst's 16-bit format (bf16 / fp16); fp32 rows with any row stride."""
    require_cuda(src, "src")
    R, Cc = src.shape
    if src.stride(1) != 1 or dst.stride(1) != 1 or dst.shape[0] != R or dst.shape[1] < Cc or dst.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.WvnError("cast_rows_bf16: fp32 [R, C] rows -> 16-bit [R, >= C] rows expected")
    check(lib().wvn_cast_rows(ptr(src), src.stride(0), ptr(dst), dst.stride(0), R, Cc, int(dst.dtype == torch.float16), stream()),
          "wvn_cast_rows")
    return dst


def compact_segment_rows(feat: torch.Tensor, nseg: torch.Tensor, side: Optional[torch.Tensor] = None):
    """feat [B,S,D] fp32 (rows of ids a frame did not produce are NaN), nseg [B] int32 (ids that exist per frame), side
    [B,S,Ds] fp32 (optional per-row data) -> (x [B*S, D], side_out [B*S, Ds] | None, rows_dev int32 [1]): the existing rows
    front to back, zeros behind, the count on the device -- no host synchronisation (``MlpTrainer.train_step(rows_dev=...)``)."""
    require_cuda(feat, "feat")
    B, S, D = feat.shape
    feat = feat.contiguous()
    nseg = nseg.to(torch.int32).contiguous()
    x = torch.empty(B * S, D, dtype=torch.float32, device=feat.device)
    so, Ds = None, 0
    if side is not None:
        side = side.float().contiguous()
        Ds = side.shape[-1]
        so = torch.empty(B * S, Ds, dtype=torch.float32, device=feat.device)
    cnt = torch.empty(1, dtype=torch.int32, device=feat.device)
    check(lib().wvn_compact_segment_rows(ptr(feat), D, ptr(side), Ds, ptr(nseg), B, S, ptr(x), ptr(so), ptr(cnt), stream()),
          "wvn_compact_segment_rows")
    return x, so, cnt


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """x [R, C] fp32 -> int32 [R] index of the row maximum (lowest index wins ties)."""
    require_cuda(x, "x")
    if x.stride(1) != 1:
        x = x.contiguous()
    R, Cc = x.shape
    out = torch.empty(R, dtype=torch.int32, device=x.device)
    check(lib().wvn_argmax_rows(ptr(x), x.stride(0), R, Cc, ptr(out), stream()), "wvn_argmax_rows")
    return out


def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    """x [R, C] fp32 -> x / max(||x||, 1e-12) (sequential fp32, the k-means kernels' normalisation)."""
    require_cuda(x, "x")
    R, Cc = x.shape
    out = torch.empty(R, Cc, dtype=torch.float32, device=x.device)
    check(lib().wvn_normalize_rows(ptr(x), x.stride(0), ptr(out), R, Cc, stream()), "wvn_normalize_rows")
    return out


def gemm_bf16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], epi: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """epilogue(a[M,K] @ w[N,K]^T + bias); a, w bf16 or fp16 (both the same; row strides allowed).  The operand format picks
    the library entry: wvn_gemm_bf16 / wvn_gemm_f16 (the same tile kernel compiled per format, csrc/operand.h)."""
    M, K = a.shape
    N = w.shape[0]
    if a.dtype != w.dtype or a.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.WvnError(f"gemm_bf16: operands must both be bfloat16 or both float16, got {a.dtype} / {w.dtype}")
    if out is None:
        dt = a.dtype if epi in (_lib.EPI_BF16, _lib.EPI_GELU_BF16, _lib.EPI_RELU_BF16) else torch.float32
        out = torch.empty(M, N, dtype=dt, device=a.device)
    fn, name = (lib().wvn_gemm_f16, "wvn_gemm_f16") if a.dtype == torch.float16 else (lib().wvn_gemm_bf16, "wvn_gemm_bf16")
    check(fn(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(out), out.stride(0), M, N, K, epi, stream()), name)
    return out


gemm_lowp = gemm_bf16


def resize_nearest_crop(img: torch.Tensor, tables) -> torch.Tensor:
    """out[..., y, x] = img[..., tables.rows[y], tables.cols[x]] (uint8 / fp32 / int32 images [..., H, W]): T.Resize(NEAREST) +
    T.CenterCrop of ImageProjector.resize_image (image_projector.py:199-200) as one gather (``transforms.ingest_tables``)."""
    require_cuda(img, "img")
    if img.shape[-2] != tables.src_h or img.shape[-1] != tables.src_w or img.element_size() not in (1, 4):
        raise _lib.WvnError(f"resize_nearest_crop: image {tuple(img.shape)} {img.dtype} does not match the tables ({tables.src_h} x {tables.src_w})")
    img = img.contiguous()
    planes = img.numel() // (tables.src_h * tables.src_w)
    out = torch.empty(*img.shape[:-2], tables.out_h, tables.out_w, dtype=img.dtype, device=img.device)
    check(lib().wvn_resize_nearest_crop(ptr(img), ptr(out), planes, tables.src_h, tables.src_w, ptr(tables.rows), ptr(tables.cols),
                                        tables.out_h, tables.out_w, img.element_size(), stream()), "wvn_resize_nearest_crop")
    return out


def crf_image(frame: torch.Tensor, size: Optional[int] = None) -> torch.Tensor:
    """frame [B,3,H,W] (fp32 in [0,1] or raw uint8) -> the u8 image [B, S, S, 3] STEGO's dense_crf rebuilds from the normalised frame:
    u8(trunc(255 * ((((x - mean) / std) * std) + mean))), one fp32 operation at a time, with x the NEAREST-resized, centre-cropped frame
    (the ingest tables of ``transforms.ingest_tables``; ``size`` None keeps the frame's own size)."""
    require_cuda(frame, "frame")
    B, Cc, Hs, Ws = frame.shape
    if Cc != 3:
        raise _lib.WvnError(f"crf_image: expected [B,3,H,W], got {tuple(frame.shape)}")
    u8 = frame.dtype == torch.uint8
    frame = (frame if u8 else frame.float()).contiguous()
    rows = cols = None
    Ho = Wo = size
    if size is None or (Hs, Ws) == (size, size):
        Ho, Wo = Hs, Ws
    else:
        from .feature_extractor.transforms import ingest_tables
        tab = ingest_tables(Hs, Ws, size, frame.device)
        rows, cols = tab.rows, tab.cols
    out = torch.empty(B, Ho, Wo, 3, dtype=torch.uint8, device=frame.device)
    check(lib().wvn_crf_image(ptr(frame), int(u8), B, Hs, Ws, ptr(rows), ptr(cols), Ho, Wo, ptr(out), stream()), "wvn_crf_image")
    return out


def dense_crf(logits, image_u8: torch.Tensor, iterations: int = 10, pos_w: float = 3.0, pos_xy_std: float = 1.0, bi_w: float = 4.0,
              bi_xy_std: float = 67.0, bi_rgb_std: float = 3.0, return_probs: bool = False, relabel_last: bool = False,
              _debug: bool = False, method: str = "exact"):
    """Mean-field dense CRF.  ``method="exact"`` (default): every pixel pair (csrc/dense_crf.hip; DESIGN.md "Dense CRF");
    ``"permutohedral"``: both kernel sums by the permutohedral-lattice filter pydensecrf runs (csrc/dense_crf_permutohedral.hip;
    DESIGN.md "Permutohedral dense CRF"), same arguments and returns.  logits [B,K,H,W] fp32 (K <= 64; any strides with the
    pixel dimensions dense, e.g. a permuted [B,H,W,K] view), image_u8 [B,H,W,3] -> labels int32 [B,H,W] (first maximum of Q^T), plus
    Q fp32 [B,K,H,W] when ``return_probs``.  ``logits`` may also be a tuple of two such tensors (K1 + K2 <= 64): two CRFs on the same
    image in one pass (shared exponentials), labels [B,2,H,W] and Q [B,K1+K2,H,W].  ``relabel_last``: the last group's labels are
    compacted to ascending contiguous ids (the k-means relabel rule) and their count per frame int32 [B] is returned after the labels.  ``_debug`` (tests): also returns the last
    iteration's messages and normalisers [B, 2 KP + 2, H, W] (include/wvn_hip.h)."""
    if method not in ("exact", "permutohedral"):
        raise _lib.WvnError(f"dense_crf: method must be 'exact' or 'permutohedral', not {method!r}")
    perm = method == "permutohedral"
    pair = isinstance(logits, (tuple, list))
    ls = list(logits) if pair else [logits]
    if len(ls) not in (1, 2):
        raise _lib.WvnError("dense_crf: one logits tensor or a pair")
    require_cuda(image_u8, "image_u8")
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 4 or image_u8.shape[-1] != 3:
        raise _lib.WvnError(f"dense_crf: image must be uint8 [B,H,W,3], got {tuple(image_u8.shape)} {image_u8.dtype}")
    B, H, W, _ = image_u8.shape
    desc = []
    for t in ls:
        require_cuda(t, "logits")
        if t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (H, W):
            raise _lib.WvnError(f"dense_crf: logits must be fp32 [B,K,{H},{W}] matching the image, got {tuple(t.shape)} {t.dtype}")
        if t.stride(2) != W * t.stride(3):
            t = t.contiguous()
        desc.append((t, t.shape[1], t.stride(0), t.stride(1), t.stride(3)))
    K1 = desc[0][1]
    K2 = desc[1][1] if pair else 0
    KT = K1 + K2
    if K1 < 1 or K2 < 0 or KT > 64 or (pair and K2 < 1):
        raise _lib.WvnError(f"dense_crf: 1..64 label columns in all (got {K1} + {K2})")
    image_u8 = image_u8.contiguous()
    dev = image_u8.device
    ng = 2 if pair else 1
    labels = torch.empty(B, ng, H, W, dtype=torch.int32, device=dev)
    probs = torch.empty(B, KT, H, W, dtype=torch.float32, device=dev) if return_probs else None
    KP = 32 if KT <= 32 else 64
    dbg = torch.zeros(B, 2 * KP + 2, H, W, dtype=torch.float32, device=dev) if _debug else None
    nseg = torch.empty(B, dtype=torch.int32, device=dev) if relabel_last else None
    name = "wvn_dense_crf_permutohedral" if perm else "wvn_dense_crf"
    nbytes = getattr(lib(), name + "_workspace_bytes")(B, H, W, KT)
    if nbytes == 0:
        raise _lib.WvnError(f"dense_crf: unsupported shape B={B}, H={H}, W={W}, K={KT}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    t1, _, b1, c1, p1 = desc[0]
    t2, _, b2, c2, p2 = desc[1] if pair else (None, 0, 0, 0, 0)
    check(getattr(lib(), name)(ptr(t1), K1, b1, c1, p1, ptr(t2), K2, b2, c2, p2, ptr(image_u8), B, H, W, int(iterations), float(pos_w),
                               float(pos_xy_std), float(bi_w), float(bi_xy_std), float(bi_rgb_std), ptr(labels), ptr(nseg), ptr(probs),
                               ptr(dbg), ptr(ws), nbytes, stream()), name)
    out = (labels if pair else labels[:, 0],)
    if relabel_last:
        out += (nseg,)
    if return_probs:
        out += (probs,)
    if _debug:
        out += (dbg,)
    return out[0] if len(out) == 1 else out


def _permutohedral_lattice(image_u8: torch.Tensor, bilateral: bool, xy_std: float, rgb_std: float = 1.0) -> list:
    """Tests: the lattice ``dense_crf(method="permutohedral")`` builds for one kernel of every frame of image_u8 [B,H,W,3]
    (include/wvn_hip.h wvn_debug_permutohedral_lattice).  Per frame a dict of CPU tensors: M, keys int32 [M, d] (ascending),
    bary fp32 [H W, d + 1], vert int32 [H W, d + 1] (table rows 1..M), nbr int32 [d + 1, M, 2] (rows, 0 = absent)."""
    require_cuda(image_u8, "image_u8")
    image_u8 = image_u8.contiguous()
    B, H, W, _ = image_u8.shape
    d = 5 if bilateral else 2
    E, dev = H * W * (d + 1), image_u8.device
    M = torch.empty(B, dtype=torch.int32, device=dev)
    keys = torch.empty(B, E, d, dtype=torch.int32, device=dev)
    bary = torch.empty(B, E, dtype=torch.float32, device=dev)
    vert = torch.empty(B, E, dtype=torch.int32, device=dev)
    nbr = torch.empty(B, d + 1, E, 2, dtype=torch.int32, device=dev)
    nbytes = lib().wvn_dense_crf_permutohedral_workspace_bytes(B, H, W, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().wvn_debug_permutohedral_lattice(ptr(image_u8), B, H, W, int(bilateral), float(xy_std), float(rgb_std), ptr(M), ptr(keys),
                                                ptr(bary), ptr(vert), ptr(nbr), ptr(ws), nbytes, stream()), "wvn_debug_permutohedral_lattice")
    out = []
    for b in range(B):
        m = int(M[b])
        out.append(dict(M=m, keys=keys[b, :m].cpu(), bary=bary[b].reshape(H * W, d + 1).cpu(), vert=vert[b].reshape(H * W, d + 1).cpu(),
                        nbr=nbr[b, :, :m].cpu()))
    return out


def gemm_f32(a, b, bias=None, epi=_lib.F32_NONE, trans_a=False, trans_b=True, out=None, mask=None):
    """fp32 GEMM; trans_b=True means b is stored [N,K] (Linear layout)."""
    M = a.shape[1] if trans_a else a.shape[0]
    K = a.shape[0] if trans_a else a.shape[1]
    N = b.shape[0] if trans_b else b.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    check(lib().wvn_gemm_f32(ptr(a), a.stride(0), int(trans_a), ptr(b), b.stride(0), int(trans_b), ptr(bias), ptr(out),
                             out.stride(0), M, N, K, epi, ptr(mask), 0 if mask is None else mask.stride(0), stream()),
          "wvn_gemm_f32")
    return out


def quantize_rows_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [R, C] fp32 or bf16 (row stride allowed) -> (q [R, C] float8_e4m3fn, scale [R] fp32): x ~ q * scale, scale = amax / 448."""
    require_cuda(x, "x")
    R, Cc = x.shape
    q = torch.empty(R, Cc, dtype=torch.float8_e4m3fn, device=x.device)
    sc = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib().wvn_quantize_rows_fp8(ptr(x), int(x.dtype == torch.bfloat16), x.stride(0), ptr(q), Cc, ptr(sc), R, Cc, stream()),
          "wvn_quantize_rows_fp8")
    return q, sc


def layernorm_fp8(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """LayerNorm(x [R, D] fp32 contiguous) quantised per row -> (q [R, D] float8_e4m3fn, scale [R]): LN(x) ~ q * scale."""
    require_cuda(x, "x")
    R, D = x.shape
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise _lib.WvnError("layernorm_fp8: contiguous fp32 rows expected")
    q = torch.empty(R, D, dtype=torch.float8_e4m3fn, device=x.device)
    sc = torch.empty(R, dtype=torch.float32, device=x.device)
    check(lib().wvn_layernorm_fp8(ptr(x), ptr(gamma), ptr(beta), ptr(q), D, ptr(sc), R, D, eps, stream()), "wvn_layernorm_fp8")
    return q, sc


def gemm_fp8(a_q: torch.Tensor, sa: torch.Tensor, w_q: torch.Tensor, sw: torch.Tensor, bias: Optional[torch.Tensor], epi: int,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """epilogue((a_q @ w_q^T) * sa[:, None] * sw[None, :] + bias); a_q [M,K], w_q [N,K] float8_e4m3fn, K % 128 == 0."""
    M, K = a_q.shape
    N = w_q.shape[0]
    if out is None:
        dt = torch.bfloat16 if epi in (_lib.EPI_BF16, _lib.EPI_GELU_BF16) else torch.float32
        out = torch.empty(M, N, dtype=dt, device=a_q.device)
    check(lib().wvn_gemm_fp8(ptr(a_q), a_q.stride(0), ptr(w_q), w_q.stride(0), ptr(sa), ptr(sw), ptr(bias), ptr(out), out.stride(0),
                             M, N, K, epi, stream()), "wvn_gemm_fp8")
    return out


def split_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 [R, C] (row stride allowed) -> bf16 [2, R, C]: hi = bf16(x), lo = bf16(x - hi) -- the operand representation of
    the exact-mode MFMA kernels (gemm_x3 / attention_x3)."""
    require_cuda(x, "x")
    R, Cc = x.shape
    out = torch.empty(2, R, Cc, dtype=torch.bfloat16, device=x.device)
    check(lib().wvn_split_planes(ptr(x), x.stride(0), ptr(out[0]), ptr(out[1]), Cc, R, Cc, stream()), "wvn_split_planes")
    return out


def gemm_x3(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], epi: int,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact-mode GEMM: a [2, M, K] and w [2, N, K] are hi / lo bf16 planes (ops.split_planes / backbone.split_planes);
    returns bf16 planes [2, M, N] for epi in {EPI_BF16, EPI_GELU_BF16, EPI_RELU_BF16}, fp32 [M, N] otherwise."""
    _, M, K = a.shape
    N = w.shape[1]
    planes = epi in (_lib.EPI_BF16, _lib.EPI_GELU_BF16, _lib.EPI_RELU_BF16)
    if out is None:
        out = torch.empty((2, M, N) if planes else (M, N), dtype=torch.bfloat16 if planes else torch.float32, device=a.device)
    c, c_lo, ldc = (out[0], out[1], out.stride(1)) if planes else (out, None, out.stride(0))
    check(lib().wvn_gemm_x3(ptr(a[0]), ptr(a[1]), a.stride(1), ptr(w[0]), ptr(w[1]), w.stride(1), ptr(bias), ptr(c), ptr(c_lo),
                            ldc, M, N, K, epi, stream()), "wvn_gemm_x3")
    return out


STEGO_HEAD_LD = 128   # row stride (floats) of the code rows the fused STEGO head writes: 16-byte aligned rows for any code dimension <= 128


def pack_stego_head(w_hid: torch.Tensor, b_hid: torch.Tensor, w_lin: torch.Tensor, b_lin: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The weight of the fused STEGO-head launch (include/wvn_hip.h: wvn_stego_head.w_cat / b_cat): hi / lo bf16 planes [2, 512, 384] of
    [W_hid (384 rows); W_lin (C <= 128 rows); zeros] and the fp32 bias [512] = [b_hid; b_lin; zeros].  fp32 device tensors in."""
    from .backbone import split_planes as _split

    D, Cc = w_hid.shape[1], w_lin.shape[0]
    if w_hid.shape != (384, 384) or w_lin.shape[1] != 384 or Cc > 128:
        raise _lib.WvnError(f"pack_stego_head: D = 384 and a code dimension <= 128 expected, got {tuple(w_hid.shape)} / {tuple(w_lin.shape)}")
    w = torch.zeros(512, D, dtype=torch.float32, device=w_hid.device)
    w[:384], w[384:384 + Cc] = w_hid.float(), w_lin.float()
    b = torch.zeros(512, dtype=torch.float32, device=w_hid.device)
    b[:384], b[384:384 + Cc] = b_hid.float(), b_lin.float()
    return _split(w), b.contiguous()


def stego_head_fused(x: torch.Tensor, stats: torch.Tensor, ln_g: torch.Tensor, ln_b: torch.Tensor, w_cat: torch.Tensor, b_cat: torch.Tensor,
                     frames: int, npatch: int, ntok_s: int, hid: Optional[torch.Tensor] = None,
                     code: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first launch of the fused STEGO head alone (csrc/gemm_a384_x3.hip, X_HEAD): x [frames * ntok_s, 384] fp32 residual rows, stats
    [frames * ntok_s, 2] = {mean, rstd} -> (hid bf16 planes [2, M, 384] = ReLU(LN(x) W_hid^T + b_hid), code fp32 [M, 128] whose columns
    hold LN(x) W_lin^T + b_lin), M = frames * npatch patch rows; patch p of frame f is read at row f * ntok_s + 1 + p.  ``hid`` /
    ``code`` may be given with MORE rows than M: the rows past M are not written."""
    require_cuda(x, "x")
    M = frames * npatch
    if hid is None:
        hid = torch.empty(2, M, 384, dtype=torch.bfloat16, device=x.device)
    if code is None:
        code = torch.empty(M, STEGO_HEAD_LD, dtype=torch.float32, device=x.device)
    if x.shape != (frames * ntok_s, 384) or not x.is_contiguous() or stats.shape != (frames * ntok_s, 2) or not stats.is_contiguous():
        raise _lib.WvnError("stego_head_fused: x [frames * ntok_s, 384] and stats [frames * ntok_s, 2], contiguous fp32, expected")
    if hid.dim() != 3 or hid.shape[0] != 2 or hid.shape[1] < M or hid.shape[2] != 384 or not hid.is_contiguous() or code.shape[0] < M or not code.is_contiguous():
        raise _lib.WvnError("stego_head_fused: hid [2, >= M, 384] bf16 and code [>= M, ld] fp32, contiguous, expected")
    check(lib().wvn_debug_stego_head_fused(ptr(x), x.stride(0), ptr(stats), ptr(ln_g), ptr(ln_b), ptr(w_cat), ptr(b_cat), ptr(hid[0]), ptr(hid[1]), ptr(code),
                                           code.stride(0), frames, npatch, ntok_s, stream()), "wvn_debug_stego_head_fused")
    return hid, code


def qkv_fused(x: torch.Tensor, ln: Tuple[torch.Tensor, torch.Tensor, float], w: torch.Tensor, bias: Optional[torch.Tensor],
              frames: int, ntok_s: int, npad: int, q_scale: float = 0.0):
    """LayerNorm + QKV projection in one launch (csrc/qkv_fused.hip).  x [frames * ntok_s, 384] fp32, w [1152, 384] bf16 ->
    q, k [frames * 6, npad, 64] bf16 and v^T [frames * 6, 64, npad] bf16 in the attention kernel's layouts.  Slots of tokens
    >= ntok_s and the padding are left untouched (returned zero-initialised)."""
    M, heads = x.shape[0], 6
    n = frames * heads * npad * 64   # the three outputs are carved from ONE allocation: the kernel addresses them through one
    buf = torch.zeros(3 * n, dtype=torch.bfloat16, device=x.device)   # 32-bit buffer descriptor (they must lie within 2 GB)
    q, k, vt = buf[:n].view(frames * heads, npad, 64), buf[n:2 * n].view(frames * heads, npad, 64), buf[2 * n:].view(frames * heads, 64, npad)
    g, b, eps = ln
    check(lib().wvn_qkv_fused(ptr(x), x.stride(0), ptr(g), ptr(b), float(eps), ptr(w), ptr(bias), ptr(q), ptr(k), ptr(vt), heads, npad,
                              ntok_s, float(q_scale), M, stream()), "wvn_qkv_fused")
    return q, k, vt


def qkv_prenorm(xn_frag: torch.Tensor, w_perm: torch.Tensor, bias: Optional[torch.Tensor], M: int, frames: int, ntok_s: int, npad: int,
                q_scale: float = 0.0):
    """The QKV projection of ``qkv_fused`` from rows that are already normalised and laid out as operand fragments
    (``proj_mlp_resident(..., next_ln=...)`` writes them; include/wvn_hip.h).  ``w_perm = w[:, vt_token_order(384)]``."""
    heads = 6
    n = frames * heads * npad * 64
    buf = torch.zeros(3 * n, dtype=w_perm.dtype, device=w_perm.device)
    q, k, vt = buf[:n].view(frames * heads, npad, 64), buf[n:2 * n].view(frames * heads, npad, 64), buf[2 * n:].view(frames * heads, 64, npad)
    fn = lib().wvn_qkv_prenorm_f16 if w_perm.dtype == torch.float16 else lib().wvn_qkv_prenorm
    check(fn(ptr(xn_frag), ptr(w_perm), ptr(bias), ptr(q), ptr(k), ptr(vt), heads, npad, ntok_s, float(q_scale), M, stream()), "wvn_qkv_prenorm")
    return q, k, vt


def unpack_row_fragments(frag: torch.Tensor, M: int) -> torch.Tensor:
    """[M, 384] rows from the fragment layout of ``proj_mlp_resident(next_ln=...)`` (tests): fragment (R, s) holds, for lane l, row
    32 R + (l & 31), columns 16 s + 4 (l >> 5) + {0..3} and 16 s + 8 + 4 (l >> 5) + {0..3}."""
    G = (M + 31) // 32
    f = frag.view(G, 24, 2, 32, 2, 4)          # [R, s, hi, row, half, e]
    rows = f.permute(0, 3, 1, 4, 2, 5)          # [R, row, s, half, hi, e]: column = 16 s + 8 half + 4 hi + e
    return rows.reshape(G * 32, 384)[:M]


def proj_mlp_fused(attn: torch.Tensor, wp: torch.Tensor, bp: Optional[torch.Tensor], ln: Tuple[torch.Tensor, torch.Tensor, float], w1: torch.Tensor,
                   b1: Optional[torch.Tensor], w2p: torch.Tensor, b2: Optional[torch.Tensor], x: torch.Tensor,
                   ls1: Optional[torch.Tensor] = None, ls2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x += (attn @ wp^T + bp) (* ls1); x += MLP(LayerNorm(x)) in ONE launch, in place (csrc/mlp_fused.hip with the projection in its
    prologue)."""
    M, F = x.shape[0], w1.shape[0]
    g, b, eps = ln
    check(lib().wvn_proj_mlp_fused(ptr(attn), attn.stride(0), ptr(wp), ptr(bp), ptr(ls1), ptr(g), ptr(b), float(eps), ptr(w1), ptr(b1),
                                   ptr(w2p), ptr(b2), ptr(ls2), ptr(x), x.stride(0), M, F, stream()), "wvn_proj_mlp_fused")
    return x


def proj_mlp_resident(attn: torch.Tensor, wp: torch.Tensor, bp: Optional[torch.Tensor], ln: Tuple[torch.Tensor, torch.Tensor, float],
                      w1p: torch.Tensor, b1: Optional[torch.Tensor], w2p: torch.Tensor, b2: Optional[torch.Tensor], x: torch.Tensor,
                      next_ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None):
    """``proj_mlp_fused`` without LayerScale, the residual rows resident in the kernel's accumulators (x read once, written once).
    ``w1p`` = fc1.weight with its column index in the fused order: ``w1[:, vt_token_order(384)]``; bf16 or fp16 operands.
    ``next_ln=(gamma, beta, eps)``: also returns LayerNorm(x_new) as operand fragments for ``qkv_prenorm`` (x, fragments)."""
    M, F = x.shape[0], w1p.shape[0]
    g, b, eps = ln
    f16 = attn.dtype == torch.float16
    fn = lib().wvn_proj_mlp_resident_f16 if f16 else lib().wvn_proj_mlp_resident
    frag = None
    ng, nb, ne = (None, None, 0.0)
    if next_ln is not None:
        ng, nb, ne = next_ln
        frag = torch.zeros((M + 31) // 32 * 24 * 512, dtype=attn.dtype, device=x.device)
    check(fn(ptr(attn), attn.stride(0), ptr(wp), ptr(bp), ptr(g), ptr(b), float(eps), ptr(w1p), ptr(b1), ptr(w2p), ptr(b2), ptr(x),
             x.stride(0), M, F, ptr(ng), ptr(nb), float(ne), ptr(frag), stream()), "wvn_proj_mlp_resident")
    return x if next_ln is None else (x, frag)


def mlp_fused(xn: Optional[torch.Tensor], w1: torch.Tensor, b1: Optional[torch.Tensor], w2p: torch.Tensor, b2: Optional[torch.Tensor],
              x: torch.Tensor, ls: Optional[torch.Tensor] = None, ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None) -> torch.Tensor:
    """x [M,384] fp32 += gelu(xn [M,384] bf16 @ w1[F,384]^T + b1) @ w2^T + b2 in ONE launch, in place.  ``w2p`` is fc2.weight
    [384, F] with its hidden index in the fused order: ``w2[:, vt_token_order(F)]`` (include/wvn_hip.h WVN_VIT_MLP_FUSED).
    ``xn=None, ln=(gamma, beta, eps)``: the kernel normalises the rows of ``x`` itself."""
    M, F = x.shape[0], w1.shape[0]
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    if (xn is None) == (ln is None):
        raise _lib.WvnError("mlp_fused takes either xn or ln=(gamma, beta, eps)")
    check(lib().wvn_mlp_fused(ptr(xn), xn.stride(0) if xn is not None else 0, ptr(g), ptr(b), float(eps), ptr(w1), ptr(b1), ptr(w2p),
                              ptr(b2), ptr(ls), ptr(x), x.stride(0), M, F, stream()), "wvn_mlp_fused")
    return x


def vt_token_order(npad: int, device=None) -> torch.Tensor:
    """Index map of the bf16 attention kernel's V^T layout (include/wvn_hip.h): stored position p of every
    aligned group of 16 tokens holds token p with bits 2 and 3 swapped (an involution).
    ``vt_stored = v.transpose(-1, -2)[..., vt_token_order(npad)]``."""
    p = torch.arange(npad, device=device)
    return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1)


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous().float()
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().wvn_cast_f32_to_bf16(ptr(x), ptr(out), x.numel(), stream()), "wvn_cast_f32_to_bf16")
    return out


def prof_enable(on: bool) -> None:
    check(lib().wvn_prof_enable(int(on)), "wvn_prof_enable")


def prof_collect():
    n = len(_lib.PROF_CATS)
    ms = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    check(lib().wvn_prof_collect(ms, cnt), "wvn_prof_collect")
    return {c: (ms[i], cnt[i]) for i, c in enumerate(_lib.PROF_CATS)}


def cu_mask_words(cus_per_xcd_lo: int, cus_per_xcd_hi: int, layout: str = "rr", xcds: int = 8, cus_per_xcd: int = 32):
    """32-bit mask words selecting CUs [lo, hi) of every XCD.  ``layout``: how the driver numbers mask bits -- "rr": bit i is CU
    i // xcds of XCD i % xcds (amdkfd spreads a queue's mask over the XCCs round-robin), "lin": bit i is CU i % cus_per_xcd of XCD
    i // cus_per_xcd."""
    n = xcds * cus_per_xcd
    bits = 0
    for i in range(n):
        cu = i // xcds if layout == "rr" else i % cus_per_xcd
        if cus_per_xcd_lo <= cu < cus_per_xcd_hi:
            bits |= 1 << i
    return [(bits >> (32 * w)) & 0xFFFFFFFF for w in range((n + 31) // 32)]


class MaskedStream:
    """A HIP stream restricted to a set of compute units (``wvn_stream_create_cu_mask``), usable as a torch stream."""

    def __init__(self, words, device=None):
        import ctypes as C
        arr = (C.c_uint32 * len(words))(*words)
        h = C.c_void_p()
        check(lib().wvn_stream_create_cu_mask(C.byref(h), arr, len(words)), "wvn_stream_create_cu_mask")
        self.handle = h.value
        self.stream = torch.cuda.ExternalStream(self.handle, device=device)

    def close(self):
        if self.handle:
            torch.cuda.synchronize()
            check(lib().wvn_stream_destroy(self.handle), "wvn_stream_destroy")
            self.handle = None


# ---- overlays (csrc/overlay.hip; include/wvn_hip.h "overlays"; tests/visu_ref.py) -------------------------------------------
def alpha_byte(alpha) -> int:
    """``np.uint8(alpha * 255)`` of the reference's ``fore[:, :, 3] = alpha * 255`` (float64 product, truncated), clamped to a byte."""
    return max(0, min(255, int(float(alpha) * 255)))


def _overlay_frames(img: torch.Tensor, who: str) -> torch.Tensor:
    if img.dim() == 3:
        img = img[None]
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] < 1 or img.shape[3] < 1:
        raise _lib.WvnError(f"{who}: img shape must be [B,3,H,W] or [3,H,W], not {tuple(img.shape)}")
    require_cuda(img, "img")
    return img.contiguous() if img.dtype == torch.uint8 else img.contiguous().float()


def _overlay_ids(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous() if t.dtype in (torch.int32, torch.int64) else t.to(torch.int32).contiguous()


def frame_max(img: torch.Tensor) -> torch.Tensor:
    """img [B,3,H,W] fp32 or uint8 -> fp32 [B]: max(0, the frame's maximum), NaN for a frame that holds a NaN (plot_image's
    ``img.max() <= 1`` decision, left on the device)."""
    img = _overlay_frames(img, "frame_max")
    B = img.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=img.device)
    check(lib().wvn_frame_max(ptr(img), int(img.dtype == torch.uint8), B, img[0].numel(), ptr(out), stream()), "wvn_frame_max")
    return out


def _overlay_call(who, img, maps, kind, seg, lut, alpha, overlay_mask, boundary_seg, boundary_alpha, unit_range, out, plain):
    if len(maps) > _lib.OVERLAY_MAX_MAPS:
        raise _lib.WvnError(f"{who}: at most {_lib.OVERLAY_MAX_MAPS} maps per call, got {len(maps)}")
    img = _overlay_frames(img, who)
    B, _, H, W = img.shape
    dev = img.device
    d = _lib.OverlayDesc()
    keep = [img]

    def frames(t, name, ids=False):
        if t.dim() == 2:
            t = t[None]
        if tuple(t.shape) != (B, H, W):
            raise _lib.WvnError(f"{who}: {name} shape must be [B,H,W] = {(B, H, W)}, not {tuple(t.shape)}")
        require_cuda(t, name)
        t = _overlay_ids(t) if ids else t
        keep.append(t)
        return t

    if maps:
        if lut is None or lut.dim() != 2 or lut.shape[1] != 3 or not (1 <= lut.shape[0] <= _lib.OVERLAY_MAX_COLOURS):
            raise _lib.WvnError(f"{who}: lut shape must be [N,3] with 1 <= N <= {_lib.OVERLAY_MAX_COLOURS}, "
                                f"not {None if lut is None else tuple(lut.shape)}")
        require_cuda(lut, "lut")
        if lut.dtype not in (torch.uint8, torch.float32):   # (c * 255) in the table's own precision, as the reference's c_map * 255
            lut = torch.nan_to_num(lut * 255, nan=0.0).clamp(0, 255).to(torch.uint8)
        lut = lut.contiguous()
        keep.append(lut)
        d.lut, d.lut_u8, d.N = ptr(lut), int(lut.dtype == torch.uint8), lut.shape[0]
        d.kind = kind
        if kind == _lib.OVERLAY_SEGMENTS:
            seg = frames(seg, "seg", ids=True)
            d.seg, d.seg_bytes = ptr(seg), seg.element_size()
            vecs = []
            for v in maps:
                v = v[None] if v.dim() == 1 else v
                if v.dim() != 2 or v.shape[0] != B or v.shape[1] < 1 or (vecs and v.shape != vecs[0].shape):
                    raise _lib.WvnError(f"{who}: per-segment values shape must be [B,S] (B = {B}), the same for every map, not {tuple(v.shape)}")
                require_cuda(v, "values")
                vecs.append(v.contiguous().float())
            keep += vecs
            d.S = vecs[0].shape[1]
            for i, v in enumerate(vecs):
                d.maps[i] = ptr(v)
        else:
            for i, m in enumerate(maps):
                m = frames(m, "labels" if kind == _lib.OVERLAY_LABELS else "values", ids=kind == _lib.OVERLAY_LABELS)
                if kind == _lib.OVERLAY_VALUES:
                    m = m.float().contiguous()
                    keep.append(m)
                if kind == _lib.OVERLAY_LABELS:
                    if i and m.element_size() != d.id_bytes:
                        raise _lib.WvnError(f"{who}: label maps of one call share a dtype")
                    d.id_bytes = m.element_size()
                d.maps[i] = ptr(m)
        d.alpha = alpha_byte(alpha)
        if overlay_mask is not None:
            mk = frames(overlay_mask, "overlay_mask")
            mk = mk.contiguous() if mk.dtype in (torch.bool, torch.uint8) else (mk != 0)
            keep.append(mk)
            d.mask = ptr(mk)
        ba = int(boundary_alpha)
        if not 0 <= ba <= 255:
            raise _lib.WvnError(f"{who}: boundary_alpha is the alpha BYTE of the reference (0..255), not {boundary_alpha}")
        d.boundary_alpha = ba
        if boundary_seg is not None and ba > 0:
            bs = frames(boundary_seg, "boundary_seg", ids=True)
            d.boundary_seg, d.boundary_bytes = ptr(bs), bs.element_size()
    npan = plain + len(maps)
    if out is None:
        out = torch.empty(B, H, npan * W, 3, dtype=torch.uint8, device=dev)
    else:
        if out.dtype != torch.uint8 or tuple(out.shape) != (B, H, npan * W, 3) or out.device != dev or out.stride(3) != 1 \
                or out.stride(2) != 3 or out.stride(1) < 3 * npan * W or (B > 1 and out.stride(0) < H * out.stride(1)):
            raise _lib.WvnError(f"{who}: out must be a uint8 [B,H,{npan}*W,3] = {(B, H, npan * W, 3)} view on {dev} with packed pixels "
                                f"(rows and frames may be pitched), not {tuple(out.shape)} {out.dtype} strides {out.stride()}")
    d.img, d.img_u8, d.B, d.H, d.W = ptr(img), int(img.dtype == torch.uint8), B, H, W
    d.nmaps, d.plain = len(maps), plain
    if unit_range is None:
        fm = frame_max(img)
        keep.append(fm)
        d.frame_max, d.unit_range = ptr(fm), -1
    else:
        d.unit_range = int(bool(unit_range))
    d.out, d.out_row_bytes, d.out_frame_bytes = ptr(out), out.stride(1), out.stride(0)
    fn = lib().wvn_overlay_panels if plain else lib().wvn_overlay
    check(fn(C.byref(d), stream()), "wvn_overlay_panels" if plain else "wvn_overlay")
    return out


def image_to_u8(img: torch.Tensor, unit_range: Optional[bool] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """plot_image (visualizer.py:516-537) on the device: img [B,3,H,W] (or [3,H,W]) fp32 / uint8 -> uint8 [B,H,W,3].  A frame
    whose maximum is <= 1 is multiplied by 255 (``unit_range`` True / False states the range and skips the reduction), then
    truncated; outside [0, 255]: clamped, NaN -> 0."""
    return _overlay_call("image_to_u8", img, [], 0, None, None, 0, None, None, 0, unit_range, out, 1)


def _overlay_kind(who, values, labels, seg):
    if (values is None) == (labels is None) or (labels is not None and seg is not None):
        raise _lib.WvnError(f"{who}: pass values [B,H,W], labels [B,H,W], or values [B,S] with seg [B,H,W]")
    return _lib.OVERLAY_LABELS if labels is not None else (_lib.OVERLAY_SEGMENTS if seg is not None else _lib.OVERLAY_VALUES)


def overlay(img: torch.Tensor, values: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
            seg: Optional[torch.Tensor] = None, lut: Optional[torch.Tensor] = None, alpha: float = 0.5,
            overlay_mask: Optional[torch.Tensor] = None, boundary_seg: Optional[torch.Tensor] = None, boundary_alpha: int = 0,
            unit_range: Optional[bool] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's overlay pictures in one launch -> uint8 [B,H,W,3] (include/wvn_hip.h "overlays" is the definition).
    ``values`` [B,H,W] float: index (v * 255) truncated and clipped (plot_detectron_classification); ``labels`` [B,H,W] int: the
    index itself (plot_segmentation / plot_detectron); ``values`` [B,S] with ``seg`` [B,H,W]: (values[seg] * 255) truncated, ids
    in [-S, 0) wrapping (plot_traversability_graph_on_seg).  ``lut`` [N,3], N <= 1024, floats in [0,1] or uint8.  An index outside
    the table leaves the plain pixel.  ``alpha``: the reference's float (its byte is ``alpha_byte``); ``overlay_mask`` pixels get
    no overlay; ``boundary_seg`` with ``boundary_alpha`` (a byte, 0 = off) composites white over 4-neighbour label edges.
    ``out``: a uint8 [B,H,W,3] view, e.g. a column slice of a wider image."""
    kind = _overlay_kind("overlay", values, labels, seg)
    return _overlay_call("overlay", img, [labels if labels is not None else values], kind, seg, lut, alpha, overlay_mask,
                         boundary_seg, boundary_alpha, unit_range, out, 0)


def overlay_panels(img: torch.Tensor, maps, lut: Optional[torch.Tensor] = None, alpha: float = 0.5, labels: bool = False,
                   seg: Optional[torch.Tensor] = None, overlay_mask: Optional[torch.Tensor] = None,
                   boundary_seg: Optional[torch.Tensor] = None, boundary_alpha: int = 0, unit_range: Optional[bool] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[plain frame | overlay of maps[0] | overlay of maps[1] | ...] side by side, uint8 [B,H,(1 + len(maps)) * W,3], the frame
    converted once, one launch (quick_start.py's ``plot_list([original, conf, trav])``).  ``maps``: up to 4 value maps [B,H,W]
    (label maps with ``labels=True``, per-segment vectors [B,S] with ``seg``); the other arguments as ``overlay``."""
    maps = list(maps)
    kind = _lib.OVERLAY_LABELS if labels else (_lib.OVERLAY_SEGMENTS if seg is not None else _lib.OVERLAY_VALUES)
    return _overlay_call("overlay_panels", img, maps, kind, seg, lut, alpha, overlay_mask, boundary_seg, boundary_alpha, unit_range,
                         out, 1)


# ---- overlays: vector primitives (csrc/draw.hip; include/wvn_hip.h "overlays: vector primitives"; tests/visu_draw_ref.py) ------
def draw(canvas: torch.Tensor, kinds: torch.Tensor, points: torch.Tensor, colours: torch.Tensor, frame: Optional[torch.Tensor] = None,
         panel: Optional[torch.Tensor] = None, panel_width: Optional[int] = None, skipped: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL.ImageDraw's thin line, 2-pixel line and +-5 ellipse, bit for bit, IN PLACE on ``canvas``: a uint8 [B,H,P*Wp,3] (or
    [H,P*Wp,3]) device tensor or view with packed pixels (rows and frames may be pitched: an overlay result, a column slice).
    ``kinds`` [N] (``DRAW_LINE`` / ``DRAW_LINE2`` / ``DRAW_DISC``), ``points`` [N,4] = x0, y0, x1, y1 in panel-local pixels (a
    disc reads its centre x0, y0), ``colours`` [N,3] uint8, ``frame`` and ``panel`` [N] (default 0), ``panel_width`` Wp (default:
    the whole width).  One launch; the highest-index primitive covering a pixel wins.  A primitive with a coordinate that is not
    finite or truncates outside [-32768, 32767], or with a frame / panel outside the canvas, is skipped and added to ``skipped``
    (int32 [1], optional).  Returns ``canvas``."""
    require_cuda(canvas, "canvas")
    c4 = canvas[None] if canvas.dim() == 3 else canvas
    if c4.dim() != 4 or c4.dtype != torch.uint8 or c4.shape[3] != 3 or min(c4.shape[:3]) < 1:
        raise _lib.WvnError(f"draw: canvas must be uint8 [B,H,W,3] or [H,W,3], not {tuple(canvas.shape)} {canvas.dtype}")
    B, H, Wc, _ = c4.shape
    Wp = Wc if panel_width is None else int(panel_width)
    if Wp < 1 or Wc % Wp:
        raise _lib.WvnError(f"draw: panel_width {panel_width} does not divide the canvas width {Wc}")
    if c4.stride(3) != 1 or c4.stride(2) != 3 or c4.stride(1) < 3 * Wc or (B > 1 and c4.stride(0) < H * c4.stride(1)):
        raise _lib.WvnError(f"draw: canvas needs packed pixels (rows and frames may be pitched), strides {canvas.stride()}")
    dev = canvas.device
    N = int(kinds.shape[0])
    if kinds.dim() != 1 or tuple(points.shape) != (N, 4) or tuple(colours.shape) != (N, 3) or colours.dtype != torch.uint8:
        raise _lib.WvnError(f"draw: kinds [N], points [N,4], colours uint8 [N,3]; got {tuple(kinds.shape)}, {tuple(points.shape)}, "
                            f"{tuple(colours.shape)} {colours.dtype}")
    if N > _lib.DRAW_MAX_PRIMITIVES:
        raise _lib.WvnError(f"draw: at most {_lib.DRAW_MAX_PRIMITIVES} primitives per call, got {N}")

    def ints(t, name):
        if t is None:
            return torch.zeros(N, dtype=torch.int32, device=dev)
        if tuple(t.shape) != (N,):
            raise _lib.WvnError(f"draw: {name} shape must be [N] = {(N,)}, not {tuple(t.shape)}")
        require_cuda(t, name)
        return t.to(torch.int32).contiguous()

    for t, name in ((kinds, "kinds"), (points, "points"), (colours, "colours")):
        require_cuda(t, name)
    keep = [ints(kinds, "kinds"), points.float().contiguous(), colours.contiguous(), ints(frame, "frame"), ints(panel, "panel")]
    d = _lib.DrawDesc()
    d.canvas, d.row_bytes, d.frame_bytes = ptr(c4), c4.stride(1), c4.stride(0)
    d.kinds, d.points, d.colours, d.frame, d.panel = (ptr(t) for t in keep)
    if skipped is not None:
        require_cuda(skipped, "skipped")
        if skipped.dtype != torch.int32 or skipped.numel() != 1:
            raise _lib.WvnError(f"draw: skipped must be int32 [1], not {tuple(skipped.shape)} {skipped.dtype}")
        d.skipped = ptr(skipped)
    d.B, d.H, d.P, d.Wp, d.N = B, H, Wc // Wp, Wp, N
    check(lib().wvn_draw(C.byref(d), stream()), "wvn_draw")
    return canvas


# ---- evaluation metrics (csrc/metrics.hip; include/wvn_hip.h "evaluation metrics"; tests/metrics_ref.py) ----------------------
class PerSegment:
    """Marks a source of ``metric_accumulate`` as a per-segment table, gathered through ``seg`` on load: ``[B,S]`` (row b S + s),
    or with ``seg_off`` any tensor whose first dimension is the concatenated segments (row seg_off[b] + s; column 0 of a matrix)."""

    def __init__(self, table: torch.Tensor):
        self.table = table


def metric_state_words(T: int) -> int:
    return 2 * (int(T) + 1) + _lib.METRIC_STATE_TAIL


def metric_state(n_pairs: int, T: int, device) -> torch.Tensor:
    """Zeroed pair states int64 [n_pairs][2 (T + 1) + 8]: hist [T+1][2], cm [2][2], n_nan, n_ignored, n_out_of_range, reserved."""
    return torch.zeros(int(n_pairs), metric_state_words(T), dtype=torch.int64, device=device)


_METRIC_DTYPES = {torch.uint8: _lib.METRIC_U8, torch.bool: _lib.METRIC_U8, torch.int32: _lib.METRIC_I32, torch.float32: _lib.METRIC_F32}


def metric_accumulate(state: torch.Tensor, thresholds: torch.Tensor, scores, targets, seg: Optional[torch.Tensor] = None,
                      seg_off: Optional[torch.Tensor] = None, tau: float = 0.5, ignore_index: Optional[int] = None,
                      seg_counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fused pixel pass: every (score, target) pair state of ``state`` [len(scores) * len(targets)][words] is added into, in one
    launch.  A source is a dense map ``[B,H,W]`` / ``[N]`` (fp32 scores; uint8, bool, int32 or fp32 targets) or ``PerSegment(table)``
    with ``seg`` ``[B,H,W]`` (int32 or int64 ids, read as they are).  ``seg_counts`` int32 ``[rows][len(targets)][2]`` (optional) receives the per-segment class counts."""
    scores, targets = list(scores), list(targets)
    if not 1 <= len(scores) <= 2 or not 1 <= len(targets) <= 2:
        raise _lib.WvnError("metric_accumulate: one or two scores and one or two targets per call")
    require_cuda(state, "state")
    require_cuda(thresholds, "thresholds")
    T = thresholds.numel()
    if thresholds.dtype != torch.float32 or not thresholds.is_contiguous():
        raise _lib.WvnError("metric_accumulate: thresholds must be a contiguous fp32 vector")
    words = metric_state_words(T)
    if state.dtype != torch.int64 or state.dim() != 2 or state.shape[0] != len(scores) * len(targets) or state.shape[1] < words \
            or state.stride(1) != 1:
        raise _lib.WvnError(f"metric_accumulate: state must be int64 [{len(scores) * len(targets)}][>= {words}]")
    shape = None
    if seg is not None:
        require_cuda(seg, "seg")
        if seg.dim() == 2:
            seg = seg[None]
        if seg.dim() != 3:
            raise _lib.WvnError(f"metric_accumulate: seg must be [B,H,W], not {tuple(seg.shape)}")
        seg = (seg if seg.dtype in (torch.int32, torch.int64) else _i32(seg)).contiguous()   # int64 ids (the reference's graphs) are read as they are
        shape = tuple(seg.shape)
    for t in scores + targets:
        if not isinstance(t, PerSegment):
            sh = tuple(t.shape) if t.dim() == 3 else (1, 1, t.numel())
            if t.dim() not in (1, 3):
                raise _lib.WvnError(f"metric_accumulate: a dense source must be [B,H,W] or [N], not {tuple(t.shape)}")
            if shape is None:
                shape = sh
            if sh != shape:
                raise _lib.WvnError(f"metric_accumulate: source shapes differ: {sh} and {shape}")
    if shape is None:
        raise _lib.WvnError("metric_accumulate: per-segment sources need seg")
    B, H, W = shape
    d = _lib.MetricDesc()
    keep = []
    S = 0
    table_rows = []   # with seg_off: the rows of every per-segment table (and of seg_counts) must agree
    if seg_off is not None:
        require_cuda(seg_off, "seg_off")
        seg_off = seg_off.to(torch.int64).contiguous()
        if seg_off.numel() != B + 1:
            raise _lib.WvnError(f"metric_accumulate: seg_off must hold B + 1 = {B + 1} offsets")
        keep.append(seg_off)

    def source(t, name, is_score):
        nonlocal S
        if isinstance(t, PerSegment):
            tab = t.table
            require_cuda(tab, name)
            if seg is None:
                raise _lib.WvnError(f"metric_accumulate: {name} is per-segment but seg is missing")
            if seg_off is None:
                if tab.dim() != 2 or tab.shape[0] != B:
                    raise _lib.WvnError(f"metric_accumulate: per-segment {name} must be [B,S] (or pass seg_off), not {tuple(tab.shape)}")
                if S and tab.shape[1] != S:
                    raise _lib.WvnError("metric_accumulate: per-segment sources differ in S")
                S = int(tab.shape[1])
                tab = tab.contiguous()
                stride = 1
            else:
                if tab.dim() == 2:
                    tab = tab[:, 0]
                if tab.dim() != 1:
                    raise _lib.WvnError(f"metric_accumulate: per-segment {name} must be [N] or [N,C] with seg_off")
                table_rows.append(int(tab.shape[0]))
                stride = int(tab.stride(0)) if tab.numel() > 1 else 1
                if stride < 1:
                    tab, stride = tab.contiguous(), 1
            kind = _lib.METRIC_PER_SEGMENT
        else:
            require_cuda(t, name)
            tab, stride, kind = t.contiguous(), 1, _lib.METRIC_DENSE
        if is_score:
            if tab.dtype != torch.float32:
                tab = tab.float()
                stride = int(tab.stride(0)) if (kind == _lib.METRIC_PER_SEGMENT and tab.dim() == 1 and tab.numel() > 1) else 1
            dt = _lib.METRIC_F32
        else:
            if tab.dtype not in _METRIC_DTYPES:
                if tab.dtype.is_floating_point:
                    tab = tab.float()
                else:   # wider integers: every value that is no label becomes one value that is none
                    keepv = (tab == 0) | (tab == 1)
                    if ignore_index is not None:
                        keepv = keepv & (tab != int(ignore_index))
                    tab = torch.where(keepv, tab, torch.full_like(tab, 2)).to(torch.uint8)
                if kind == _lib.METRIC_PER_SEGMENT and tab.dim() == 1 and tab.numel() > 1:
                    stride = int(tab.stride(0))
            dt = _METRIC_DTYPES[tab.dtype]
        keep.append(tab)
        return ptr(tab), kind, stride, dt

    for i, t in enumerate(scores):
        d.score[i], d.score_kind[i], d.score_stride[i], _ = source(t, f"scores[{i}]", True)
    for j, t in enumerate(targets):
        d.target[j], d.target_kind[j], d.target_stride[j], d.target_dtype[j] = source(t, f"targets[{j}]", False)
    if seg is not None and seg_off is None and S == 0:
        S = 1 if seg_counts is None else int(seg_counts.shape[0]) // B
    if seg_counts is not None:
        require_cuda(seg_counts, "seg_counts")
        if seg is None or seg_counts.dtype != torch.int32 or not seg_counts.is_contiguous() or seg_counts.dim() != 3 \
                or tuple(seg_counts.shape[1:]) != (len(targets), 2) or (seg_off is None and seg_counts.shape[0] != B * S):
            raise _lib.WvnError(f"metric_accumulate: seg_counts must be contiguous int32 [rows][{len(targets)}][2] and needs seg")
        if seg_off is not None:
            table_rows.append(int(seg_counts.shape[0]))
    if len(set(table_rows)) > 1:
        raise _lib.WvnError(f"metric_accumulate: the per-segment tables and seg_counts differ in their rows: {table_rows}")
    if ignore_index is not None and not -2 ** 31 <= int(ignore_index) < 2 ** 31:
        raise _lib.WvnError("metric_accumulate: ignore_index must fit 32 bits")
    d.seg, d.seg_off, d.thresholds, d.state, d.seg_counts = ptr(seg), ptr(seg_off), ptr(thresholds), ptr(state), ptr(seg_counts)
    d.state_stride = int(state.stride(0))
    d.tau = float(tau)
    d.n_scores, d.n_targets, d.B, d.H, d.W, d.S, d.T = len(scores), len(targets), B, H, W, S, T
    d.has_ignore, d.ignore_index = int(ignore_index is not None), int(ignore_index or 0)
    d.seg_bytes = 0 if seg is None else seg.element_size()
    check(lib().wvn_metric_accumulate(C.byref(d), stream()), "wvn_metric_accumulate")
    return state


def metric_curve(state: torch.Tensor, thresholds: torch.Tensor):
    """One pair state (int64 [words]) -> (fpr, tpr, thresholds) fp64 [T] in ascending fpr, scal fp64 [2] = {binned AUROC, accuracy},
    cnt int64 [3] = {P, N, degenerate}: all on the device, one launch."""
    require_cuda(state, "state")
    require_cuda(thresholds, "thresholds")
    T = thresholds.numel()
    if state.dtype != torch.int64 or state.dim() != 1 or state.numel() < metric_state_words(T) or not state.is_contiguous():
        raise _lib.WvnError(f"metric_curve: state must be a contiguous int64 vector of >= {metric_state_words(T)} words")
    if thresholds.dtype != torch.float32 or not thresholds.is_contiguous():
        raise _lib.WvnError("metric_curve: thresholds must be a contiguous fp32 vector")
    dev = state.device
    curves = torch.empty(3, T, dtype=torch.float64, device=dev)
    scal = torch.empty(2, dtype=torch.float64, device=dev)
    cnt = torch.empty(3, dtype=torch.int64, device=dev)
    check(lib().wvn_metric_curve(ptr(state), ptr(thresholds), T, ptr(curves[0]), ptr(curves[1]), ptr(curves[2]), ptr(scal), ptr(cnt),
                                 stream()), "wvn_metric_curve")
    return curves[0], curves[1], curves[2], scal, cnt


def metric_auroc_weighted(score: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor):
    """Exact AUROC of weighted entries (score fp32, pos / neg pixel counts) -> scal fp64 [1], cnt int64 [4] = {U2, P, N, degenerate}.
    The entries are sorted here (torch.sort: plumbing); ties, prefixes and U2 are the kernel's.  No entries: the degenerate result."""
    require_cuda(score, "score")
    require_cuda(pos, "pos")
    require_cuda(neg, "neg")
    E = score.numel()
    if pos.numel() != E or neg.numel() != E:
        raise _lib.WvnError("metric_auroc_weighted: score, pos and neg differ in length")
    if E > 2 ** 24:
        raise _lib.WvnError(f"metric_auroc_weighted: at most 2^24 entries, got {E}")
    dev = score.device
    scal = torch.zeros(1, dtype=torch.float64, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    if E == 0:
        cnt[3] = 1
        return scal, cnt
    s, order = torch.sort(score.reshape(-1).float(), descending=True)
    p = pos.reshape(-1).to(torch.int64)[order].contiguous()
    n = neg.reshape(-1).to(torch.int64)[order].contiguous()
    check(lib().wvn_metric_auroc_weighted(ptr(s), ptr(p), ptr(n), E, ptr(scal), ptr(cnt), stream()), "wvn_metric_auroc_weighted")
    return scal, cnt


# ---- JPEG ingest (include/wvn_hip.h: "JPEG ingest"; csrc/jpeg_host.cpp + csrc/jpeg.hip) ----
def _jpeg_buffers(frames, who: str):
    """bytes / bytearray / memoryview / uint8 CPU tensor, or a list of those -> [numpy uint8 views] (no copy; the views keep the bytes alive)."""
    import numpy as np

    if isinstance(frames, (bytes, bytearray, memoryview, torch.Tensor)) or hasattr(frames, "__array_interface__"):
        frames = [frames]
    out = []
    for i, f in enumerate(frames):
        if isinstance(f, torch.Tensor):
            if f.is_cuda or f.dtype != torch.uint8 or f.dim() != 1:
                raise _lib.WvnError(f"{who}: frame {i}: a 1-d uint8 CPU tensor of the file's bytes expected, got {f.dtype} {tuple(f.shape)} on {f.device}")
            a = f.contiguous().numpy()
        elif isinstance(f, (bytes, bytearray, memoryview)):
            a = np.frombuffer(f, dtype=np.uint8)
        elif hasattr(f, "__array_interface__"):
            a = np.ascontiguousarray(f)
            if a.dtype != np.uint8 or a.ndim != 1:
                raise _lib.WvnError(f"{who}: frame {i}: a 1-d uint8 array of the file's bytes expected, got {a.dtype} {a.shape}")
        else:
            raise _lib.WvnError(f"{who}: frame {i}: bytes, bytearray or a uint8 CPU tensor expected, got {type(f).__name__}")
        if a.size == 0:
            raise _lib.WvnError(f"{who}: frame {i} is empty")
        out.append(a)
    if not out:
        raise _lib.WvnError(f"{who}: no frames")
    return out


def jpeg_status_name(status: int) -> str:
    return "WVN_JPEG_" + _lib.JPEG_STATUS[status] if 0 <= status < len(_lib.JPEG_STATUS) else f"status {status}"


def _jpeg_info(a):
    g = _lib.JpegGeometry()
    return lib().wvn_jpeg_info(a.ctypes.data, a.size, C.byref(g)), g


def jpeg_info(data) -> dict:
    """Header of one JPEG stream (host only): {"width", "height", "components", "sampling": "gray" | "4:4:4" | "4:2:2" | "4:2:0",
    "restart_interval"}.  WvnError naming the status for a stream the decoder refuses (its tables and scan header are checked too)."""
    (a,) = _jpeg_buffers(data, "jpeg_info")
    rc, g = _jpeg_info(a)
    if rc != _lib.JPEG_OK:
        raise _lib.WvnError(f"jpeg_info: {jpeg_status_name(rc)}" if rc < 1000 else "jpeg_info: bad argument")
    return {"width": g.width, "height": g.height, "components": g.components, "sampling": _lib.JPEG_SAMPLING[g.sampling],
            "restart_interval": g.restart_interval}


def jpeg_coefficients(data):
    """The host stage alone, for one frame: (status, coef int16 [blocks, 64] quantised and in natural order, component after
    component, qtables int32 [3, 64] in natural order, geometry or None).  CPU tensors; nothing touches the GPU."""
    (a,) = _jpeg_buffers(data, "jpeg_coefficients")
    rc, g = _jpeg_info(a)
    if rc != _lib.JPEG_OK:
        return rc, None, None, None
    n = lib().wvn_jpeg_coef_bytes(C.byref(g))
    coef = torch.empty(n // 128, 64, dtype=torch.int16)
    qt = torch.empty(3, 64, dtype=torch.int16)
    rc = lib().wvn_jpeg_coefficients(a.ctypes.data, a.size, C.byref(g), coef.data_ptr(), n, qt.data_ptr())
    if rc >= 1000:
        check(rc, "wvn_jpeg_coefficients")
    return rc, coef, qt.to(torch.int32) & 0xFFFF, g


def jpeg_decode(frames, device, *, gray: bool = False, threads: int = 8, strict: bool = True):
    """Baseline JPEG streams -> (uint8 [B,3,H,W] on `device`, status int32 [B] on the CPU), bit-identical to libjpeg's default decode
    (Pillow, cv2.imdecode up to its BGR order): the Huffman stage on `threads` host workers (default 8, at most 16), inverse DCT,
    fancy chroma upsampling and YCbCr -> RGB in two HIP kernels on the current stream.  ``frames``: bytes, bytearray, a uint8 CPU
    tensor, or a list of those; all frames of a call share size, sampling and component count (WvnError before anything runs
    otherwise).  ``gray=True``: [B,1,H,W], one-component files only.  ``strict=True`` raises WvnError naming the first failing frame and
    its status; ``strict=False`` returns such a frame all zero with its status (jpeg_status_name), its neighbours untouched -- but a
    batch in which NO frame has a readable header raises even then: without one geometry there is no frame size to return."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.WvnError(f"jpeg_decode: device must be a GPU (got {device}); the HIP path has no CPU fallback")
    threads = int(threads)
    if not 1 <= threads <= _lib.JPEG_MAX_THREADS:
        raise _lib.WvnError(f"jpeg_decode: threads={threads} must lie in [1, {_lib.JPEG_MAX_THREADS}]")
    bufs = _jpeg_buffers(frames, "jpeg_decode")
    B = len(bufs)
    if B > _lib.JPEG_MAX_BATCH:
        raise _lib.WvnError(f"jpeg_decode: {B} frames in one call; at most {_lib.JPEG_MAX_BATCH}")
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in bufs])
    sizes = (C.c_size_t * B)(*[a.size for a in bufs])
    status = (C.c_int * B)()
    # the geometry of every frame in one host call (markers and lengths up to SOS; the tables are built once, by the decode)
    geos = (_lib.JpegGeometry * B)()
    check(lib().wvn_jpeg_probe_batch(ptrs, sizes, B, geos, status), "wvn_jpeg_probe_batch")
    geo = None
    for i in range(B):
        g = geos[i]
        if status[i] != _lib.JPEG_OK:
            if strict:
                raise _lib.WvnError(f"jpeg_decode: frame {i}: {jpeg_status_name(status[i])}")
            continue
        if geo is None:
            geo, first = g, i
        elif (g.width, g.height, g.components, g.sampling) != (geo.width, geo.height, geo.components, geo.sampling):
            def _d(x):
                return f"{x.width}x{x.height} {_lib.JPEG_SAMPLING[x.sampling]}"
            raise _lib.WvnError(f"jpeg_decode: mixed geometry in one batch: frame {first} is {_d(geo)}, frame {i} is {_d(g)}; "
                                "group the frames and decode each group")
    if geo is None:
        raise _lib.WvnError("jpeg_decode: no frame of the batch has a readable header: the frame size is unknown")
    if gray and geo.components != 1:
        raise _lib.WvnError("jpeg_decode: gray=True needs one-component (grayscale) files")
    with torch.cuda.device(device):
        out = torch.empty(B, 1 if gray else 3, geo.height, geo.width, dtype=torch.uint8, device=device)
        ws = torch.empty(lib().wvn_jpeg_workspace_bytes(C.byref(geo), B), dtype=torch.uint8, device=device)
        check(lib().wvn_jpeg_decode_batch(ptrs, sizes, B, C.byref(geo), ptr(out), int(gray), ptr(ws), threads, status, stream()),
              "wvn_jpeg_decode_batch")
    st = torch.tensor(list(status), dtype=torch.int32)
    if strict:
        for i, rc in enumerate(status):
            if rc != _lib.JPEG_OK:
                raise _lib.WvnError(f"jpeg_decode: frame {i}: {jpeg_status_name(rc)}")
    return out, st


# ---- Raw camera ingest (include/wvn_hip.h: "Raw camera ingest"; csrc/rectify.hip; the definition: tests/rectify_ref.py) ----
DISTORTION_MODELS = ("plumb_bob", "equidistant")
_RECTIFY_Q = 32   # Q5, OpenCV's INTER_BITS


class RectifyMap:
    """The rectification of one camera geometry: ``qx``, ``qy`` int32 [h,w] on the device (Q5 source coordinates of every output
    pixel), ``src_size`` (H, W), ``out_size`` (h, w) and ``K_new`` (3 x 3 float64 numpy), the pinhole matrix of the RECTIFIED frames:
    the one ImageProjector must be given, not the sensor's K.  ``K_tensor`` is K_new as ros_cam_info_to_tensors shapes it."""

    def __init__(self, qx: torch.Tensor, qy: torch.Tensor, src_size, out_size, K_new):
        self.qx, self.qy, self.src_size, self.out_size, self.K_new = qx, qy, tuple(src_size), tuple(out_size), K_new

    @property
    def K_tensor(self) -> torch.Tensor:
        """[1,4,4] fp32 on the map's device (ros_converter.py:86-92)."""
        K = torch.eye(4, dtype=torch.float32)
        K[:3, :3] = torch.from_numpy(self.K_new).to(torch.float32)
        return K.unsqueeze(0).to(self.qx.device)


_RECTIFY_CACHE = {}


def _rectify_map_host(K, D, model: str, src_size, out_size, new_K, Rm):
    """The map in float64 numpy, operation by operation as tests/rectify_ref.py states it -> (qx, qy) int32 [h,w]."""
    import numpy as np

    (H, W), (h, w) = src_size, out_size
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        M = Rm.T @ np.linalg.inv(new_K)
        X, Y, Z = (M[i, 0] * u + M[i, 1] * v + M[i, 2] for i in range(3))
        x, y = X / Z, Y / Z
        if model == "plumb_bob":
            k1, k2, p1, p2, k3 = D
            r2 = x * x + y * y
            rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        else:
            k1, k2, k3, k4 = D
            r = np.sqrt(x * x + y * y)
            t = np.arctan(r)
            t2 = t * t
            td = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r == 0, 1.0, td / np.where(r == 0, 1.0, r))
            xd, yd = x * s, y * s
        sx = K[0, 0] * xd + K[0, 2]
        sy = K[1, 1] * yd + K[1, 2]
        # bounded, so that the stored integers are: anything at or beyond -2 / W + 1 has all four taps outside anyway
        sx = np.clip(np.where(np.isfinite(sx), sx, -2.0), -2, W + 1)
        sy = np.clip(np.where(np.isfinite(sy), sy, -2.0), -2, H + 1)
    return np.rint(_RECTIFY_Q * sx).astype(np.int32), np.rint(_RECTIFY_Q * sy).astype(np.int32)


def _size2(size, what: str):
    try:
        a, b = (int(v) for v in size)
    except (TypeError, ValueError):
        raise _lib.WvnError(f"rectify_map: {what} must be (height, width), got {size!r}") from None
    if not (1 <= a <= _lib.FRAME_MAX_DIM and 1 <= b <= _lib.FRAME_MAX_DIM):
        raise _lib.WvnError(f"rectify_map: {what}={(a, b)}: each side must lie in [1, {_lib.FRAME_MAX_DIM}]")
    return a, b


def _mat3(M, what: str):
    import numpy as np

    try:
        a = np.array(M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M, dtype=np.float64)
    except (TypeError, ValueError):
        raise _lib.WvnError(f"rectify_map: {what} must hold 9 numbers") from None
    if a.size != 9 or not np.isfinite(a).all():
        raise _lib.WvnError(f"rectify_map: {what} must hold 9 finite numbers, got shape {a.shape}")
    return a.reshape(3, 3)


def rectify_map(K, D, model: str, src_size, out_size=None, new_K=None, R=None, device="cuda") -> RectifyMap:
    """The rectification map of one camera: sensor matrix ``K`` (3 x 3), distortion ``D`` of ``model`` "plumb_bob" (k1, k2, p1, p2[,
    k3]) or "equidistant" (k1..k4, the fisheye model), source size (H, W) -> RectifyMap for output size ``out_size`` (default: the
    source's) under the pinhole matrix ``new_K`` (default: K scaled to the output size by the width and height ratios, image_proc's
    P = K) and the rectifying rotation ``R`` (default identity).  Computed once per geometry on the host in float64 and cached."""
    import numpy as np

    if model not in DISTORTION_MODELS:
        raise _lib.WvnError(f"rectify_map: distortion model {model!r} is not supported; the models are {', '.join(DISTORTION_MODELS)}")
    try:
        Dv = [float(d) for d in D]
    except (TypeError, ValueError):
        raise _lib.WvnError("rectify_map: D must be a sequence of numbers") from None
    if model == "plumb_bob" and len(Dv) == 4:
        Dv.append(0.0)
    want = 5 if model == "plumb_bob" else 4
    if len(Dv) != want or not all(np.isfinite(Dv)):
        raise _lib.WvnError(f"rectify_map: {model} takes {'4 or 5' if want == 5 else '4'} finite coefficients, got {len(list(D))}")
    src = _size2(src_size, "src_size")
    out = src if out_size is None else _size2(out_size, "out_size")
    Km = _mat3(K, "K")
    Kn = np.diag([out[1] / src[1], out[0] / src[0], 1.0]) @ Km if new_K is None else _mat3(new_K, "new_K")
    Rm = np.eye(3) if R is None else _mat3(R, "R")
    if abs(np.linalg.det(Kn)) < 1e-300:
        raise _lib.WvnError("rectify_map: new_K is singular")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.WvnError(f"rectify_map: device must be a GPU (got {device}); the HIP path has no CPU fallback")
    key = (Km.tobytes(), tuple(Dv), model, src, out, Kn.tobytes(), Rm.tobytes(), str(device))
    m = _RECTIFY_CACHE.get(key)
    if m is None:
        qx, qy = _rectify_map_host(Km, Dv, model, src, out, Kn, Rm)
        m = RectifyMap(torch.from_numpy(qx).to(device), torch.from_numpy(qy).to(device), src, out, Kn)
        _RECTIFY_CACHE[key] = m
    return m


def rectify_map_from_camera_info(height, width, distortion_model, D, K, R, P, out_size=None, device="cuda") -> RectifyMap:
    """rectify_map from the fields of a sensor_msgs/CameraInfo, as plain sequences: K_new is the left 3 x 3 of ``P`` (scaled by the
    width and height ratios when ``out_size`` differs from (height, width); K itself where P is all zero, an uncalibrated message).  An
    empty model name or an all-zero (or empty) D is the identity distortion; any other model than plumb_bob / equidistant is refused."""
    import numpy as np

    Dv = [float(d) for d in D]
    model = distortion_model
    if model == "" or not any(Dv):
        if model not in ("",) + DISTORTION_MODELS:
            raise _lib.WvnError(f"rectify_map: distortion model {model!r} is not supported; the models are {', '.join(DISTORTION_MODELS)}")
        model, Dv = "plumb_bob", [0.0] * 5
    Pm = np.array(P, dtype=np.float64)
    if Pm.size != 12:
        raise _lib.WvnError(f"rectify_map: P must hold 12 numbers, got {Pm.size}")
    Kn = Pm.reshape(3, 4)[:, :3] if Pm.any() else _mat3(K, "K")
    src = _size2((height, width), "(height, width)")
    out = src if out_size is None else _size2(out_size, "out_size")
    Kn = np.diag([out[1] / src[1], out[0] / src[0], 1.0]) @ Kn
    return rectify_map(K, Dv, model, src, out, Kn, R if len(R) else None, device)


def _bytes_per_pixel(encoding: str) -> int:
    return 3 if encoding in ("rgb8", "bgr8") else 1


def _frame_source(frames: torch.Tensor, encoding: str, step, width, channels, who: str):
    """-> (contiguous uint8 tensor, kind, B, H, W, step, frame_stride); refusals raise before the device is looked at."""
    if encoding not in _lib.SRC_KINDS:
        raise _lib.WvnError(f"{who}: encoding {encoding!r} is not supported; the source kinds are {', '.join(_lib.SRC_KINDS)}")
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise _lib.WvnError(f"{who}: a uint8 tensor expected, got {getattr(frames, 'dtype', type(frames).__name__)}")
    bpp = _bytes_per_pixel(encoding)
    packed, planar = bpp == 3, encoding == "planar"
    if step is not None:
        # rows of `step` bytes as the message carries them: [B,H,step] or [H,step], the width given apart
        if planar:
            raise _lib.WvnError(f"{who}: step applies to the camera encodings, not to planar frames")
        if width is None:
            raise _lib.WvnError(f"{who}: step needs width (the rows are [.., H, step] bytes)")
        if frames.dim() == 2:
            frames = frames[None]
        if frames.dim() != 3:
            raise _lib.WvnError(f"{who}: with step, frames are [B,H,step] or [H,step] bytes, got {tuple(frames.shape)}")
        B, H, got = frames.shape
        W, step = int(width), int(step)
        if got != step:
            raise _lib.WvnError(f"{who}: rows of {got} bytes, but step={step}")
        if W < 1 or step < W * bpp:
            raise _lib.WvnError(f"{who}: step={step} is smaller than a row of {W} pixels ({W * bpp} bytes)")
    else:
        nd = 3 + int(packed or planar)
        if frames.dim() == nd - 1:
            frames = frames[None]
        if frames.dim() != nd or (packed and frames.shape[3] != 3) or (planar and frames.shape[1] != 3):
            shape = "[B,H,W,3]" if packed else "[B,3,H,W]" if planar else "[B,H,W]"
            raise _lib.WvnError(f"{who}: {encoding} frames are {shape} (or one frame without B), got {tuple(frames.shape)}")
        B, H, W = (frames.shape[0], frames.shape[2], frames.shape[3]) if planar else frames.shape[:3]
        step = W * bpp
    least = 3 if encoding.startswith("bayer") else 1
    if B < 1 or H < least or W < least:
        raise _lib.WvnError(f"{who}: {encoding} frames need B >= 1 and H, W >= {least}, got B={B}, {H} x {W}")
    _out_order(encoding, False, channels, who)
    require_cuda(frames, "frames")
    return frames.contiguous(), _lib.SRC_KINDS[encoding], B, H, W, step, (3 if planar else 1) * H * step


def _out_order(encoding: str, bgr: bool, channels, who: str):
    if channels not in (None, 1, 3) or (channels == 1 and encoding != "mono8"):
        raise _lib.WvnError(f"{who}: channels={channels!r}: None or 3, or 1 for mono8")
    if encoding == "mono8" and channels != 3:
        return 1, _lib.ORDER_GRAY
    return 3, _lib.ORDER_BGR if bgr else _lib.ORDER_RGB


def unpack_frames(frames: torch.Tensor, encoding: str, *, step=None, width=None, bgr: bool = False, channels=None) -> torch.Tensor:
    """Camera frames -> planar uint8 [B,C,H,W] at full resolution in one launch: the bilinear demosaic of the four 8-bit Bayer
    encodings, the HWC -> planar unpack of rgb8 / bgr8, mono8 (C = 1; ``channels=3`` replicates the plane), "planar" (a copy, or the
    R <-> B exchange).  ``frames``: uint8 on the GPU, [B,H,W] (mono8, bayer_*8), [B,H,W,3] (rgb8, bgr8) or [B,3,H,W] (planar), B
    optional; or, with ``step`` and ``width``, the padded rows of the message, [B,H,step].  C = 3 is R,G,B, or B,G,R with ``bgr``."""
    src, kind, B, H, W, step, stride = _frame_source(frames, encoding, step, width, channels, "unpack_frames")
    C_, order = _out_order(encoding, bgr, channels, "unpack_frames")
    out = torch.empty(B, C_, H, W, dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        check(lib().wvn_unpack_frames(ptr(src), kind, B, H, W, step, stride, ptr(out), order, stream()), "wvn_unpack_frames")
    return out


def debayer(raw: torch.Tensor, pattern: str) -> torch.Tensor:
    """uint8 [B,H,W] (or [H,W]) mosaics -> uint8 [B,3,H,W] RGB: unpack_frames for ``pattern`` "rggb", "bggr", "gbrg", "grbg" (or the
    encoding's full name, "bayer_gbrg8")."""
    enc = pattern if pattern.startswith("bayer_") else f"bayer_{pattern}8"
    if not enc.startswith("bayer_") or enc not in _lib.SRC_KINDS:
        raise _lib.WvnError(f"debayer: pattern {pattern!r} is not one of rggb, bggr, gbrg, grbg")
    return unpack_frames(raw, enc)


# ops.rectify on a mosaic: "fused" demosaics at the taps in the one launch; "two_step" is unpack_frames + a planar rectify.  The fused
# kernel is the faster one at every measured shape (profiles/rectify.md: 1.7 - 1.9x at full resolution, 2.1 - 3.1x at the 448 x 448 crop), so it is
# the default at every output size; "two_step" stays selectable for the comparison.
RECTIFY_MOSAIC_ROUTES = ("fused", "two_step")


def rectify(frames: torch.Tensor, rmap: RectifyMap, encoding: str = "planar", *, step=None, width=None, bgr: bool = False,
            channels=None, route=None) -> torch.Tensor:
    """Camera frames of any kind unpack_frames takes (default: planar [B,3,H,W], what jpeg_decode returns) -> rectified planar uint8
    [B,C,h,w] through ``rmap``: bilinear with 5-bit weights, taps outside the frame are 0.  For a mosaic the demosaic happens at the
    taps of the same launch and no full-resolution RGB frame is written (``route="two_step"`` forces debayer + rectify, the same
    bytes; None is "fused", the faster one at every measured output size: profiles/rectify.md)."""
    if not isinstance(rmap, RectifyMap):
        raise _lib.WvnError(f"rectify: rmap must be a RectifyMap (ops.rectify_map), got {type(rmap).__name__}")
    if route not in (None,) + RECTIFY_MOSAIC_ROUTES:
        raise _lib.WvnError(f"rectify: route={route!r}: None or one of {RECTIFY_MOSAIC_ROUTES}")
    as_given = {"step": step, "width": width}
    src, kind, B, H, W, step, stride = _frame_source(frames, encoding, step, width, channels, "rectify")
    C_, order = _out_order(encoding, bgr, channels, "rectify")
    if (H, W) != rmap.src_size:
        raise _lib.WvnError(f"rectify: the map is for {rmap.src_size[0]} x {rmap.src_size[1]} frames, these are {H} x {W}")
    if rmap.qx.device != src.device:
        raise _lib.WvnError(f"rectify: the map lives on {rmap.qx.device}, the frames on {src.device}")
    h, w = rmap.out_size
    if encoding.startswith("bayer") and route == "two_step":
        return rectify(unpack_frames(src, encoding, **as_given), rmap, "planar", bgr=bgr)
    out = torch.empty(B, C_, h, w, dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        check(lib().wvn_rectify_frames(ptr(src), kind, B, H, W, step, stride, ptr(rmap.qx), ptr(rmap.qy), h, w, ptr(out), order,
                                       stream()), "wvn_rectify_frames")
    return out


def upload_raw_frames(frames, nbytes: int, device, who: str = "upload_raw_frames") -> torch.Tensor:
    """The ``data`` of raw camera messages of one size (bytes, bytearray, a 1-d uint8 CPU tensor, or a list of those) -> uint8
    [B,nbytes] on ``device`` in ONE upload; a message shorter than ``nbytes`` raises."""
    bufs = _jpeg_buffers(frames, who)
    for i, a in enumerate(bufs):
        if a.size < nbytes:
            raise _lib.WvnError(f"{who}: frame {i} holds {a.size} bytes; height * step = {nbytes}")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.WvnError(f"{who}: device must be a GPU (got {device}); the HIP path has no CPU fallback")
    host = torch.empty(len(bufs), nbytes, dtype=torch.uint8)
    view = host.numpy()
    for i, a in enumerate(bufs):
        view[i] = a[:nbytes]
    return host.to(device)


# ------------------------------------------------------------------------------------------------------------- traversability grid map
GRID_DEFAULT_DISCS = ((30, 15), (55, 20), (90, 25))   # smart_carrot.py:74-85: (distance, radius = thickness / 2) in cells of its 200-cell map


def _grid_layer(t: torch.Tensor, name: str, who: str, dtype=torch.float32, N=None) -> int:
    require_cuda(t, name)
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] != t.shape[1] or not t.is_contiguous() or (N is not None and t.shape[0] != N):
        raise _lib.WvnError(f"{who}: {name} must be a contiguous {dtype} [N,N] layer" + (f" with N = {N}" if N is not None else "") +
                            f" (got {t.dtype} {tuple(t.shape)})")
    return t.shape[0]


def grid_fuse_images(maps: torch.Tensor, intrinsics: torch.Tensor, pose_cam_in_world: torch.Tensor, elevation: torch.Tensor, layers,
                     hits: torch.Tensor, center, resolution: float, alpha: float = 0.5, min_depth: float = 0.1, max_range=None,
                     occlusion_margin: float = 0.05) -> None:
    """Paint camera images onto grid layers, in place (include/wvn_hip.h: wvn_grid_fuse_images).  maps [B,C,H,W] fp32 (C <= 4),
    intrinsics and pose_cam_in_world [B,4,4], elevation [N,N] (NaN = unknown), ``layers``: C fp32 [N,N] tensors, hits int32 [N,N];
    ``center`` = (x, y) of the grid.  The cameras are applied in order; one launch, nothing is read back."""
    who = "grid_fuse_images"
    require_cuda(maps, "maps")
    if maps.dtype != torch.float32 or maps.dim() != 4:
        raise _lib.WvnError(f"{who}: maps must be fp32 [B,C,H,W] (got {maps.dtype} {tuple(maps.shape)})")
    B, Cc, H, W = maps.shape
    layers = list(layers)
    if not (1 <= Cc <= _lib.GRID_MAX_CHANNELS) or len(layers) != Cc:
        raise _lib.WvnError(f"{who}: {Cc} channels for {len(layers)} layers; 1 to {_lib.GRID_MAX_CHANNELS} channels, one layer each")
    N = _grid_layer(elevation, "elevation", who)
    for k, t in enumerate(layers):
        _grid_layer(t, f"layers[{k}]", who, N=N)
    _grid_layer(hits, "hits", who, torch.int32, N)
    mats = []
    for name, m in (("intrinsics", intrinsics), ("pose_cam_in_world", pose_cam_in_world)):
        require_cuda(m, name)
        if tuple(m.shape) != (B, 4, 4):
            raise _lib.WvnError(f"{who}: {name} must be [{B},4,4] (got {tuple(m.shape)})")
        mats.append(m.to(torch.float32).contiguous())
    maps = maps.contiguous()
    table = (C.c_void_p * Cc)(*[ptr(t) for t in layers])
    with torch.cuda.device(maps.device):
        check(lib().wvn_grid_fuse_images(ptr(maps), B, Cc, H, W, ptr(mats[0]), ptr(mats[1]), ptr(elevation), N, float(center[0]),
                                         float(center[1]), float(resolution), table, ptr(hits), float(alpha), float(min_depth),
                                         float("inf") if max_range is None else float(max_range), float(occlusion_margin), stream()),
              "wvn_grid_fuse_images")


def grid_sdf(layer: torch.Tensor, threshold: float, resolution: float, unknown: str = "obstacle", out=None):
    """Exact Euclidean signed distance field of {layer < threshold} (include/wvn_hip.h: wvn_grid_sdf) -> (sdf fp32 [N,N] in metres,
    d2 int32 [N,N] in squared cells); positive = free.  ``unknown``: what a NaN cell counts as, "obstacle", "free" or "neither" (NaN out).
    ``out`` = (sdf, d2) to write into existing tensors."""
    who = "grid_sdf"
    N = _grid_layer(layer, "layer", who)
    if unknown not in _lib.GRID_UNKNOWN:
        raise _lib.WvnError(f"{who}: unknown={unknown!r} is not one of {tuple(_lib.GRID_UNKNOWN)}")
    if out is None:
        sdf = torch.empty(N, N, dtype=torch.float32, device=layer.device)
        d2 = torch.empty(N, N, dtype=torch.int32, device=layer.device)
    else:
        sdf, d2 = out
        _grid_layer(sdf, "out[0]", who, N=N)
        _grid_layer(d2, "out[1]", who, torch.int32, N)
    with torch.cuda.device(layer.device):
        check(lib().wvn_grid_sdf(ptr(layer), N, float(threshold), _lib.GRID_UNKNOWN[unknown], float(resolution), ptr(d2), ptr(sdf), stream()),
              "wvn_grid_sdf")
    return sdf, d2


def grid_carrot(sdf: torch.Tensor, elevation: torch.Tensor, yaw: float, center, resolution: float, distance_force_factor: float = 0.0,
                center_force_factor: float = 0.0, discs=GRID_DEFAULT_DISCS, want_masked: bool = False):
    """The goal selection of smart_carrot.py in one launch (include/wvn_hip.h: wvn_grid_carrot) -> (cell int32 [3] = (i, j, found),
    goal fp32 [3] = (score, x, y), masked score layer or None), all on the device.  ``discs``: (distance, radius) pairs in cells."""
    who = "grid_carrot"
    N = _grid_layer(sdf, "sdf", who)
    _grid_layer(elevation, "elevation", who, N=N)
    discs = [(int(d), int(r)) for d, r in discs]
    if not (1 <= len(discs) <= _lib.GRID_MAX_DISCS):
        raise _lib.WvnError(f"{who}: {len(discs)} discs; 1 to {_lib.GRID_MAX_DISCS}")
    table = (C.c_int * (2 * len(discs)))(*[v for d in discs for v in d])
    cell = torch.empty(3, dtype=torch.int32, device=sdf.device)
    goal = torch.empty(3, dtype=torch.float32, device=sdf.device)
    masked = torch.empty(N, N, dtype=torch.float32, device=sdf.device) if want_masked else None
    with torch.cuda.device(sdf.device):
        check(lib().wvn_grid_carrot(ptr(sdf), ptr(elevation), N, math.cos(yaw), math.sin(yaw), float(distance_force_factor),
                                    float(center_force_factor), table, len(discs), float(center[0]), float(center[1]), float(resolution),
                                    ptr(cell), ptr(goal), ptr(masked), stream()), "wvn_grid_carrot")
    return cell, goal, masked


# ---- elevation from depth (include/wvn_hip.h: wvn_grid_elevation_*; csrc/elevation.hip) ----
# anymal_parameters.yaml of the reference's elevation_mapping_cupy configuration; clear_margin and clear_min_rays are this project's own
GRID_ELEVATION_DEFAULTS = dict(sensor_noise_factor=0.05, mahalanobis_thresh=2.0, outlier_variance=0.01, min_valid_distance=0.5,
                               max_height_range=1.0, ramped_height_range_a=0.3, ramped_height_range_b=1.0, ramped_height_range_c=0.2,
                               initial_variance=1000.0, max_variance=100.0, max_ray_length=10.0, clear_margin=0.05, clear_min_rays=1)


def grid_elevation_params(**kw) -> "_lib.GridElevationParams":
    unknown = set(kw) - set(GRID_ELEVATION_DEFAULTS)
    if unknown:
        raise _lib.WvnError(f"grid_elevation: unknown parameters {sorted(unknown)}")
    p = dict(GRID_ELEVATION_DEFAULTS, **kw)
    return _lib.GridElevationParams(p["sensor_noise_factor"], p["mahalanobis_thresh"], p["outlier_variance"], p["min_valid_distance"],
                                    p["max_height_range"], p["ramped_height_range_a"], p["ramped_height_range_b"],
                                    p["ramped_height_range_c"], p["initial_variance"], p["max_variance"], p["max_ray_length"],
                                    p["clear_margin"], int(p["clear_min_rays"]))


def grid_elevation_workspace(N: int, device) -> torch.Tensor:
    """The zeroed integer workspace of an N x N map (the kernels leave it zero: allocate it once per map)."""
    nbytes = lib().wvn_grid_elevation_workspace_bytes(int(N))
    if nbytes == 0:
        raise _lib.WvnError(f"grid_elevation_workspace: {N} cells a side; 1 to {_lib.GRID_MAX_N}")
    return torch.zeros(nbytes // 8, dtype=torch.int64, device=device)


def _grid_elevation(who, launch, poses, elevation, variance, layers, hits, z_ref, clear_rays, params, workspace, B):
    N = _grid_layer(elevation, "elevation", who)
    _grid_layer(variance, "variance", who, N=N)
    _grid_layer(hits, "hits", who, torch.int32, N)
    layers = list(layers)
    if len(layers) > _lib.GRID_MAX_CHANNELS:
        raise _lib.WvnError(f"{who}: {len(layers)} image layers; at most {_lib.GRID_MAX_CHANNELS}")
    for k, t in enumerate(layers):
        _grid_layer(t, f"layers[{k}]", who, N=N)
    require_cuda(poses, "pose_sensor_in_map")
    if tuple(poses.shape) != (B, 4, 4):
        raise _lib.WvnError(f"{who}: pose_sensor_in_map must be [{B},4,4] (got {tuple(poses.shape)})")
    poses = poses.to(torch.float32).contiguous()
    if z_ref is None:
        z_ref = poses[0, 2, 3:4]       # sensor 0's t_z, read by the kernels where it lies
    elif not isinstance(z_ref, torch.Tensor):
        z_ref = torch.full((1,), float(z_ref), dtype=torch.float32, device=elevation.device)
    if not z_ref.is_cuda or z_ref.dtype != torch.float32 or z_ref.numel() != 1:
        raise _lib.WvnError(f"{who}: z_ref must be a number or one fp32 on the GPU")
    if workspace is None:
        workspace = grid_elevation_workspace(N, elevation.device)
    need = lib().wvn_grid_elevation_workspace_bytes(N)
    if not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise _lib.WvnError(f"{who}: the workspace must be a contiguous GPU tensor of at least {need} bytes")
    params = grid_elevation_params() if params is None else params
    flags = _lib.GRID_ELEVATION_CLEAR_RAYS if clear_rays else 0
    stats = torch.empty(len(_lib.GRID_ELEVATION_STATS), dtype=torch.int32, device=elevation.device)
    table = (C.c_void_p * max(len(layers), 1))(*[ptr(t) for t in layers])
    with torch.cuda.device(elevation.device):
        launch(poses, N, C.byref(params), ptr(z_ref), flags, ptr(workspace))
        check(lib().wvn_grid_elevation_finalise(ptr(elevation), ptr(variance), table, len(layers), ptr(hits), N, C.byref(params), ptr(z_ref),
                                                flags, ptr(workspace), ptr(stats), stream()), "wvn_grid_elevation_finalise")
    return stats


def grid_elevation_points(points: torch.Tensor, pose_sensor_in_map: torch.Tensor, elevation: torch.Tensor, variance: torch.Tensor, layers,
                          hits: torch.Tensor, center, resolution: float, counts=None, z_ref=None, clear_rays: bool = False, params=None,
                          workspace=None) -> torch.Tensor:
    """Fuse the point clouds of one callback into the elevation and variance layers, in place (include/wvn_hip.h:
    wvn_grid_elevation_accumulate_points + wvn_grid_elevation_finalise).  points [B,Pmax,3] fp32 in the sensor frames, ``counts`` [B]
    int32 on the GPU (None: every slot is a point), pose_sensor_in_map [B,4,4]; ``layers`` / ``hits``: the image layers and hit counts
    that ray clearing resets.  ``z_ref``: None (sensor 0's t_z, taken on the device), a number, or one fp32 on the GPU.  Two launches,
    nothing is read back -> the class counters, int32 [8] on the GPU in the order of _lib.GRID_ELEVATION_STATS."""
    who = "grid_elevation_points"
    require_cuda(points, "points")
    if points.dtype != torch.float32 or points.dim() != 3 or points.shape[2] != 3:
        raise _lib.WvnError(f"{who}: points must be fp32 [B,Pmax,3] (got {points.dtype} {tuple(points.shape)})")
    B, Pmax, _ = points.shape
    if B * Pmax > _lib.GRID_ELEVATION_MAX_POINTS:
        raise _lib.WvnError(f"{who}: {B * Pmax} point slots; at most {_lib.GRID_ELEVATION_MAX_POINTS} per call (the 64-bit sums' bound)")
    points = points.contiguous()
    if counts is not None:
        require_cuda(counts, "counts")
        if counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
            raise _lib.WvnError(f"{who}: counts must be int32 [{B}] (got {counts.dtype} {tuple(counts.shape)})")
        counts = counts.contiguous()

    def launch(poses, N, p, z, flags, ws):
        check(lib().wvn_grid_elevation_accumulate_points(ptr(points), ptr(counts), B, Pmax, ptr(poses), ptr(elevation), ptr(variance), N,
                                                         float(center[0]), float(center[1]), float(resolution), p, z, flags, ws, stream()),
              "wvn_grid_elevation_accumulate_points")

    return _grid_elevation(who, launch, pose_sensor_in_map, elevation, variance, layers, hits, z_ref, clear_rays, params, workspace, B)


def grid_elevation_depth(depth: torch.Tensor, intrinsics: torch.Tensor, pose_cam_in_world: torch.Tensor, elevation: torch.Tensor,
                         variance: torch.Tensor, layers, hits: torch.Tensor, center, resolution: float, z_ref=None, clear_rays: bool = False,
                         params=None, workspace=None) -> torch.Tensor:
    """The same from depth images [B,H,W], fp32 metres or uint16 millimetres (0, NaN, inf: no point), with the scaled intrinsics
    [B,4,4] as for grid_fuse_images; the points are formed on load (wvn_grid_elevation_accumulate_depth)."""
    who = "grid_elevation_depth"
    require_cuda(depth, "depth")
    if depth.dtype not in (torch.float32, torch.uint16) or depth.dim() != 3:
        raise _lib.WvnError(f"{who}: depth must be fp32 or uint16 [B,H,W] (got {depth.dtype} {tuple(depth.shape)})")
    B, H, W = depth.shape
    if B * H * W > _lib.GRID_ELEVATION_MAX_POINTS:
        raise _lib.WvnError(f"{who}: {B * H * W} pixels; at most {_lib.GRID_ELEVATION_MAX_POINTS} per call (the 64-bit sums' bound)")
    require_cuda(intrinsics, "intrinsics")
    if tuple(intrinsics.shape) != (B, 4, 4):
        raise _lib.WvnError(f"{who}: intrinsics must be [{B},4,4] (got {tuple(intrinsics.shape)})")
    K = intrinsics.to(torch.float32).contiguous()
    depth = depth.contiguous()
    dtype = _lib.GRID_DEPTH_U16 if depth.dtype == torch.uint16 else _lib.GRID_DEPTH_F32

    def launch(poses, N, p, z, flags, ws):
        check(lib().wvn_grid_elevation_accumulate_depth(ptr(depth), dtype, B, H, W, ptr(K), ptr(poses), ptr(elevation), ptr(variance), N,
                                                        float(center[0]), float(center[1]), float(resolution), p, z, flags, ws, stream()),
              "wvn_grid_elevation_accumulate_depth")

    return _grid_elevation(who, launch, pose_cam_in_world, elevation, variance, layers, hits, z_ref, clear_rays, params, workspace, B)
