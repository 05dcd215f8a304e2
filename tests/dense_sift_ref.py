"""The dense-SIFT definition csrc/dense_sift.hip is held to (include/wvn_hip.h), as torch operations in a chosen dtype: float64 is the
statement, float32 the same text as the yardstick of what fp32 arithmetic makes of it.  It is the published algorithm (Lowe's
descriptor evaluated at every pixel: soft-binned gradient orientations, a triangular 4 x 4 pooling window, 4 x 4 spatial bins, the
L2 / clamp 0.2 / L2 normalisation, RootSIFT), written from that description as 8 + 1 convolutions per channel; the kornia package
whose DenseSIFTDescriptor the reference calls is absent, so parity with the package itself is unpinned.

    dense_sift(img [B,C,H,W]) -> [B, 128 C, H, W];  pieces: gradient_planes, pooled, descriptor_raw, normalise.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-10
A = 8            # angular bins
NS = 4           # spatial bins per axis
K1 = (0.25, 0.75, 0.75, 0.25)


def gradient_planes(ch: torch.Tensor) -> torch.Tensor:
    """Steps 1 and 2: ch [N,1,H,W] -> the A soft-binned magnitude planes [N,A,H,W]."""
    p = F.pad(ch, (1, 1, 1, 1), mode="replicate")
    gx = (p[:, :, 1:-1, 2:] - p[:, :, 1:-1, :-2]) / 2
    gy = (p[:, :, 2:, 1:-1] - p[:, :, :-2, 1:-1]) / 2
    mag = torch.sqrt(gx * gx + gy * gy + EPS)
    ori = torch.atan2(gy, gx + EPS) + 2.0 * math.pi
    o = float(A) * ori / (2.0 * math.pi)
    fl = torch.floor(o)
    w1 = o - fl
    b0 = fl % A
    b1 = (b0 + 1) % A
    v0 = (1.0 - w1) * mag
    v1 = w1 * mag
    return torch.cat([(b0 == a).to(ch.dtype) * v0 + (b1 == a).to(ch.dtype) * v1 for a in range(A)], dim=1)


def pooled(planes: torch.Tensor) -> torch.Tensor:
    """Step 3: [N,A,H,W] -> Q [N,A,H+1,W+1], the k (x) k cross-correlation with zero padding 2, one convolution per plane."""
    k = torch.tensor(K1, dtype=planes.dtype, device=planes.device)
    kk = (k[:, None] * k[None, :])[None, None]
    return torch.cat([F.conv2d(planes[:, a:a + 1], kk, padding=2) for a in range(A)], dim=1)


def descriptor_raw(q: torch.Tensor) -> torch.Tensor:
    """Step 4: Q [N,A,H+1,W+1] -> [N,128,H,W]: the identity "reshape" convolution, zero padding 1; column a * 16 + i * 4 + j."""
    eye = torch.eye(NS * NS, dtype=q.dtype, device=q.device).reshape(NS * NS, 1, NS, NS)
    n, a, h1, w1 = q.shape
    out = F.conv2d(q.reshape(n * a, 1, h1, w1), eye, padding=1)          # [N*A, 16, H, W]
    return out.reshape(n, a * NS * NS, h1 - 1, w1 - 1)


def normalise_l1(d: torch.Tensor) -> torch.Tensor:
    """Step 5 up to the L1-normalised vector (the square of the final descriptor minus eps)."""
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    d = d.clamp(0.0, 0.2)
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return d / d.abs().sum(dim=1, keepdim=True).clamp_min(1e-12)


def normalise(d: torch.Tensor) -> torch.Tensor:
    return torch.sqrt(normalise_l1(d) + EPS)


def dense_sift(img: torch.Tensor, dtype=torch.float64, squared: bool = False) -> torch.Tensor:
    """img [B,C,H,W] (uint8 means x / 255 in fp32 first, like the kernel) -> [B, 128 C, H, W] in ``dtype``; channel c of the frame
    fills columns [128 c, 128 c + 128).  ``squared``: stop before sqrt(. + eps)."""
    if img.dtype == torch.uint8:
        img = img.float() / 255
    B, C, H, W = img.shape
    ch = img.to(dtype).reshape(B * C, 1, H, W)
    raw = descriptor_raw(pooled(gradient_planes(ch)))
    d = normalise_l1(raw) if squared else normalise(raw)
    return d.reshape(B, C * A * NS * NS, H, W)
