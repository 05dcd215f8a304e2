"""csrc/random_pixels.hip on the GPU: ops.random_pixels against the plain statement of its definition (tests/random_pixels_ref.py)
bit for bit, ops.gather_bilinear against the dense up-sampled map it indexes (the reference's ``dense.reshape(D, H*H)[:, idx].T``,
feature_extractor.py:96-111), and the sampled maps through the two pooling kernels that consume them downstream."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import random_pixels_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("B,H,W,nr,frame0", [
    (3, 24, 24, 100, 0),
    (2, 32, 32, 1, 7),                   # 32 * 32 = 4^5: no cycle walking
    (1, 33, 33, 1089, 12345),            # the whole frame
    (2, 5, 7, 35, 2 ** 32 - 1),          # the frame index wraps between the two images
    (2, 224, 224, 100, 64),
])
@pytest.mark.parametrize("seed", [0, 3])
def test_random_pixels_equals_the_statement(dev, B, H, W, nr, frame0, seed):
    idx, seg = ops.random_pixels(B, H, W, nr, seed=seed, frame0=frame0, device=dev)
    assert idx.shape == (B, nr) and idx.dtype == torch.int32 and seg.shape == (B, H, W) and seg.dtype == torch.int32
    idx0, seg0 = REF.random_pixels(B, H, W, nr, seed=seed, frame0=frame0)
    assert torch.equal(idx.cpu(), torch.from_numpy(idx0))
    assert torch.equal(seg.cpu(), torch.from_numpy(seg0))


def _hand_made_idx(H, extra_seed):
    """The four corners, one duplicate, and a few interior pixels; two images with different orders."""
    corners = [0, H - 1, H * H - H, H * H - 1]
    inner = torch.randint(0, H * H, (5,), generator=g(extra_seed)).tolist()
    a = corners + inner + [inner[0]]
    b = [inner[1]] + corners[::-1] + inner + [H * H - 1]
    return torch.tensor([a, b[:len(a)]], dtype=torch.int32)


@pytest.mark.parametrize("G,H,D", [(7, 24, 90), (8, 64, 384), (2, 33, 5)])
def test_gather_equals_indexing_the_dense_map(dev, G, H, D):
    tokens = torch.randn(2, G * G, D, generator=g(G + H + D)).to(dev)
    idx = _hand_made_idx(H, H).to(dev)
    for v in (0, H - 1, H * H - H, H * H - 1):
        assert (idx[0] == v).any()
    assert idx[0].unique().numel() < idx.shape[1]
    feat = ops.gather_bilinear(tokens, idx, G, H)
    dense = ops.upsample_bilinear(tokens, G, H).reshape(2, D, H * H)
    want = torch.stack([dense[b][:, idx[b].long()].T for b in range(2)])
    assert feat.shape == (2, idx.shape[1], D)
    assert torch.equal(feat, want)
    # int64 indices (what torch indexing produces) are accepted as they are
    assert torch.equal(ops.gather_bilinear(tokens, idx.long(), G, H), want)


def test_gather_gives_nan_rows_for_indices_off_the_map(dev):
    tokens = torch.randn(1, 4, 5, generator=g(1)).to(dev)
    idx = torch.tensor([[-1, 0, 81, 80]], dtype=torch.int32, device=dev)
    feat = ops.gather_bilinear(tokens, idx, 2, 9)
    assert torch.isnan(feat[0, 0]).all() and torch.isnan(feat[0, 2]).all()
    assert torch.isfinite(feat[0, 1]).all() and torch.isfinite(feat[0, 3]).all()


@pytest.mark.parametrize("G,H,D,nr", [(7, 24, 90, 100), (8, 64, 384, 37)])
def test_segpool_on_a_sampled_map_agrees_with_the_gather(dev, G, H, D, nr):
    """A one-pixel segment's mean is the interpolated feature at that pixel.  The pooling kernel rounds the four tap weights to 2^-40
    fixed point and sums four products in fp32 (three roundings): below 2.5e-7 of the largest tap; the bound is 1e-6 of it."""
    tokens = torch.randn(2, G * G, D, generator=g(nr)).to(dev)
    idx, seg = ops.random_pixels(2, H, H, nr, seed=1, frame0=5, device=dev)
    got = ops.segpool_bilinear_mean(seg, tokens, G, nr)
    want = ops.gather_bilinear(tokens, idx, G, H)
    err = (got - want).abs().max().item()
    print(f"segpool vs gather: max abs difference {err:.3e}, bound {1e-6 * tokens.abs().max().item():.3e}")
    assert err <= 1e-6 * tokens.abs().max().item()


def test_label_pool_on_a_sampled_map(dev):
    """MissionNode.update_supervision_signal on a random-pixel map: per sample the nanmean over channels of the mask at its pixel (0 where
    every channel is NaN), valid = signal > 0.  1e-6: the kernel's 2^-32 fixed-point step plus fp32 rounding of values in [0, 1]."""
    H, W, nr, C = 24, 40, 100, 3
    mask = torch.rand(C, H, W, generator=g(0))
    mask[torch.rand(C, H, W, generator=g(1)) < 0.5] = float("nan")
    idx, seg = ops.random_pixels(2, H, W, nr, seed=2, frame0=9, device=dev)
    for b in range(2):
        signal, valid = ops.label_pool(mask.to(dev), seg[b], nr)
        px = mask.reshape(C, H * W)[:, idx[b].cpu().long()]          # [C, nr]
        want = torch.nan_to_num(torch.nanmean(px.double(), dim=0), nan=0.0)
        assert torch.isnan(px).all(0).any() and (~torch.isnan(px)).all(0).any()      # the fixture has both kinds of pixel
        assert (signal.cpu().double() - want).abs().max().item() <= 1e-6
        assert torch.equal(valid.cpu(), want > 0)


def test_refusals(dev):
    with pytest.raises(_lib.WvnError):
        ops.random_pixels(1, 8, 8, 65, device=dev)               # nr > H*W
    with pytest.raises(_lib.WvnError):
        ops.random_pixels(1, 8, 8, 0, device=dev)
    with pytest.raises(_lib.WvnError):
        ops.random_pixels(1, 8, 8, 4, device="cpu")
    tokens = torch.randn(1, 16, 8, generator=g(0))
    idx = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(_lib.WvnError):
        ops.gather_bilinear(tokens, idx.to(dev), 4, 16)          # CPU tokens
    with pytest.raises(_lib.WvnError):
        ops.gather_bilinear(tokens.to(dev), idx, 4, 16)          # CPU indices
    with pytest.raises(_lib.WvnError):
        ops.gather_bilinear(tokens.to(dev), idx.to(dev), 5, 16)  # 16 tokens are not a 5 x 5 grid
    with pytest.raises(_lib.WvnError):
        ops.gather_bilinear(tokens.to(dev), idx.to(dev).expand(2, 3), 4, 16)   # batch of idx != batch of tokens
    with pytest.raises(_lib.WvnError):
        ops.gather_bilinear(tokens.to(dev), idx.to(dev), 4, 0)
