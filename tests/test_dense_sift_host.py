"""The dense-SIFT definition without a GPU: the float64 statement (tests/dense_sift_ref.py, 8 + 1 convolutions) against an independent
direct-sum evaluation (plain loops over the 7 x 7 gradient pixels one descriptor depends on), and the properties the definition
implies: output shape, unit L1 norm of the squared descriptor, the flat image, the column order a * 16 + i * 4 + j."""
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_sift_ref as REF  # noqa: E402

K = (0.25, 0.75, 0.75, 0.25)
EPS = 1e-10


def direct_descriptor(I, y, x):
    """Steps 1-5 for pixel (y, x) of the image I (list of rows of Python floats): 128 values, no convolution, no padding buffers."""
    H, W = len(I), len(I[0])
    raw = [0.0] * 128
    for yy in range(y - 3, y + 4):
        for xx in range(x - 3, x + 4):
            if not (0 <= yy < H and 0 <= xx < W):
                continue                                   # zero padding of the planes
            gx = (I[yy][min(xx + 1, W - 1)] - I[yy][max(xx - 1, 0)]) / 2
            gy = (I[min(yy + 1, H - 1)][xx] - I[max(yy - 1, 0)][xx]) / 2
            mag = math.sqrt(gx * gx + gy * gy + EPS)
            o = 8.0 * (math.atan2(gy, gx + EPS) + 2.0 * math.pi) / (2.0 * math.pi)
            fl = math.floor(o)
            w1 = o - fl
            b0 = int(fl) % 8
            b1 = (b0 + 1) % 8
            for i in range(4):
                p = y - 1 + i                              # row of Q this spatial bin reads
                if not 0 <= p <= H:
                    continue                               # zero padding of Q
                ki = yy - (p - 2)
                if not 0 <= ki < 4:
                    continue
                for j in range(4):
                    q = x - 1 + j
                    if not 0 <= q <= W:
                        continue
                    kj = xx - (q - 2)
                    if not 0 <= kj < 4:
                        continue
                    w = K[ki] * K[kj]
                    raw[b0 * 16 + i * 4 + j] += w * (1.0 - w1) * mag
                    raw[b1 * 16 + i * 4 + j] += w * w1 * mag
    n = max(math.sqrt(sum(v * v for v in raw)), 1e-12)
    d = [min(max(v / n, 0.0), 0.2) for v in raw]
    n = max(math.sqrt(sum(v * v for v in d)), 1e-12)
    d = [v / n for v in d]
    n = max(sum(abs(v) for v in d), 1e-12)
    return [math.sqrt(v / n + EPS) for v in d]


def test_statement_equals_the_direct_sum():
    H, W = 13, 11
    img = torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    got = REF.dense_sift(img)[0]
    rows = img[0, 0].tolist()
    pixels = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),                       # corners
              (0, 5), (H - 1, 4), (6, 0), (7, W - 1), (1, 1), (H - 2, W - 2), (2, 8), (10, 2)]   # edges and next to them
    gen = torch.Generator().manual_seed(1)
    while len(pixels) < 40:
        p = (int(torch.randint(0, H, (1,), generator=gen)), int(torch.randint(0, W, (1,), generator=gen)))
        if p not in pixels:
            pixels.append(p)
    assert sum(3 <= y < H - 4 and 3 <= x < W - 4 for y, x in pixels) >= 5          # interior ones too
    worst = 0.0
    for y, x in pixels:
        want = torch.tensor(direct_descriptor(rows, y, x), dtype=torch.float64)
        worst = max(worst, (got[:, y, x] - want).abs().max().item())
    print(f"statement vs direct sum over {len(pixels)} pixels: max abs difference {worst:.3e}")
    assert worst <= 1e-12


def test_shape_and_channel_blocks():
    img = torch.rand(2, 3, 9, 14, generator=torch.Generator().manual_seed(2))
    d = REF.dense_sift(img)
    assert d.shape == (2, 384, 9, 14) and d.dtype == torch.float64
    for c in range(3):   # channel c of the frame fills columns [128 c, 128 c + 128)
        # (1e-14, not equality: the convolution library may sum a batch of 6 planes in another order than a batch of 2)
        assert (d[:, 128 * c:128 * (c + 1)] - REF.dense_sift(img[:, c:c + 1])).abs().max().item() <= 1e-14
    assert REF.dense_sift(img[:, :1]).shape == (2, 128, 9, 14)
    assert REF.dense_sift(img[:, :1], dtype=torch.float32).dtype == torch.float32
    u8 = torch.randint(0, 256, (1, 1, 6, 7), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    assert torch.equal(REF.dense_sift(u8), REF.dense_sift(u8.float() / 255))


def test_squared_descriptor_sums_to_one_plus_128_eps():
    img = torch.rand(1, 1, 12, 10, generator=torch.Generator().manual_seed(4))
    d = REF.dense_sift(img)
    assert (d.pow(2).sum(1) - (1 + 128 * EPS)).abs().max().item() <= 1e-12
    assert (REF.dense_sift(img, squared=True).sum(1) - 1).abs().max().item() <= 1e-12


def test_flat_image_gives_one_constant_descriptor():
    """No gradient: mag = sqrt(eps) in plane 0 everywhere.  Every pixel whose 7 x 7 support lies inside the image (and whose Q window
    does) has the same descriptor, whatever the grey level: 16 equal values in plane 0, sqrt(eps) elsewhere."""
    a = REF.dense_sift(torch.full((1, 1, 12, 15), 0.3, dtype=torch.float64))[0]
    b = REF.dense_sift(torch.full((1, 1, 12, 15), 0.8, dtype=torch.float64))[0]
    assert torch.equal(a, b)
    inner = a[:, 3:-3, 3:-3].reshape(128, -1)
    assert (inner - inner[:, :1]).abs().max().item() <= 1e-15
    want = torch.full((128,), math.sqrt(EPS), dtype=torch.float64)
    want[:16] = math.sqrt(1.0 / 16 + EPS)
    assert (inner[:, 0] - want).abs().max().item() <= 1e-12
    # at the border the zero paddings empty some spatial bins: the corner pixel keeps the 3 x 3 bins that reach into the image
    assert (a[:16, 0, 0].reshape(4, 4)[0] - math.sqrt(EPS)).abs().max().item() <= 1e-12
    assert (a[:16, 0, 0].reshape(4, 4)[1:, 1:] > 0.1).all()


def test_column_order_on_a_single_edge():
    """One vertical edge (bright left, dark right): gx = -1/2 on the two columns beside it, gy = 0, so ori = pi + 2 pi, o = 12, bin 4.
    For a pixel three columns left of the edge only the last spatial column (j = 3) sees it, three columns right only j = 0; the same
    image transposed (gy = -1/2: ori = 3 pi / 2, bin 6) moves the energy to the spatial ROWS i."""
    H, W, c = 16, 16, 8
    img = torch.zeros(1, 1, H, W, dtype=torch.float64)
    img[..., :c] = 1.0
    d = REF.dense_sift(img, squared=True)[0]
    y = 8
    left = d[:, y, c - 3].reshape(8, 4, 4)      # gradient columns c - 1, c = x + 2, x + 3
    right = d[:, y, c + 2].reshape(8, 4, 4)     # gradient columns x - 3, x - 2
    for v, j in ((left, 3), (right, 0)):
        # (weights 1 in column j and 1/4 in the column beside it: 0.2 / (4 * 0.2 + 4 * 0.25 / sqrt(4.25)) = 0.156 after the clamp)
        assert v[4, :, j].min().item() > 0.15 and (v[4, :, j] - v[4, 0, j]).abs().max().item() <= 1e-12
        assert v.max().item() == v[4, 0, j].item()
        rest = v.clone()
        rest[4] = 0
        assert rest.max().item() < 1e-3          # (plane 0 holds the flat pixels' sqrt(eps) magnitudes)
    assert left[4, :, :2].max().item() == 0 and right[4, :, 2:].max().item() == 0
    dt = REF.dense_sift(img.transpose(2, 3).contiguous(), squared=True)[0]
    up = dt[:, c - 3, y].reshape(8, 4, 4)
    plane = up[5] + up[6]                        # o = 6 up to rounding: the weight sits in bin 6, or in bin 5 with w1 = 1 - 1e-16
    assert plane[3, :].min().item() > 0.15 and plane[:2, :].max().item() == 0
    assert up[6][3, :].min().item() > 0.15


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from wild_visual_navigation_amd import _lib

    h = _lib.lib()
    p = 1 << 20   # (never dereferenced: every call below is refused first)
    assert h.wvn_dense_sift(None, 0, p, 1, 3, 8, 8, None) == 1001
    assert h.wvn_dense_sift(p, 0, p, 1, 2, 8, 8, None) == 1001                 # C = 2
    assert h.wvn_dense_sift(p, 0, p, 1, 3, 3, 8, None) == 1001                 # H = 3
    assert h.wvn_dense_sift(p, 1, p, 1, 3, 8, 3, None) == 1001
    assert h.wvn_dense_sift(p, 0, p, 0, 3, 8, 8, None) == 1001
    assert h.wvn_dense_sift(p, 0, p, 21846, 3, 8, 8, None) == 1001             # B * C > 65535
    assert h.wvn_dense_sift(p, 0, p, 1, 1, 16385, 8, None) == 1001
    assert h.wvn_dense_sift_segpool(p, 0, p, p, p, p, 1, 3, 8, 8, 0, None) == 1001      # S = 0
    assert h.wvn_dense_sift_segpool(p, 0, None, p, p, p, 1, 3, 8, 8, 4, None) == 1001
    assert h.wvn_dense_sift_segpool(p, 0, p, p, p, None, 1, 3, 8, 8, 4, None) == 1001
    assert h.wvn_dense_sift_segpool(p, 0, p, p, p, p, 1, 2, 8, 8, 4, None) == 1001
    assert h.wvn_dense_sift_segpool(p, 0, p, p, p, p, 16, 3, 8, 8, 1 << 20, None) == 1001   # B * S * 384 >= 2^31
    assert C.sizeof(C.c_longlong) == 8


def test_ops_refuse_cpu_tensors():
    import pytest

    from wild_visual_navigation_amd import _lib, ops

    img = torch.rand(1, 3, 8, 8)
    with pytest.raises(_lib.WvnError):
        ops.dense_sift(img)
    with pytest.raises(_lib.WvnError):
        ops.dense_sift_segpool(img, torch.zeros(1, 8, 8, dtype=torch.int32), 1)
