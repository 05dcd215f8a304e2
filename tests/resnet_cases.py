"""Inputs and case tables for the ResNet-18 pyramid kernels (csrc/resnet.hip, csrc/pyramid_pool.hip) away from the square frames of
tests/test_gpu_resnet.py, shared by tests/test_resnet_cases_host.py (CPU: every case reaches the path it is there for, asserted from
the statement tests/resnet_ref.py and the launch arithmetic alone) and tests/test_gpu_resnet_shapes.py (GPU).  Helper only: no tests.

Every input is built from the case and a seed, computed once (lru_cache) and never modified.  H != W everywhere a kernel takes both:
an H / W or OH / OW exchange in an index expression changes an address that stays inside the buffer but names another element.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import resnet_ref as REF

U = 2.0 ** -24
BM, BN, BK = 64, 64, 32          # the convolution's tile (csrc/resnet.hip): 64 output pixels x 64 channels, K in chunks of 32

ConvCase = namedtuple("ConvCase", "name B H W cin cout k stride pad")


def g(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------- convolution
NHWC_CASES = [
    ConvCase("3x3s1_5x11", 2, 5, 11, 64, 128, 3, 1, 1),
    ConvCase("3x3s1_11x5", 2, 11, 5, 64, 128, 3, 1, 1),
    ConvCase("3x3s2_7x12", 2, 7, 12, 64, 128, 3, 2, 1),          # OH = 4, OW = 6
    ConvCase("1x1s2_9x6", 2, 9, 6, 64, 128, 1, 2, 0),
    ConvCase("cin32_6x10", 2, 6, 10, 32, 64, 3, 1, 1),           # one chunk per tap, grid.y = 1
    ConvCase("cin96_6x10", 2, 6, 10, 96, 192, 3, 1, 1),          # three chunks per tap (Cin no power of two), grid.y = 3
    ConvCase("k5p2_6x9", 2, 6, 9, 32, 64, 5, 1, 2),
    ConvCase("k7p3s2_9x14", 2, 9, 14, 32, 64, 7, 2, 3),          # K = 1568
    ConvCase("k2p0s2_7x10", 2, 7, 10, 32, 64, 2, 2, 0),          # the last input row is read by no window
    ConvCase("k3p0_5x8", 2, 5, 8, 32, 64, 3, 1, 0),
    ConvCase("k3p3_4x6", 2, 4, 6, 32, 64, 3, 1, 3),              # pad > k / 2: output 8 x 10, corner windows wholly in the padding
    ConvCase("k1p1_4x7", 2, 4, 7, 32, 64, 1, 1, 1),              # the whole output border is padding
    ConvCase("one_pixel_b1", 1, 3, 3, 32, 64, 3, 1, 0),          # M = 1
    ConvCase("one_pixel_b2", 2, 3, 3, 32, 64, 3, 1, 0),          # M = 2: one output pixel per frame
    ConvCase("one_row_1x7", 2, 1, 7, 32, 64, 3, 1, 1),
    ConvCase("m64_8x8", 1, 8, 8, 32, 64, 3, 1, 1),               # M = 64: one full tile, no tail
    ConvCase("m256_8x16", 2, 8, 16, 32, 64, 3, 1, 1),            # M = 256: four full tiles
    ConvCase("m65_5x13", 1, 5, 13, 32, 64, 3, 1, 1),             # M = 65: a tile with one row
]
FRAME_CASES = [
    ConvCase("stem7x7_10x15", 2, 10, 15, 3, 64, 7, 2, 3),
    ConvCase("stem7x7_15x10", 2, 15, 10, 3, 64, 7, 2, 3),
    ConvCase("stem3x3_6x9", 2, 6, 9, 3, 64, 3, 1, 1),            # K = 27: Kpad is one chunk, the prefetch branch is never taken
    ConvCase("stem1x1_5x7", 2, 5, 7, 3, 64, 1, 1, 0),            # K = 3
]
CONV_BY_NAME = {c.name: c for c in NHWC_CASES + FRAME_CASES}
# (Cin, Cout, k, stride, pad, frame): each refused before a launch
CONV_REFUSALS = {"cin48": (48, 64, 3, 1, 1, False), "cout96": (64, 96, 3, 1, 1, False), "k8": (32, 64, 8, 1, 3, False),
                 "stride3": (32, 64, 3, 3, 1, False), "pad4": (32, 64, 3, 1, 4, False), "frame_cin4": (4, 64, 7, 2, 3, True)}


def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def geometry(c):
    """The launch arithmetic of conv_launch: K, Kpad, chunks per tap (NHWC), M, grid."""
    OH, OW = out_hw(c)
    K = c.cin * c.k * c.k
    M = c.B * OH * OW
    return dict(OH=OH, OW=OW, K=K, Kpad=(K + BK - 1) // BK * BK, chunks_per_tap=c.cin // BK, M=M, grid=((M + BM - 1) // BM, c.cout // BN))


def _seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) * 8


def _bn(cout, seed):
    return (0.5 + torch.rand(cout, generator=g(seed + 2)), torch.randn(cout, generator=g(seed + 3)),
            torch.randn(cout, generator=g(seed + 4)), 0.5 + torch.rand(cout, generator=g(seed + 5)))


def conv_bound(xin, w, scale, shift, resid, stride, pad, stem):
    """The forward error bound of tests/test_gpu_resnet.py, elementwise: (K + 10) u (|scale| conv(|x| + c, |w|) + |shift| + |residual|),
    c = mean / std for the stem and 0 otherwise.  xin: the float64 input of the convolution (the normalised frame for the stem)."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    c =(torch.tensor(REF.MEAN) / torch.tensor(REF.STD)).double().view(1, 3, 1, 1) if stem else 0.0
    mag = F.conv2d(xin.abs() + c, w.double().abs(), stride=stride, padding=pad) * scale.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    return (K + 10) * U * (mag + (resid.double().abs() if resid is not None else 0.0))


@functools.lru_cache(maxsize=None)
def conv_float_case(name, u8=False):
    """(x NCHW, w, bn, resid NCHW, want {(residual, relu): float64 NCHW}, bound {residual: float64 NCHW}) of one configuration with
    random fp32 inputs (a frame: uniform in [0, 1], or uint8 with ``u8``) and a BatchNorm whose four terms all vary."""
    c = CONV_BY_NAME[name]
    stem = c.cin == 3
    seed = _seed(c)
    OH, OW = out_hw(c)
    if stem:
        x = torch.randint(0, 256, (c.B, 3, c.H, c.W), generator=g(seed), dtype=torch.uint8) if u8 else torch.rand(c.B, 3, c.H, c.W, generator=g(seed))
    else:
        x = torch.randn(c.B, c.cin, c.H, c.W, generator=g(seed))
    K = c.cin * c.k * c.k
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g(seed + 1)) * (2.0 / K) ** 0.5
    bn = _bn(c.cout, seed)
    resid = torch.randn(c.B, c.cout, OH, OW, generator=g(seed + 6))
    xin = REF.normalize(x) if stem else x.double()
    want = {(r, a): REF.conv_bn_act(xin, w, bn, c.stride, c.pad, resid if r else None, a) for r in (False, True) for a in (False, True)}
    scale, shift = REF.bn_scale_shift(*bn)
    bound = {r: conv_bound(xin, w, scale, shift, resid if r else None, c.stride, c.pad, stem) for r in (False, True)}
    return x, w, bn, resid, want, bound


EXACT_SCALES = (0.5, 1.0, 2.0, -1.0)
EXACT_X, EXACT_SHIFT, EXACT_RESID = 4, 8, 16     # |x| <= 4, |shift| <= 8, |residual| <= 16, all integers


@functools.lru_cache(maxsize=None)
def conv_exact_case(name):
    """The exact twin of an NHWC configuration: integer inputs and residuals, weights in {-1, 0, 1}, scale in {0.5, 1, 2, -1} per channel,
    integer shift.  Every partial sum is an integer below K max|x| max|w| < 2^24 and the epilogue yields integers and halves, so the
    fp32 chain rounds nowhere and the result equals the float64 statement, whatever the order of the additions.
    -> (x NCHW, w, scale, shift, resid NCHW, want {(residual, relu): float64 NCHW})"""
    c = CONV_BY_NAME[name]
    assert c.cin != 3, "the stem's normalisation is not exact"
    seed = _seed(c) + 1000
    OH, OW = out_hw(c)
    x = torch.randint(-EXACT_X, EXACT_X + 1, (c.B, c.cin, c.H, c.W), generator=g(seed)).float()
    w = torch.randint(-1, 2, (c.cout, c.cin, c.k, c.k), generator=g(seed + 1)).float()
    scale = torch.tensor(EXACT_SCALES)[torch.randint(0, 4, (c.cout,), generator=g(seed + 2))]
    shift = torch.randint(-EXACT_SHIFT, EXACT_SHIFT + 1, (c.cout,), generator=g(seed + 3)).float()
    resid = torch.randint(-EXACT_RESID, EXACT_RESID + 1, (c.B, c.cout, OH, OW), generator=g(seed + 4)).float()
    want = {(r, a): REF.conv_affine_act(x, w, scale, shift, c.stride, c.pad, resid if r else None, a) for r in (False, True) for a in (False, True)}
    return x, w, scale, shift, resid, want


# ---------------------------------------------------------------------------------------------------- max-pool
MAXPOOL_SHAPES = [(9, 16, 64), (16, 9, 5), (1, 7, 3), (7, 1, 64), (2, 2, 130)]      # (H, W, C), B = 2


@functools.lru_cache(maxsize=None)
def maxpool_case(H, W, C):
    """All-negative NCHW input (a zero padding would win every border window) and F.max_pool2d(3, 2, 1) of it."""
    x = -0.5 - torch.rand(2, C, H, W, generator=g(H * 1000 + W * 10 + C))
    return x, F.max_pool2d(x, kernel_size=3, stride=2, padding=1)


# ---------------------------------------------------------------------------------------------------- whole network
NET_FRAMES = [(2, 64, 96), (2, 96, 64), (2, 32, 128), (1, 128, 32)]                 # (B, H, W); level 4 of the last two: 1 x 4, 4 x 1


def rel_err(got, want):
    return ((got.double() - want).abs().max() / want.abs().max()).item()


@functools.lru_cache(maxsize=None)
def net_state_dict():
    from wild_visual_navigation_amd.feature_extractor import torchvision_interface as TVI

    return TVI.synthetic_resnet18_state_dict(0)


@functools.lru_cache(maxsize=None)
def net_case(B, H, W):
    """(frames fp32 [B,3,H,W], the float64 maps, per level the fp32 CPU run's distance from float64: the yardstick)."""
    img = torch.rand(B, 3, H, W, generator=g(H * 7 + W))
    f64 = REF.resnet18(net_state_dict(), img)
    f32 = REF.resnet18(net_state_dict(), img, dtype=torch.float32)
    return img, f64, {k: rel_err(f32[k], f64[k]) for k in f64}


# ---------------------------------------------------------------------------------------------------- pooling
POOL_H, POOL_W, POOL_S = 256, 288, 12
L_ID, STRIPE_ID, BLOCK_ID, ABSENT_ID = 3, 1, 2, 11


def _pool_map_a():
    """256 x 288, ids 0..11 (11 without a pixel):
    0  the background: 66 of the 72 stride-32 samples, so its cell loop takes a second trip at every level;
    1  two diagonal stripes sixteen pixels long at the two ends of a 100 x 100 bounding box (625 level-1 cells): the 64-cell rounds
       between them hold no match;
    2  a 30 x 30 block between the stride-32 samples: the centroid cell at level 4, means at levels 1 to 3;
    3  an L of two three-pixel bars that lie between the stride-4 samples: the centroid cell at every level, and that cell is in the
       hollow of the L;
    4, 5  single pixels in the last and the first column of a 16-pixel run of the statistics pass (5 on the stride-4 lattice);
    6, 7  single pixels in the last row and in the last column;
    8  a block in the top right corner that holds four stride-32 samples;
    9, 10  three-pixel specks;
    a patch of -1 and a patch of 99 (>= S), both away from the stride-32 samples."""
    seg = torch.zeros(POOL_H, POOL_W, dtype=torch.int64)
    for t in range(16):
        seg[64 + t, 64 + t] = STRIPE_ID
        seg[148 + t, 148 + t] = STRIPE_ID
    seg[97:127, 193:223] = BLOCK_ID
    seg[176:232, 9:12] = L_ID          # the vertical bar: rows 176..231, columns 9..11
    seg[229:232, 12:86] = L_ID         # the horizontal bar: rows 229..231, columns 12..85; centroid (218.6, 31.9) -> floor (218, 31)
    seg[50, 47] = 4
    seg[52, 48] = 5
    seg[255, 101] = 6
    seg[77, 287] = 7
    seg[0:41, 220:288] = 8
    seg[9, 130:133] = 9
    seg[170:173, 250] = 10
    seg[200:216, 130:151] = -1
    seg[232:251, 200:221] = 99
    return seg


def _pool_map_b():
    """The other frame of the batch: six 40 x 40 blocks that hold a sample of every level (ids 6..11), five 3 x 3 blocks between the
    stride-4 samples (ids 1..5), background 0, a column of -1 and a row of 99."""
    seg = torch.zeros(POOL_H, POOL_W, dtype=torch.int64)
    for k in range(6, 12):
        y, x = 20 + (k - 6) // 3 * 120, 30 + (k - 6) % 3 * 90
        seg[y: y + 40, x: x + 40] = k
    for k in range(1, 6):
        y, x = 4 * (3 + 11 * k) + 1, 4 * (60 - 9 * k) + 1
        seg[y: y + 3, x: x + 3] = k
    seg[:, 283] = -1
    seg[250, :] = 99
    return seg


def _pool_map_tall():
    """96 x 32 (level 4 is 3 x 1), ids 0..4 as bands of 20 rows, shifted by two ids right of column 20; a few -1."""
    seg = (torch.arange(96)[:, None] // 20).expand(96, 32).clone()
    seg[:, 20:] = (seg[:, 20:] + 2) % 5
    seg[5:90:7, 3] = -1
    return seg


POOL_FRAMES = {   # name -> (builder of segs [B,H,W] int64, S, seg dtype handed to the kernel)
    "wide": (lambda: torch.stack([_pool_map_a(), _pool_map_b()]), POOL_S, torch.int32),
    "tall": (lambda: _pool_map_tall()[None], 5, torch.int64),
    "one_id": (lambda: torch.zeros(1, 32, 32, dtype=torch.int64), 1, torch.int32),
    "one_id_s3000": (lambda: torch.zeros(1, 32, 32, dtype=torch.int64), 3000, torch.int32),
}


def integer_levels(B, H, W, seed):
    """Integer-valued fp32 NCHW level maps: float64 sums of them are exact in any order."""
    return [torch.randint(-8, 9, (B, c, H // s, W // s), generator=g(seed + s)).float() for c, s in zip(REF.CHANNELS, REF.STRIDES)]


def randn_levels(B, H, W, seed):
    return [torch.randn(B, c, H // s, W // s, generator=g(seed + s)) for c, s in zip(REF.CHANNELS, REF.STRIDES)]


@functools.lru_cache(maxsize=None)
def pool_case(name, kind="int"):
    """(segs int64 [B,H,W], S, seg dtype, NCHW level maps, want float64 [B,S,960], fallback bool [B,S,4]) of a frame."""
    build, S, dtype = POOL_FRAMES[name]
    segs = build()
    B, H, W = segs.shape
    levels = (integer_levels if kind == "int" else randn_levels)(B, H, W, H * 3 + W)   # (one_id and one_id_s3000: the same maps)
    out = [REF.pyramid_pool([m[b] for m in levels], segs[b], S) for b in range(B)]
    return segs, S, dtype, levels, torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def bounding_box(seg, i):
    ys, xs = torch.nonzero(seg == i, as_tuple=True)
    return int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())


def box_cells(seg, i, s):
    """The cells of the stride-s grid whose sample pixel lies in id i's bounding box, as the pool kernel walks them:
    (cy0, cx0, cy1, cx1); empty when cy0 > cy1 or cx0 > cx1."""
    y0, x0, y1, x1 = bounding_box(seg, i)
    return (y0 + s - 1) // s, (x0 + s - 1) // s, y1 // s, x1 // s


def rounds_of(seg, i, s):
    """Matches per 64-cell round of the pool kernel's walk over id i's box at stride s."""
    cy0, cx0, cy1, cx1 = box_cells(seg, i, s)
    if cy0 > cy1 or cx0 > cx1:
        return []
    m = (seg[cy0 * s: cy1 * s + 1: s, cx0 * s: cx1 * s + 1: s] == i).reshape(-1)
    return [int(m[b: b + 64].sum()) for b in range(0, m.numel(), 64)]
