"""tests/resnet_cases.py without a GPU: every case of tests/test_gpu_resnet_shapes.py reaches the path it is there for.  The
conditions are asserted from the launch arithmetic of csrc/resnet.hip, the walk of csrc/pyramid_pool.hip restated on the segment map,
and the float64 statement tests/resnet_ref.py -- never from a kernel's output.  The refusals run the C entry points, which return
before anything touches a GPU."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_cases as RC  # noqa: E402
import resnet_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib, ops  # noqa: E402


# ---------------------------------------------------------------------------------------------------- convolution
def test_convolution_cases_reach_their_paths():
    geo = {c.name: RC.geometry(c) for c in RC.NHWC_CASES + RC.FRAME_CASES}
    assert len(geo) == len(RC.NHWC_CASES) + len(RC.FRAME_CASES) == 22
    # rectangular in and out wherever the case is not about a single pixel or a full tile
    for c in RC.NHWC_CASES + RC.FRAME_CASES:
        if not c.name.startswith(("one_pixel", "m64")):
            assert c.H != c.W and geo[c.name]["OH"] != geo[c.name]["OW"], c
    assert (geo["3x3s1_5x11"]["OH"], geo["3x3s1_5x11"]["OW"]) == (5, 11) and (geo["3x3s1_11x5"]["OH"], geo["3x3s1_11x5"]["OW"]) == (11, 5)
    assert (geo["3x3s2_7x12"]["OH"], geo["3x3s2_7x12"]["OW"]) == (4, 6)
    assert (geo["1x1s2_9x6"]["OH"], geo["1x1s2_9x6"]["OW"]) == (5, 3)
    assert geo["cin32_6x10"]["chunks_per_tap"] == 1 and geo["cin32_6x10"]["grid"][1] == 1
    assert geo["cin96_6x10"]["chunks_per_tap"] == 3 and geo["cin96_6x10"]["grid"][1] == 3 and 96 & 95
    assert geo["k7p3s2_9x14"]["K"] == 1568 and geo["k5p2_6x9"]["K"] == 800
    c = RC.CONV_BY_NAME["k2p0s2_7x10"]
    assert (geo[c.name]["OH"] - 1) * c.stride + c.k - 1 < c.H - 1            # the last input row is read by no window
    assert (geo["k3p0_5x8"]["OH"], geo["k3p0_5x8"]["OW"]) == (3, 6)
    assert (geo["k3p3_4x6"]["OH"], geo["k3p3_4x6"]["OW"]) == (8, 10) and RC.CONV_BY_NAME["k3p3_4x6"].pad > 3 // 2
    assert (geo["k1p1_4x7"]["OH"], geo["k1p1_4x7"]["OW"]) == (6, 9)
    assert geo["one_pixel_b1"]["M"] == 1 and geo["one_pixel_b2"]["M"] == 2 and geo["one_pixel_b2"]["OH"] == geo["one_pixel_b2"]["OW"] == 1
    assert (geo["one_row_1x7"]["OH"], geo["one_row_1x7"]["OW"]) == (1, 7)
    assert geo["m64_8x8"]["M"] == 64 and geo["m64_8x8"]["grid"][0] == 1
    assert geo["m256_8x16"]["M"] == 256 and geo["m256_8x16"]["grid"][0] == 4
    assert geo["m65_5x13"]["M"] == 65 and geo["m65_5x13"]["grid"][0] == 2
    # more than one tile of rows with a tail, and more than one K chunk, somewhere
    assert any(v["grid"][0] > 1 and v["M"] % RC.BM for v in geo.values())
    # the stems: a Kpad of several chunks (the prefetch branch is taken) and of one (it never is)
    assert geo["stem7x7_10x15"]["K"] == 147 and geo["stem7x7_10x15"]["Kpad"] == 160
    assert (geo["stem7x7_10x15"]["OH"], geo["stem7x7_10x15"]["OW"]) == (5, 8) and (geo["stem7x7_15x10"]["OH"], geo["stem7x7_15x10"]["OW"]) == (8, 5)
    assert geo["stem3x3_6x9"]["K"] == 27 and geo["stem3x3_6x9"]["Kpad"] == RC.BK
    assert geo["stem1x1_5x7"]["K"] == 3 and geo["stem1x1_5x7"]["Kpad"] == RC.BK


@pytest.mark.parametrize("case", RC.NHWC_CASES, ids=lambda c: c.name)
def test_exact_twin_is_exact_in_fp32(case):
    """K max|x| max|w| < 2^24: every partial sum of the chain is an integer fp32 holds; the epilogue's values are integers and halves
    far below 2^24.  The statement's results are then representable in fp32 one for one."""
    x, w, scale, shift, resid, want = RC.conv_exact_case(case.name)
    K = case.cin * case.k * case.k
    assert K * x.abs().max().item() * w.abs().max().item() < 2 ** 24
    assert x.abs().max() == RC.EXACT_X and set(w.unique().tolist()) == {-1.0, 0.0, 1.0} and torch.equal(x, x.round())
    assert set(scale.unique().tolist()) <= set(RC.EXACT_SCALES) and scale.unique().numel() >= 2
    assert torch.equal(shift, shift.round()) and torch.equal(resid, resid.round())
    for v in want.values():
        assert torch.equal(v * 2, (v * 2).round()) and v.abs().max() < 2 ** 20 and torch.equal(v.float().double(), v)
    assert (want[(True, False)] < 0).any() and (want[(True, True)] >= 0).all()


def test_windows_in_the_padding_give_the_shift():
    """pad > k / 2: the corner outputs' windows lie wholly in the zero padding, so before the residual they are exactly shift; with
    k = 1, pad = 1 that holds for the whole border."""
    x, w, scale, shift, resid, want = RC.conv_exact_case("k3p3_4x6")
    out = want[(False, False)]
    for cy, cx in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert torch.equal(out[:, :, cy, cx], shift.double().expand(2, -1))
    assert not torch.equal(out[:, :, 1, 1], shift.double().expand(2, -1))
    out = RC.conv_exact_case("k1p1_4x7")[5][(False, False)]
    sh = RC.conv_exact_case("k1p1_4x7")[3].double().view(1, -1, 1)
    assert torch.equal(out[:, :, 0, :], sh.expand(2, -1, 9)) and torch.equal(out[:, :, -1, :], sh.expand(2, -1, 9))
    assert torch.equal(out[:, :, :, 0], sh.expand(2, -1, 6)) and torch.equal(out[:, :, :, -1], sh.expand(2, -1, 6))


def test_float_cases_are_built_once_and_bounded():
    for c in RC.NHWC_CASES + RC.FRAME_CASES:
        x, w, bn, resid, want, bound = RC.conv_float_case(c.name)
        assert RC.conv_float_case(c.name)[0] is x                                # cached: shared, never rebuilt
        OH, OW = RC.out_hw(c)
        assert all(v.shape == (c.B, c.cout, OH, OW) and v.dtype == torch.float64 for v in want.values())
        assert all((b > 0).all() and b.shape == (c.B, c.cout, OH, OW) for b in bound.values())
        # the bound is a rounding-error bound: some 1e-7 to 1e-4 of the values, never a tolerance of their size
        assert bound[True].max().item() < 2e-3 * max(1.0, want[(True, False)].abs().max().item())
    u8 = RC.conv_float_case("stem7x7_10x15", True)[0]
    assert u8.dtype == torch.uint8 and u8.shape == (2, 3, 10, 15)


@pytest.mark.parametrize("name", list(RC.CONV_REFUSALS))
def test_c_entry_refuses_on_a_rectangular_input(name):
    h = _lib.lib()
    words = (C.c_longlong * 8)()
    p = C.addressof(words)   # never dereferenced: the call is refused first
    cin, cout, k, stride, pad, frame = RC.CONV_REFUSALS[name]
    kind = ops.CONV_IN_FRAME_F32 if frame else ops.CONV_IN_NHWC
    assert h.wvn_conv2d_bn_act(p, kind, p, p, p, None, 1, p, 2, 10, 15, cin, cout, k, stride, pad, None) == _lib.ERR_ARG
    assert all(w == 0 for w in words)


# ---------------------------------------------------------------------------------------------------- max-pool
def test_max_pool_cases():
    for H, W, Cc in RC.MAXPOOL_SHAPES:
        x, want = RC.maxpool_case(H, W, Cc)
        assert H != W or Cc % 64                                                  # rectangular, or a channel count off the usual 64
        assert want.shape == (2, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and (x < 0).all() and (want < 0).all()
    assert 2 * 1 * 1 * 130 > 256 and 2 * 8 * 5 * 5 > 256                         # (2, 2, 130) and (16, 9, 5): a second block of threads


# ---------------------------------------------------------------------------------------------------- whole network
@pytest.mark.parametrize("B, H, W", RC.NET_FRAMES)
def test_network_statement_on_rectangular_frames(B, H, W):
    img, f64, yard = RC.net_case(B, H, W)
    assert H != W and img.shape == (B, 3, H, W)
    for l, (k, v) in enumerate(f64.items()):
        s = REF.STRIDES[l]
        assert v.shape == (B, REF.CHANNELS[l], H // s, W // s) and v.max() > 0
        assert 1e-7 < yard[k] < 2e-6          # the fp32 CPU run of the same statement: the yardstick the GPU is held to 4 x of
    if (H, W) in ((32, 128), (128, 32)):
        assert f64["feat4"].shape[2:] == ((1, 4) if H == 32 else (4, 1))


def test_c_entry_workspace_arithmetic_on_rectangular_frames():
    h = _lib.lib()
    words = (C.c_longlong * 8)()
    p = C.addressof(words)
    for B, H, W in RC.NET_FRAMES:
        lv = [B * (H // s) * (W // s) * c * 4 for c, s in zip(REF.CHANNELS, REF.STRIDES)]
        al = [(v + 255) // 256 * 256 for v in lv]
        assert [h.wvn_resnet18_level_offset(B, H, W, l) for l in (1, 2, 3, 4)] == [0, al[0], al[0] + al[1], al[0] + al[1] + al[2]]
        need = sum(al) + 5 * al[0]
        assert h.wvn_resnet18_workspace_bytes(B, H, W) == need and need % 4 == 0
        assert h.wvn_resnet18_forward(p, p, 0, B, H, W, p, need - 4, None) == 1002          # one element short
    assert h.wvn_resnet18_workspace_bytes(3, 64, 96) > h.wvn_resnet18_workspace_bytes(1, 64, 96)
    assert h.wvn_resnet18_workspace_bytes(1, 48, 64) == 0 and h.wvn_resnet18_workspace_bytes(1, 64, 48) == 0
    assert h.wvn_resnet18_forward(p, p, 0, 1, 48, 64, p, 1 << 30, None) == _lib.ERR_ARG
    with pytest.raises(_lib.WvnError, match="multiples of 32"):
        ops.resnet18_workspace(1, 48, 64, "cpu")
    assert all(w == 0 for w in words)


# ---------------------------------------------------------------------------------------------------- pooling
def _cell(cy, cx, s, h, w):
    return min(cy // s, h - 1), min(cx // s, w - 1)


def test_wide_frame_conditions():
    segs, S, dtype, levels, want, fallback = RC.pool_case("wide")
    H, W = RC.POOL_H, RC.POOL_W
    assert segs.shape == (2, H, W) and H < W and S == 12 and not torch.equal(segs[0], segs[1])
    assert [m.shape for m in levels] == [(2, c, H // s, W // s) for c, s in zip(REF.CHANNELS, REF.STRIDES)]
    assert all(torch.equal(m, m.round()) and m.abs().max() <= 8 for m in levels)
    a = segs[0]
    # the background: more than 64 of the 72 level-4 cells, a second trip of the cell loop at every level
    assert (a[::32, ::32] == 0).sum() > 64 and a[::32, ::32].numel() == 72
    assert all(len(RC.rounds_of(a, 0, s)) >= 2 for s in REF.STRIDES)
    # the stripes: a box of more than 192 level-1 cells, and a 64-cell round without a match between rounds that have one
    cy0, cx0, cy1, cx1 = RC.box_cells(a, RC.STRIPE_ID, 4)
    rounds = RC.rounds_of(a, RC.STRIPE_ID, 4)
    assert (cy1 - cy0 + 1) * (cx1 - cx0 + 1) > 192 and 0 in rounds[1:-1] and rounds[0] > 0 and rounds[-1] > 0
    # the 30 x 30 block: the centroid cell at level 4 only
    y0, x0, y1, x1 = RC.bounding_box(a, RC.BLOCK_ID)
    assert (y1 - y0 + 1, x1 - x0 + 1) == (30, 30) and fallback[0, RC.BLOCK_ID].tolist() == [False, False, False, True]
    # the L: the centroid cell at every level; that cell holds none of its pixels; rounding the centroid, or exchanging the row and
    # column sums, names another cell
    ys, xs = torch.nonzero(a == RC.L_ID, as_tuple=True)
    n, sy, sx = ys.numel(), int(ys.sum()), int(xs.sum())
    cy, cx = REF.centroid(a, RC.L_ID)
    assert (cy, cx) == (sy // n, sx // n) and fallback[0, RC.L_ID].all()
    ry, rx = (2 * sy + n) // (2 * n), (2 * sx + n) // (2 * n)
    for s in REF.STRIDES:
        h, w = H // s, W // s
        cell = _cell(cy, cx, s, h, w)
        assert _cell(ry, rx, s, h, w) != cell and _cell(cx, cy, s, h, w) != cell
    assert (a[cy // 4 * 4: cy // 4 * 4 + 4, cx // 4 * 4: cx // 4 * 4 + 4] != RC.L_ID).all()
    # the level maps tell those cells apart (else a wrong cell could carry the right vector)
    for l, s in enumerate(REF.STRIDES):
        m, (h, w) = levels[l][0], (H // s, W // s)
        right, rounded, swapped = _cell(cy, cx, s, h, w), _cell(ry, rx, s, h, w), _cell(cx, cy, s, h, w)
        assert not torch.equal(m[:, right[0], right[1]], m[:, rounded[0], rounded[1]])
        assert not torch.equal(m[:, right[0], right[1]], m[:, swapped[0], swapped[1]])
    # single pixels: the last and the first column of a 16-pixel run, the last row, the last column
    pix = {i: torch.nonzero(a == i).tolist() for i in (4, 5, 6, 7)}
    assert all(len(v) == 1 for v in pix.values())
    assert pix[4][0][1] % 16 == 15 and pix[5][0][1] % 16 == 0 and pix[6][0][0] == H - 1 and pix[7][0][1] == W - 1
    assert fallback[0, 5].tolist() == [False, True, True, True] and fallback[0, 4].all() and fallback[0, 6].all() and fallback[0, 7].all()
    # ids outside [0, S) are present, one id below S is not
    assert (a == -1).sum() > 64 and (a >= S).sum() > 64 and (a == RC.ABSENT_ID).sum() == 0 and torch.isnan(want[0, RC.ABSENT_ID]).all()
    assert all((a == i).any() for i in range(S) if i != RC.ABSENT_ID) and all((segs[1] == i).any() for i in range(S))
    assert (segs[1] == -1).any() and (segs[1] >= S).any()
    # both branches carry at least a third of the present (id, level) pairs
    present = torch.stack([torch.tensor([(segs[b] == i).any().item() for i in range(S)]) for b in range(2)])
    n_fall, n_mean = int(fallback.sum()), int((present[:, :, None] & ~fallback).sum())
    assert 3 * n_fall >= n_fall + n_mean and 3 * n_mean >= n_fall + n_mean, (n_fall, n_mean)
    assert torch.equal(torch.isnan(want).all(2), ~present) and torch.equal(torch.isnan(want).any(2), ~present)


def test_tall_and_one_id_frame_conditions():
    segs, S, dtype, levels, want, fallback = RC.pool_case("tall")
    assert segs.shape == (1, 96, 32) and S == 5 and dtype == torch.int64 and levels[3].shape == (1, 512, 3, 1)
    assert fallback.any() and (~fallback).any() and not torch.isnan(want).any() and (segs == -1).any()
    assert fallback[0, :, 3].sum() >= 2                    # the three level-4 samples cannot carry five ids
    segs, S, dtype, levels, want, fallback = RC.pool_case("one_id")
    assert segs.shape == (1, 32, 32) and S == 1 and not fallback.any() and levels[3].shape == (1, 512, 1, 1)
    assert torch.equal(want[0, 0, 448:], levels[3][0, :, 0, 0].double())
    assert torch.equal(want[0, 0, :64], levels[0][0].double().mean((1, 2)))            # (integer maps: exact in any order)
    segs, S, dtype, levels, want, fallback = RC.pool_case("one_id_s3000")
    assert S == 3000 and torch.isnan(want[0, 1:]).all() and not torch.isnan(want[0, 0]).any()
    assert torch.equal(want[0, 0], RC.pool_case("one_id")[4][0, 0])


def test_randn_frame_for_the_factor_rule():
    segs, S, dtype, levels, want, fallback = RC.pool_case("wide", "randn")
    assert torch.equal(segs, RC.pool_case("wide")[0]) and torch.equal(fallback, RC.pool_case("wide")[5])
    assert not torch.equal(levels[0], levels[0].round())
