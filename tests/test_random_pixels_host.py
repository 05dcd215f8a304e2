"""The random-pixel sampler's definition without a GPU: the plain statement (tests/random_pixels_ref.py) is a permutation, its map is
consistent with its indices, and the draws are uniform over the frame; argument validation of the two C entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import random_pixels_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib  # noqa: E402

SIZES = [(24, 24), (32, 32), (33, 33), (5, 7)]   # 32 x 32 = 4^5 exactly: no cycle walking
CHI2_LIMIT = 37.70   # the 0.999 quantile of chi-square with 15 degrees of freedom (4 x 4 cells)


@pytest.mark.parametrize("H,W", SIZES)
def test_full_draw_is_a_permutation(H, W):
    for seed, frame in ((0, 0), (1, 5), (2, 2 ** 32 - 1)):
        idx, _ = REF.random_pixels(1, H, W, H * W, seed=seed, frame0=frame)
        assert np.array_equal(np.sort(idx[0]), np.arange(H * W))


def test_32x32_needs_no_cycle_walking():
    assert REF.half_bits(32 * 32) == 5 and 4 ** 5 == 32 * 32
    assert REF.half_bits(33 * 33) == 6 and REF.half_bits(24 * 24) == 5 and REF.half_bits(35) == 3 and REF.half_bits(1) == 0


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("nr", [1, 7, None])
def test_map_is_consistent_with_indices(H, W, nr):
    nr = H * W if nr is None else nr
    idx, seg = REF.random_pixels(2, H, W, nr, seed=3, frame0=11)
    for b in range(2):
        assert np.array_equal(seg[b].reshape(-1)[idx[b]], np.arange(nr))
        assert int((seg[b] >= 0).sum()) == nr
        assert seg[b].min() >= -1 and seg[b].max() == nr - 1


def test_inverse_inverts():
    for n_pix in (1, 2, 35, 576, 1024, 1089):
        j = np.arange(n_pix)
        assert np.array_equal(REF.pi_inv(REF.pi(j, n_pix, 4, 9), n_pix, 4, 9), j)


def _chi2(pixels, H, W):
    y, x = pixels // W, pixels % W
    cell = (y // (H // 4)) * 4 + x // (W // 4)
    counts = np.bincount(cell, minlength=16).astype(np.float64)
    expect = pixels.size / 16.0
    return float(((counts - expect) ** 2 / expect).sum())


@pytest.mark.parametrize("H", [224, 24])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_draws_are_uniform_over_the_frame(H, seed):
    """100 samples of each of frames 0..63 over 4 x 4 equal cells: 400 expected per cell."""
    px = np.concatenate([REF.pi(np.arange(100), H * H, seed, f) for f in range(64)])
    stat = _chi2(px, H, H)
    print(f"H={H} seed={seed} chi2={stat:.2f}")
    assert stat < CHI2_LIMIT


@pytest.mark.parametrize("H", [224, 24])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_first_draw_is_uniform_over_frames(H, seed):
    """j = 0 alone over frames 0..4095: 256 expected per cell."""
    px = np.concatenate([REF.pi(0, H * H, seed, f) for f in range(4096)])
    stat = _chi2(px, H, H)
    print(f"H={H} seed={seed} first-draw chi2={stat:.2f}")
    assert stat < CHI2_LIMIT


def test_same_key_same_samples_and_frames_differ():
    a, sa = REF.random_pixels(1, 24, 24, 100, seed=5, frame0=9)
    b, sb = REF.random_pixels(1, 24, 24, 100, seed=5, frame0=9)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    c, _ = REF.random_pixels(1, 24, 24, 100, seed=5, frame0=10)
    d, _ = REF.random_pixels(1, 24, 24, 100, seed=6, frame0=9)
    assert not np.array_equal(a, c) and not np.array_equal(a, d)
    # a batch is its frames one after the other, and the frame index wraps at 2^32
    e, se = REF.random_pixels(2, 5, 7, 35, seed=5, frame0=2 ** 32 - 1)
    f, sf = REF.random_pixels(1, 5, 7, 35, seed=5, frame0=0)
    assert np.array_equal(e[1], f[0]) and np.array_equal(se[1], sf[0])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """WVN_ERR_ARG (1001) before any launch: nr > H*W, nr < 1, H*W > 2^30, null outputs."""
    h = _lib.lib()
    p = 1 << 20   # (never dereferenced)
    assert h.wvn_random_pixels(0, 0, 1, 8, 8, 65, p, p, None) == 1001
    assert h.wvn_random_pixels(0, 0, 1, 8, 8, 0, p, p, None) == 1001
    assert h.wvn_random_pixels(0, 0, 1, 32768, 32769, 1, p, p, None) == 1001
    assert h.wvn_random_pixels(0, 0, 0, 8, 8, 1, p, p, None) == 1001
    assert h.wvn_random_pixels(0, 0, 1, 8, 8, 1, None, None, None) == 1001
    assert h.wvn_gather_bilinear(None, p, p, 1, 2, 8, 4, 1, None) == 1001
    assert h.wvn_gather_bilinear(p, p, p, 1, 2, 8, 4, 0, None) == 1001
    assert h.wvn_gather_bilinear(p, p, p, 1, 0, 8, 4, 1, None) == 1001
    assert h.wvn_gather_bilinear(p, p, p, 1, 2, 32769, 4, 1, None) == 1001
