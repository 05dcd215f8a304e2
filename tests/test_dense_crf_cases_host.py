"""Coverage conditions of tests/dense_crf_cases.py, on the CPU: every named frame still reaches the kernel path it was chosen for
(sort tiles, radix pass parity, chunks per lattice point, contributors per point), evaluated on the float32 lattice statement of
tests/test_dense_crf_permutohedral.py.  These are conditions on the test inputs, not checks of the kernels: the GPU tests that use the
cases are in tests/test_gpu_dense_crf_permutohedral_edges.py."""
import functools

import numpy as np
import pytest

from tests.dense_crf_cases import CASES, CH, TILE, TINY, chunk_stats, key_bits, passes
from tests.test_dense_crf_permutohedral import features32, lattice32, lattice_literal


def _features(name, d):
    c = CASES[name]
    img = c.image(0).numpy()
    return features32(c.H, c.W, img, c.pos_xy) if d == 2 else features32(c.H, c.W, img, c.bi_xy, c.bi_rgb)


@functools.lru_cache(maxsize=None)
def _stats(name, d):
    """(M, points with at least one whole chunk, most chunks on a point, most contributors on a point, lowest and highest key)."""
    lat = lattice32(_features(name, d))
    count, chunks = chunk_stats(lat)
    assert count.sum() == CASES[name].E(d) and count.min() >= 1
    return lat["M"], int((chunks > 0).sum()), int(chunks.max()), int(count.max()), int(lat["keys"].min()), int(lat["keys"].max())


def _bits(name, d):
    c = CASES[name]
    return key_bits(d, c.H, c.W, c.pos_xy) if d == 2 else key_bits(d, c.H, c.W, c.bi_xy, c.bi_rgb)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_is_inside_the_accepted_range(name):
    c = CASES[name]
    assert 1 <= c.H <= 2048 and 1 <= c.W <= 2048                      # perm_shape_ok
    for d in (2, 5):
        assert _bits(name, d) is not None, (name, d)                   # lattice_setup does not refuse
        assert c.NT(d) == -(-c.E(d) // TILE)
    for b in range(3):
        img = c.image(b)
        assert img.dtype.is_floating_point is False and tuple(img.shape) == (c.H, c.W, 3) and img.element_size() == 1


def test_key_bits_of_the_tested_stego_constants():
    """The widths DESIGN.md quotes for pos_xy_std = 1 and 67 / 3: 46 bits (6 passes) for the bilateral lattice at every size the
    first tests use, 18 bits at 97 x 131 and 22 at 448^2 (3 passes) for the Gaussian; and two ranges the host refuses."""
    for H, W in ((64, 64), (40, 56), (97, 131), (224, 224), (448, 448)):
        assert key_bits(5, H, W, 67.0, 3.0) == 46
    assert key_bits(2, 97, 131, 1.0) == 18 and key_bits(2, 448, 448, 1.0) == 22
    assert key_bits(5, 8, 8, 67.0, 0.01) is None and key_bits(5, 8, 8, 67.0, 0.2) is None
    assert key_bits(2, 2048, 2048, 0.05) is None


def test_case_a_has_more_than_256_sort_tiles():
    b, gs = CASES["tiles_bilateral"], CASES["tiles_gaussian"]
    assert (b.H * b.W, b.E(5), b.NT(5)) == (87447, 524682, 257)
    assert (gs.E(2), gs.NT(2)) == (529197, 259)
    assert b.NT(5) >= 257 and gs.NT(2) >= 257
    # barely past it: one image row less and the bilateral lattice is back to a single scan round
    assert (b.E(5) - 6 * b.W + TILE - 1) // TILE <= 256
    assert passes(_bits("tiles_bilateral", 5)) == 6 and passes(_bits("tiles_gaussian", 2)) == 3
    M, with_chunk, most, longest, _, _ = _stats("tiles_bilateral", 5)
    assert 3000 <= M <= 8000 and with_chunk >= 1000 and most >= 8 and longest >= 512
    M, with_chunk, most, longest, _, _ = _stats("tiles_gaussian", 2)
    assert M > 200000 and with_chunk == 0 and longest <= 4


@pytest.mark.parametrize("name,gauss_bits,bi_bits,bi_passes", [("passes_5", 14, 37, 5), ("passes_7", 18, 52, 7), ("passes_4", 10, 31, 4)])
def test_case_b_pass_counts(name, gauss_bits, bi_bits, bi_passes):
    assert (CASES[name].H, CASES[name].W) == (40, 56)
    assert _bits(name, 2) == gauss_bits and _bits(name, 5) == bi_bits and passes(bi_bits) == bi_passes
    assert (bi_passes & 1) == {"passes_5": 1, "passes_7": 1, "passes_4": 0}[name]      # which ping-pong half holds the sorted pairs


def test_case_b_lattices_are_not_degenerate():
    assert _stats("passes_5", 5)[:4] == (113, 42, 13, 924)      # pydensecrf's defaults: few points, long lists
    assert _stats("passes_7", 5)[1:3] == (0, 0) and _stats("passes_7", 5)[0] > 8000 and _stats("passes_7", 2)[0] == 40 * 56 * 3
    assert _stats("passes_4", 5)[0] == 41 and _stats("passes_4", 2)[:4] == (7, 7, 34, 2240)


def test_case_c_contributor_extremes():
    assert all((CASES[n].H, CASES[n].W) == (64, 64) for n in ("constant", "flat_blocks", "random", "wide_gaussian"))
    # one colour: 21 lattice points, one of them with every pixel (4096 contributors, 63 whole chunks and a head)
    assert _stats("constant", 5)[:4] == (21, 18, 63, 4096)
    M, with_chunk, most, longest, _, _ = _stats("flat_blocks", 5)
    assert 40 <= M <= 80 and with_chunk >= 30 and most >= 20 and longest >= 20 * CH
    # noise: almost every vertex its own point, no chunk anywhere
    M, with_chunk, most, longest, _, _ = _stats("random", 5)
    assert M > 24000 and with_chunk == 0 and most == 0 and longest <= 3
    # the Gaussian lattice's chunk path (never reached at pos_xy_std = 1: at most 4 contributors)
    assert _stats("wide_gaussian", 2)[:4] == (10, 9, 50, 3275)
    for name in ("constant", "flat_blocks", "random", "blocky64"):
        assert _stats(name, 2)[1:4] == (0, 0, 4)
    assert _stats("constant", 5)[2] >= 50 and _stats("wide_gaussian", 2)[2] >= 50


def test_case_c_checker_has_the_widest_keys():
    assert (CASES["checker"].H, CASES["checker"].W) == (33, 47)
    img = CASES["checker"].image(0)
    assert set(img.unique().tolist()) == {0, 255}
    assert img[0, 0].tolist() == [255, 0, 0] and img[0, -1].tolist() == [0, 255, 0] and img[-1, 0].tolist() == [0, 0, 255]
    lo, hi = _stats("checker", 5)[4:]
    assert lo <= -370 and hi >= 290
    lo, hi = _stats("checker_narrow", 5)[4:]
    assert lo == -1120 and hi >= 880
    assert passes(_bits("checker", 5)) == 6 and passes(_bits("checker_narrow", 5)) == 7
    assert _stats("checker", 5)[1] > 0 and _stats("checker_narrow", 5)[1] > 0


def test_case_d_tiny_frames_are_below_a_chunk_or_a_tile():
    assert [(CASES[n].H, CASES[n].W) for n in TINY] == [(1, 1), (1, 70), (70, 1), (3, 5), (2, 11)]
    assert CASES["tiny_3x5"].E(2) == 45 < CH                     # no chunk position at all: a zero-byte partial buffer
    assert CASES["tiny_2x11"].E(2) == 66 and 66 // CH == 1 and 66 % CH == 2
    assert CASES["tiny_1x1"].E(2) == 3 and CASES["tiny_1x1"].E(5) == 6
    for n in TINY:
        assert CASES[n].NT(2) == 1 and CASES[n].NT(5) == 1


@pytest.mark.parametrize("d", [2, 5])
@pytest.mark.parametrize("name", TINY)
def test_case_d_statement_equals_the_literal_loop(name, d):
    f = _features(name, d)
    want, got = lattice_literal(f), lattice32(f)
    assert got["M"] == want["M"]
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["vert"], want["vert"])
    assert np.array_equal(got["bary"].view(np.int32), want["bary"].view(np.int32))
    assert np.array_equal(got["nbr"], want["nbr"])


def test_chunk_stats_on_a_hand_made_order():
    """Points of 70, 60, 130 and 1 contributors at sorted positions [0, 70), [70, 130), [130, 260), [260, 261): aligned 64-blocks
    inside them: {0}, none, {3} (192..255), none."""
    vert = np.repeat(np.array([1, 2, 3, 4]), [70, 60, 130, 1])
    count, chunks = chunk_stats(dict(M=4, vert=np.random.default_rng(0).permutation(vert).reshape(-1, 3)))
    assert count.tolist() == [70, 60, 130, 1] and chunks.tolist() == [1, 0, 1, 0]
