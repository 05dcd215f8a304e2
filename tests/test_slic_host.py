"""The integer SLIC without a GPU: what the rows of tests/slic_cases.py are worth, and the oracle itself held to something.

* ``slic_switchable`` with every switch off is ``oracle.slic.slic`` on every row.
* Every mutant (one rule of the algorithm stated wrongly) gives other labels than the oracle on the rows named for it below, so the
  bit-for-bit GPU comparison of those rows (tests/test_gpu_slic.py) depends on that rule.  All nine are killed; none had to be given up.
  Findings on the way: the rounding of m2q (0.02^2 * 4096 = 1.6384 -> 2, truncated 1) shows on NO smooth, noise, flat or block frame --
  the colour term outweighs it by orders of magnitude -- and needed the `faint_noise` builder; an emptied cluster's centre (kept or
  zeroed) matters on 3 of 49 `blocks` seeds only (slic_cases.BLOCKS_SEED).
* ``oracle.slic.lab64`` is CIELAB: over all 2^24 colours |lab64 / 64 - float64 CIELAB| is at most 0.2226 (L), 1.2553 (a), 0.6272 (b).
* ``wvn_slic_num_clusters`` (host arithmetic of the library) is the oracle's nx * ny.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_cases as SC  # noqa: E402

from oracle import slic as OSL  # noqa: E402
from wild_visual_navigation_amd import _lib  # noqa: E402


def test_case_table_has_the_geometry_it_claims():
    """The rows are there for their pixel-count remainders, grid shapes and LDS sizes: hold them to it."""
    want = {"tail169": (169, None), "tail255": (255, None), "tail172": (172, 35), "onerow": (None, 17), "onecol": (None, 17),
            "flat": (None, 23), "single": (None, 1), "pixel": (None, 1), "lds57600": (None, 2880), "lds61440": (None, 3072),
            "lds52020": (None, 2601), "compact": (None, 36), "ties": (None, 20), "empty": (None, 20)}
    seen = set()
    for c in SC.CASES:
        tag = c.name.split("-")[0]
        _, nx, ny, _ = OSL.geometry(c.H, c.W, c.num_components, c.compactness)
        if tag in want:
            rem, K = want[tag]
            assert rem is None or (c.H * c.W) % 256 == rem, c.name
            assert K is None or nx * ny == K, (c.name, nx, ny)
            seen.add(tag)
        if tag == "onerow" or tag == "flat":
            assert ny == 1 and nx > 2
        if tag == "onecol":
            assert nx == 1 and ny > 2
        if tag.startswith("lds"):
            assert 48 * 1024 < 5 * nx * ny * 4 <= 60 * 1024
    assert seen == set(want)
    assert len({c.name for c in SC.CASES}) == len(SC.CASES)
    assert OSL.geometry(96, 96, 40, 0.02)[3] == 2 and int(np.float32(0.02) * np.float32(0.02) * np.float32(4096.0)) == 1
    assert any(c.H * c.W < 64 for c in SC.CASES) and any(c.W < 64 < c.H * c.W for c in SC.CASES)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_switchable_restatement_equals_the_oracle(case):
    got = SC.slic_switchable(SC.image(case), case.num_components, case.compactness, case.iters)
    want = SC.oracle_labels(case)
    assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want)


# mutant -> (switch, rows that must tell it from the oracle).  Every row named here is compared bit for bit on the GPU.
KILLERS = {
    "1 ties to the highest id": (dict(ties_highest=True), (
        "ties-const-70x90-n20-m0-it10", "ties-const-70x90-n20-m10-it10", "ties-halves-70x90-n20-m10-it10",
        "ties-two_level_noise-70x90-n20-m0.5-it10", "ties-const-70x90-n20-m10-it1")),
    "2 emptied cluster's centre zeroed": (dict(empty_zeroed=True), (
        "empty-blocks-64x80-n20-m0.02-it10", "empty-blocks-64x80-n20-m1-it10")),
    "3 centre update truncated": (dict(update_truncated=True), (
        "compact-smooth-96x96-n40-m1000-it10", "tail172-smooth-50x70-n30-m10-it10", "ties-two_level_noise-70x90-n20-m10-it10")),
    "4 centre update with C division": (dict(update_c_division=True), (
        "tail172-smooth-50x70-n30-m10-it10", "wrap-float_wrap-70x90-n20-m0.5-it10", "ties-noise-70x90-n20-m10-it10")),
    "5 m2q truncated": (dict(m2q_truncated=True), (
        "m2q-faint_noise-96x96-n40-m0.02-it10", "m2q-faint_noise-64x80-n20-m0.02-it10")),
    "6 float to uint8 by rounding": (dict(u8_round=True), (
        "wrap-float_wrap-37x53-n12-m10-it10", "float-smooth_float-72x104-n100-m10-it10")),
    "7 float to uint8 saturating": (dict(u8_saturate=True), (
        "wrap-float_wrap-37x53-n12-m10-it10", "wrap-float_wrap-70x90-n20-m0.5-it10")),
    "8a window misses its last row of cells": (dict(window_short="row"), (
        "onerow-smooth-8x200-n10-m10-it10", "flat-noise-3x300-n5-m10-it10", "tail169-noise-37x53-n12-m10-it10")),
    "8b window misses its last column of cells": (dict(window_short="col"), (
        "onecol-noise-200x8-n10-m10-it10", "tail255-smooth-65x63-n9-m10-it10")),
    "9 one update too many": (dict(extra_update=True), (
        "ties-noise-70x90-n20-m10-it1", "ties-noise-70x90-n20-m10-it2", "tail169-smooth-37x53-n12-m10-it10",
        "e2e-noise-72x104-n100-m10-it10")),
}


@pytest.mark.parametrize("mutant", list(KILLERS), ids=lambda m: m.replace(" ", "_"))
def test_every_mutant_is_killed(mutant):
    switch, rows = KILLERS[mutant]
    for name in rows:
        c = SC.by_name(name)
        got = SC.slic_switchable(SC.image(c), c.num_components, c.compactness, c.iters, **switch)
        share = float((got != SC.oracle_labels(c)).mean())
        print(f"mutant {mutant}: {name}: {100 * share:.2f} % of the labels differ")
        assert share > 0, f"{name} no longer tells mutant '{mutant}' from the oracle"


def test_inputs_take_the_paths_they_are_there_for():
    """Counters of the restatement: clusters are emptied on the `blocks` rows, ties decide labels on the flat rows, centre sums are
    negative where the floor division is tested, and on a noise row next to no wave of 64 pixels agrees on one cluster."""
    st = {}
    c = SC.by_name("empty-blocks-64x80-n20-m0.02-it10")
    SC.slic_switchable(SC.image(c), c.num_components, c.compactness, c.iters, stats=st)
    assert st["empty_events"] >= 8
    c = SC.by_name("ties-const-70x90-n20-m10-it10")
    SC.slic_switchable(SC.image(c), c.num_components, c.compactness, c.iters, stats=st)
    assert st["tied_pixels"] >= 1000 and st["empty_events"] == 0
    c = SC.by_name("tail172-smooth-50x70-n30-m10-it10")
    SC.slic_switchable(SC.image(c), c.num_components, c.compactness, c.iters, stats=st)
    assert st["negative_sums"] >= 100

    def uniform_wave_share(case):
        lab = SC.oracle_labels(case).ravel()
        full = lab[: lab.size // 64 * 64].reshape(-1, 64)
        return float((full == full[:, :1]).all(1).mean())

    noisy = uniform_wave_share(SC.by_name("compact-noise-96x96-n40-m0-it10"))
    wide = [uniform_wave_share(SC.by_name(f"wide-{b}-130x200-n4-m1000-it10")) for b in ("smooth", "noise")]
    lone = uniform_wave_share(SC.by_name("single-noise-61x67-n1-m10-it10"))
    print(f"waves that agree on one cluster: noise, compactness 0: {noisy:.3f}; 66-pixel cells: smooth {wide[0]:.3f}, noise {wide[1]:.3f}; "
          f"one cluster: {lone:.3f}")
    # (cells narrower than a wave -- every other row -- never take the wave-reduced path; the wide and single rows are there for it)
    assert noisy == 0.0 and lone == 1.0 and 0.05 < wide[0] < 0.95


# measured over all 2^24 colours (deterministic integer arithmetic: no margin), rounded up to the next 0.01
LAB_BOUND = (0.23, 1.26, 0.63)


def test_integer_lab_is_cielab_over_every_colour():
    """|lab64 / 64 - float64 CIELAB| over all 2^24 sRGB colours: 0.2226 (L), 1.2553 (a), 0.6272 (b) -- a quarter of a unit of L and about one
    of a and b (a just-noticeable difference is about 2.3), from the 12-bit linear and XYZ tables."""
    worst = np.zeros(3)
    for r0 in range(0, 256, 16):
        u8 = SC.all_colours_slab(r0, r0 + 16)
        err = np.abs(OSL.lab64(u8) / 64.0 - SC.cielab_float64(u8))
        worst = np.maximum(worst, err.max(axis=1))
    print(f"integer Lab against float64 CIELAB, all 2^24 colours: max|dL| = {worst[0]:.4f}, max|da| = {worst[1]:.4f}, max|db| = {worst[2]:.4f}")
    for ch in range(3):
        assert worst[ch] <= LAB_BOUND[ch], (ch, worst)
        assert worst[ch] > LAB_BOUND[ch] - 0.01, f"the bound of channel {ch} is stale: measured {worst[ch]}"


def test_num_clusters_is_the_oracles_geometry():
    """wvn_slic_num_clusters for H, W in 1 .. 80 and eight component counts, among them H*W, H*W + 1 and 10^6 (S2 = 1) and the perfect
    squares of S2, where an integer square root off by one shows."""
    h = _lib.lib()
    squares = 0
    for H in range(1, 81):
        for W in range(1, 81):
            for nc in (1, 2, 7, 36, 100, H * W, H * W + 1, 10 ** 6):
                S2, nx, ny, _ = OSL.geometry(H, W, nc)
                r = int(np.sqrt(S2))
                squares += r * r == S2 and S2 > 1
                got = h.wvn_slic_num_clusters(H, W, nc)
                assert got == nx * ny, (H, W, nc, got, nx, ny)
    assert squares > 100
    assert OSL.geometry(60, 60, 36)[0] == 100 and h.wvn_slic_num_clusters(60, 60, 36) == 36
    assert h.wvn_slic_num_clusters(0, 8, 4) == 0 and h.wvn_slic_num_clusters(8, 8, 0) == 0


def test_debug_slic_lab_validates_its_arguments():
    h = _lib.lib()
    p = 1 << 20   # (never dereferenced: every call below is refused first)
    assert h.wvn_debug_slic_lab(None, 1, 16, p, p, p, None) == 1001
    assert h.wvn_debug_slic_lab(p, 1, 16, None, p, p, None) == 1001
    assert h.wvn_debug_slic_lab(p, 1, 16, p, None, p, None) == 1001
    assert h.wvn_debug_slic_lab(p, 0, 16, p, p, None, None) == 1001
    assert h.wvn_debug_slic_lab(p, 1, 0, p, p, p, None) == 1001 and h.wvn_debug_slic_lab(p, 0, -5, p, p, p, None) == 1001
