"""Connectivity enforcement without a GPU: the plain statement (tests/slic_connectivity_ref.py) against maps whose answer is worked
out by hand and against its own properties on real SLIC maps; argument validation of the two C entry points; the public keywords."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slic_connectivity_ref as REF  # noqa: E402

from oracle import slic as OSL  # noqa: E402
from wild_visual_navigation_amd import _lib, ops  # noqa: E402
from wild_visual_navigation_amd.feature_extractor import FeatureExtractor  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", REF.hand_cases(), ids=lambda c: c[0])
def test_plain_statement_on_hand_written_maps(case):
    _, labels, min_size, expected = case
    assert np.array_equal(REF.enforce_connectivity(labels, min_size), expected)


def test_nested_island_takes_two_rounds():
    _, labels, min_size, _ = [c for c in REF.hand_cases() if c[0] == "nested"][0]
    assert REF.enforce_connectivity(labels, min_size, return_rounds=True)[1] == 2


def test_plain_statement_on_slic_maps_of_the_demo_frames():
    frames = torch.load(os.path.join(ROOT, "tests", "golden", "demo_frames_224.pt"))["frames_u8"]
    K = 100
    min_size = REF.min_size_for(224, 224, K)
    assert min_size == 125
    for i in range(frames.shape[0]):
        L = OSL.slic(frames[i, :, :, :224].contiguous().numpy(), 100, 10.0)
        before = REF.small_components(L, min_size)
        out, rounds = REF.enforce_connectivity(L, min_size, return_rounds=True)
        print(f"frame {i}: {before} components below {min_size}, {rounds} rounds, {(out != L).sum()} pixels change")
        # not vacuous: this input exercises chains (measured 864 - 6480 components and 3 - 7 rounds)
        assert before >= 100 and rounds >= 3
        assert out.dtype == np.int32 and out.min() >= 0 and out.max() < K
        assert REF.small_components(out, min_size) == 0
        assert np.array_equal(REF.enforce_connectivity(out, min_size), out)


def test_argument_validation_without_gpu():
    h = _lib.lib()
    p = 1 << 20   # (never dereferenced: every call below is refused first)
    good = h.wvn_slic_connectivity_scratch_bytes(2, 224, 224, 100)
    assert good >= 2 * 224 * 224 * 4 * 7
    assert h.wvn_slic_connectivity_scratch_bytes(0, 224, 224, 100) == 0
    assert h.wvn_slic_connectivity_scratch_bytes(1, 0, 224, 100) == 0 and h.wvn_slic_connectivity_scratch_bytes(1, 224, 0, 100) == 0
    assert h.wvn_slic_connectivity_scratch_bytes(1, 224, 224, 0) == 0
    assert h.wvn_slic_connectivity_scratch_bytes(1, 1 << 15, 1 << 15, 100) == 0      # beyond the 32-bit index range of the kernels

    def call(lin=p, lout=p, B=2, H=224, W=224, K=100, min_size=125, scratch=p, nbytes=good):
        return h.wvn_slic_connectivity(lin, lout, B, H, W, K, min_size, scratch, nbytes, None)

    assert call(lin=None) == 1001 and call(lout=None) == 1001 and call(scratch=None) == 1001
    assert call(min_size=0) == 1001 and call(min_size=-3) == 1001
    assert call(K=0) == 1001 and call(B=0) == 1001 and call(H=0) == 1001 and call(W=0) == 1001
    assert call(nbytes=good - 1) == 1001 and call(nbytes=0) == 1001
    assert call(H=1 << 15, W=1 << 15) == 1001


def test_tile_constants_of_header_and_ops_agree():
    src = open(os.path.join(ROOT, "include", "wvn_hip.h")).read()
    th = int(re.search(r"#define WVN_SLIC_CC_TILE_H (\d+)", src).group(1))
    tw = int(re.search(r"#define WVN_SLIC_CC_TILE_W (\d+)", src).group(1))
    assert ops.SLIC_CC_TILE == (th, tw)


def test_min_size_rule():
    assert ops.slic_min_size(224, 224, 100) == 125 and ops.slic_min_size(448, 448, 100) == 501
    assert ops.slic_min_size(8, 8, 100) == 1 and ops.slic_min_size(224, 224, 100, 0.5) == 250


def test_public_keywords_and_their_defaults():
    sig = inspect.signature(ops.slic)
    assert sig.parameters["enforce_connectivity"].default is False and sig.parameters["min_size_factor"].default == 0.25
    fe = FeatureExtractor("cpu", feature_type="none")                      # segmentation_type defaults to "slic"
    assert fe.segmentation_type == "slic"
    assert fe._slic_enforce_connectivity is False and fe._slic_min_size_factor == 0.25
    fe = FeatureExtractor("cpu", feature_type="none", slic_enforce_connectivity=True, slic_min_size_factor=0.5)
    assert fe._slic_enforce_connectivity is True and fe._slic_min_size_factor == 0.5


def test_no_cpu_fallback():
    with pytest.raises(_lib.WvnError):
        ops.slic_enforce_connectivity(torch.zeros(4, 4, dtype=torch.int32), 2, 2)
