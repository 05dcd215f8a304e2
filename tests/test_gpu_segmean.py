"""ops.segmean_tokens (segmean_partial_kernel / segmean_final_kernel in csrc/segments.hip; the route of FeatureExtractor.sparsify_features
on a dense map) against float64, at the shapes its one golden test leaves out: a pixel count that is no multiple of the 2048-pixel chunk,
a channel count that is no multiple of 64, a segment count at the LDS limit (S * 65 * 4 <= 60 KB: S <= 236), ids outside [0, S)."""
import numpy as np
import pytest
import torch

from wild_visual_navigation_amd import _lib

pytestmark = pytest.mark.gpu

WVN_ERR_ARG = 1001
U = 2.0 ** -24   # unit round-off of fp32
# (B, P, S, D): two chunks with a 37-pixel tail and a 6-channel slab tail | three chunks, S at the limit, D < 64 | one short chunk,
# one segment | whole chunks, six full slabs
CASES = [(2, 2048 + 37, 7, 70), (1, 5000, 236, 33), (2, 300, 1, 64), (1, 4096, 50, 384)]


def _ids(B, P, S, seed):
    """ids in [-1, S + 2): -1, S and S + 1 must be ignored; in frame 0 the id S // 2 is left without pixels (its row must be NaN)."""
    seg = np.random.default_rng(seed).integers(-1, S + 2, (B, P)).astype(np.int32)
    seg[0][seg[0] == S // 2] = -1
    return seg


def _raw_segmean(seg, tok, S, dev, guard=256):
    """lib().wvn_segmean_tokens on guarded buffers -> (feat [B,S,D], cnt [B,S]) as numpy."""
    B, P, D = tok.shape
    h = _lib.lib()
    seg_d, tok_d = torch.from_numpy(seg).to(dev), torch.from_numpy(tok).to(dev)
    out = torch.full((guard + B * S * D + guard,), float("inf"), dtype=torch.float32, device=dev)
    cnt = torch.full((guard + B * S + guard,), -7, dtype=torch.int32, device=dev)
    nbytes = h.wvn_segmean_scratch_bytes(B, P, S, D)
    scratch = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    rc = h.wvn_segmean_tokens(seg_d.data_ptr(), tok_d.data_ptr(), out.data_ptr() + guard * 4, cnt.data_ptr() + guard * 4, scratch.data_ptr(),
                              nbytes, B, P, S, D, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool(torch.isinf(out[:guard]).all()) and bool(torch.isinf(out[guard + B * S * D:]).all()), "feat written out of bounds"
    assert bool((cnt[:guard] == -7).all()) and bool((cnt[guard + B * S:] == -7).all()), "cnt written out of bounds"
    assert bool((scratch[nbytes:] == 0xA5).all()), "scratch written past wvn_segmean_scratch_bytes"
    return out[guard:guard + B * S * D].reshape(B, S, D).cpu().numpy(), cnt[guard:guard + B * S].reshape(B, S).cpu().numpy()


def _reference(seg, tok, S):
    """float64: per (frame, id) the pixel count, the sum and the sum of |x| over the pixels with that id."""
    B, P, D = tok.shape
    n = np.zeros((B, S), np.int64)
    s = np.zeros((B, S, D), np.float64)
    sa = np.zeros((B, S, D), np.float64)
    t64 = tok.astype(np.float64)
    for b in range(B):
        ok = (seg[b] >= 0) & (seg[b] < S)
        n[b] = np.bincount(seg[b][ok], minlength=S)
        np.add.at(s[b], seg[b][ok], t64[b][ok])
        np.add.at(sa[b], seg[b][ok], np.abs(t64[b][ok]))
    return n, s, sa


@pytest.mark.parametrize("B,P,S,D", CASES)
def test_segmean_integer_tokens_exact(dev, B, P, S, D):
    """Tokens are integers in [-64, 64]: every partial and total sum is exact in fp32 whatever the order (|sum| <= 64 * 5000 < 2^24), so the
    result is float32(sum / n) up to the one division: within 1 ulp of the float64 quotient rounded to fp32, equal to it if fp32 division
    is correctly rounded (float64 -> float32 double rounding of a quotient of 24-bit operands is innocuous).  Observed on gfx950: equal in every
    element of the four cases (0 of 27 545 means differ)."""
    seg = _ids(B, P, S, seed=B * P + S)
    tok = np.random.default_rng(D).integers(-64, 65, (B, P, D)).astype(np.float32)
    got, cnt = _raw_segmean(seg, tok, S, dev)
    n, s, _ = _reference(seg, tok, S)
    assert np.array_equal(cnt, n), "pixel counts"
    assert n[0, S // 2] == 0 and (n.sum() > 0)
    empty = n == 0
    assert np.isnan(got[empty]).all() and np.isfinite(got[~empty]).all()
    want = (s[~empty] / n[~empty][:, None]).astype(np.float32)
    g = got[~empty]
    ulp = np.spacing(np.abs(want))
    inexact = int((g != want).sum())
    print(f"(B,P,S,D)=({B},{P},{S},{D}): {inexact} of {g.size} means differ from the correctly rounded quotient; "
          f"worst {np.max(np.abs(g.astype(np.float64) - want) / ulp):.2f} ulp")
    assert (np.abs(g.astype(np.float64) - want.astype(np.float64)) <= ulp).all()


@pytest.mark.parametrize("B,P,S,D", CASES)
def test_segmean_real_tokens_within_the_summation_bound(dev, B, P, S, D):
    """randn tokens: |got - mean64| <= (n_s - 1) 2^-24 mean_s|x| + 2^-24 |mean64| per element -- the forward bound of recursive fp32
    summation (any order) plus one division.  Derived, not measured; the worst ratio of error to bound is printed."""
    seg = _ids(B, P, S, seed=B * P + S + 1)
    tok = torch.randn(B, P, D, generator=torch.Generator().manual_seed(P + D)).numpy()
    got, cnt = _raw_segmean(seg, tok, S, dev)
    n, s, sa = _reference(seg, tok, S)
    assert np.array_equal(cnt, n)
    empty = n == 0
    assert empty[0, S // 2] and np.isnan(got[empty]).all()
    nn = n[~empty][:, None].astype(np.float64)
    mean = s[~empty] / nn
    bound = (nn - 1) * U * (sa[~empty] / nn) + U * np.abs(mean)
    err = np.abs(got[~empty].astype(np.float64) - mean)
    ratio = err / bound
    print(f"(B,P,S,D)=({B},{P},{S},{D}): worst error / bound = {ratio.max():.3f}, max|err| = {err.max():.3e}, pixels per id up to {int(n.max())}")
    assert (err <= bound).all()


def test_segmean_refuses_more_segments_than_fit_in_lds(dev):
    """S = 237: 237 * 65 * 4 = 61 620 B > 60 KB.  WVN_ERR_ARG, and nothing written; S = 236 is the last that runs (a case above)."""
    B, P, S, D = 1, 300, 237, 8
    h = _lib.lib()
    seg = torch.zeros(B, P, dtype=torch.int32, device=dev)
    tok = torch.ones(B, P, D, dtype=torch.float32, device=dev)
    out = torch.full((B, S, D), float("inf"), dtype=torch.float32, device=dev)
    cnt = torch.full((B * S,), -7, dtype=torch.int32, device=dev)
    nbytes = h.wvn_segmean_scratch_bytes(B, P, S, D)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    rc = h.wvn_segmean_tokens(seg.data_ptr(), tok.data_ptr(), out.data_ptr(), cnt.data_ptr(), scratch.data_ptr(), nbytes, B, P, S, D,
                              _lib.stream())
    torch.cuda.synchronize()
    assert rc == WVN_ERR_ARG
    assert bool(torch.isinf(out).all()) and bool((cnt == -7).all()) and bool((scratch == 0xA5).all())
