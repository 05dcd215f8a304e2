"""Segment-graph kernels (csrc/segments.hip) at production sizes against the CPU oracle: adjacency and centres beyond one
bitmap byte per compaction thread, label pooling and the fused bilinear pooling on ViT/16- and DINOv2/14-style grids, on both sides
of the LDS limit that picks the weights kernel, and the square-frame contract of the fused pooling.  Maps and references are built
once per module and never modified (tests clone before they plant anything)."""
import functools

import pytest
import torch

from oracle import interfaces as OI, segments as OS
from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd._lib import lib, ptr, stream

pytestmark = pytest.mark.gpu

WVN_ERR_ARG = 1001
NAN = float("nan")


def g(seed):
    return torch.Generator().manual_seed(seed)


def _blobs(H, W, S, seed):
    """Voronoi cells of S random centres (the construction of tests/test_gpu_kernels.py)."""
    gg = g(seed)
    cy, cx = torch.rand(S, generator=gg) * H, torch.rand(S, generator=gg) * W
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    return ((ys[..., None] - cy) ** 2 + (xs[..., None] - cx) ** 2).argmin(-1)


# (H, W, S): S = 33 is the first size at which a compaction thread owns two bitmap bytes (33 * 33 > 1024); 100 and 196 are the SLIC and
# 16-pixel-grid sizes (10 and 38 bytes per thread); 300 gives 88 bytes per thread and leaves the last thread ranges past S * S
GRAPH_MAPS = [("blobs", 64, 64, 33), ("blobs", 96, 160, 100), ("blobs", 224, 224, 196), ("grid16", 224, 224, 196),
              ("blobs", 100, 100, 300)]
GRAPH_IDS = [f"{k}-{H}x{W}-S{S}" for k, H, W, S in GRAPH_MAPS]


@functools.lru_cache(maxsize=None)
def _graph_map(kind, H, W, S):
    """-> (seg [H,W] int64 with ids 0..max, n_seg = max id + 1)."""
    seg = OS.segment_grid(H, W, 16)[0, 0].clone() if kind == "grid16" else _blobs(H, W, S, 100 + S)
    return seg, int(seg.max()) + 1


@functools.lru_cache(maxsize=None)
def _graph_map_holed(kind, H, W, S):
    """The map with a band of -1 rows, a -1 column, ids >= n_seg and one id (3) without pixels."""
    seg, n_seg = _graph_map(kind, H, W, S)
    seg = seg.clone()
    seg[seg == 3] = 0
    seg[H // 3:H // 3 + 5, :] = -1
    seg[:, W // 2] = -1
    seg[H // 2, 3:9] = n_seg
    seg[H - 2, 1:4] = n_seg + 9
    seg[1, W - 3] = 1 << 30
    return seg, n_seg


def _edges_bruteforce(seg, S):
    """Set of (left, right) over horizontally / vertically adjacent pixel pairs with both ids in [0, S), sorted by (right, left)."""
    s = seg.tolist()
    H, W = len(s), len(s[0])
    pairs = set()
    for y in range(H):
        for x in range(W):
            a = s[y][x]
            if not 0 <= a < S:
                continue
            if x + 1 < W:
                b = s[y][x + 1]
                if b != a and 0 <= b < S:
                    pairs.add((a, b))
            if y + 1 < H:
                b = s[y + 1][x]
                if b != a and 0 <= b < S:
                    pairs.add((a, b))
    return torch.tensor(sorted(pairs, key=lambda p: (p[1], p[0])), dtype=torch.int64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _edges_oracle(kind, H, W, S):
    return OS.adjacency_list(_graph_map(kind, H, W, S)[0][None, None])


def _centers_f64(seg, S):
    """OS.centers restated for maps that carry -1 and ids >= S: fp64 coordinate sums / fp64 counts, rounded once to fp32."""
    H, W = seg.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    flat = seg.reshape(-1)
    keep = (flat >= 0) & (flat < S)
    ids = flat[keep]
    cnt = torch.zeros(S, dtype=torch.float64).index_add_(0, ids, torch.ones(ids.numel(), dtype=torch.float64))
    sx = torch.zeros(S, dtype=torch.float64).index_add_(0, ids, xs.reshape(-1)[keep].double())
    sy = torch.zeros(S, dtype=torch.float64).index_add_(0, ids, ys.reshape(-1)[keep].double())
    return torch.stack([sx / cnt, sy / cnt], dim=1).float()


def _assert_same_with_nan(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)), (what, (got - want).nan_to_num().abs().max())


# ------------------------------------------------------------------------------------------- adjacency
@pytest.mark.parametrize("kind,H,W,S", GRAPH_MAPS, ids=GRAPH_IDS)
def test_adjacency_matches_oracle_beyond_one_byte_per_thread(dev, kind, H, W, S):
    seg, n_seg = _graph_map(kind, H, W, S)
    want = _edges_oracle(kind, H, W, S)
    assert want.shape[0] > n_seg  # (a map whose graph is worth compacting)
    d = seg.to(dev)
    got = ops.seg_adjacency(d, n_seg).cpu()
    assert got.shape == want.shape and torch.equal(got, want)
    # trailing ids that never occur: the key stride changes from max + 1 to n_seg, the edges and their order must not
    got = ops.seg_adjacency(d, n_seg + 7).cpu()
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("kind,H,W,S", GRAPH_MAPS, ids=GRAPH_IDS)
def test_adjacency_ignores_unlabelled_and_out_of_range_pixels(dev, kind, H, W, S):
    seg, n_seg = _graph_map_holed(kind, H, W, S)
    want = _edges_bruteforce(seg, n_seg)
    assert want.shape[0] > n_seg
    got = ops.seg_adjacency(seg.to(dev), n_seg).cpu()
    assert got.shape == want.shape and torch.equal(got, want)


def test_adjacency_truncates_at_max_edges_and_still_counts_every_edge(dev):
    kind, H, W, S = GRAPH_MAPS[1]
    seg, n_seg = _graph_map(kind, H, W, S)
    want = _edges_oracle(kind, H, W, S)
    E = want.shape[0]
    max_edges, guard, sentinel = E - 5, 16, -7
    edges = torch.full((max_edges + guard, 2), sentinel, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    bitmap = torch.empty(n_seg * n_seg, dtype=torch.uint8, device=dev)
    d = seg.to(torch.int32).to(dev).contiguous()
    rc = lib().wvn_seg_adjacency(ptr(d), ptr(edges), ptr(count), ptr(bitmap), H, W, n_seg, max_edges, stream())
    assert rc == 0
    assert int(count.item()) == E
    edges = edges.cpu()
    assert torch.equal(edges[:max_edges], want[:max_edges])
    assert torch.equal(edges[max_edges:], torch.full((guard, 2), sentinel, dtype=torch.int64))


# --------------------------------------------------------------------------------------------- centres
@pytest.mark.parametrize("kind,H,W,S", GRAPH_MAPS, ids=GRAPH_IDS)
def test_centers_equal_oracle_bit_for_bit(dev, kind, H, W, S):
    """Integer coordinate sums, one fp64 quotient, one rounding to fp32: the same value as the oracle's, not a close one."""
    seg, n_seg = _graph_map(kind, H, W, S)
    want = OS.centers(seg[None, None])
    _assert_same_with_nan(ops.seg_centers(seg.to(dev), n_seg).cpu(), want, "plain")
    # an id without pixels (NaN row) and trailing ids that never occur (NaN rows)
    holed = seg.clone()
    holed[holed == 3] = 0
    want = torch.cat([OS.centers(holed[None, None]), torch.full((n_seg + 7 - int(holed.max()) - 1, 2), NAN)])
    assert bool(torch.isnan(want[3]).all())
    _assert_same_with_nan(ops.seg_centers(holed.to(dev), n_seg + 7).cpu(), want, "empty id + trailing ids")
    # -1 pixels and ids >= n_seg contribute to no centre
    holed, n_seg = _graph_map_holed(kind, H, W, S)
    _assert_same_with_nan(ops.seg_centers(holed.to(dev), n_seg).cpu(), _centers_f64(holed, n_seg), "-1 band")


# --------------------------------------------------------------------------------------- label pooling
# signal tolerance: the per-pixel channel mean is the same fp32 expression on both sides; the 2^-32 fixed-point sum adds at most 2^-33
# per pixel to the mean; what remains is one fp32 rounding of a value <= 1 on each side: 2 * 2^-24 = 1.2e-7
LABEL_ATOL = 2e-7


def _label_node(C, H, W, S, seed):
    """-> (mask [C,H,W] with NaN, seg [H,W] int64 with -1 / >= S planted, want_signal [S], want_valid [S], (nan ids, zero id))."""
    gg = g(seed)
    seg = _blobs(H, W, S, seed + 1)
    mask = torch.rand(C, H, W, generator=gg)
    mask[torch.rand(C, H, W, generator=gg) < 0.5] = NAN
    mask[:, torch.rand(H, W, generator=gg) < 0.1] = NAN
    present = torch.unique(seg).tolist()
    nan_ids, zero_id = (present[1], present[len(present) // 2]), present[-2]
    for i in nan_ids:
        mask[:, seg == i] = NAN
    mask[:, seg == zero_id] = 0.0
    drop = torch.rand(H, W, generator=gg)
    seg = seg.clone()
    seg[drop < 0.02] = -1
    seg[(drop >= 0.02) & (drop < 0.04)] = S + 2
    seg[0, 0] = 1 << 30
    bad = (seg < 0) | (seg >= S)
    for i in nan_ids + (zero_id,):
        assert bool((seg == i).any())
    mask_o, seg_o = mask.clone(), seg.clone()
    mask_o[:, bad] = NAN
    seg_o[bad] = 0
    sig, valid = OS.update_supervision_signal(mask_o, seg_o)
    pad = S - sig.shape[0]
    return mask, seg, torch.cat([sig, torch.zeros(pad)]), torch.cat([valid, torch.zeros(pad, dtype=torch.bool)]), (nan_ids, zero_id)


def _check_label_node(sig, valid, node, what):
    _, _, want_sig, want_valid, (nan_ids, zero_id) = node
    sig, valid = sig.cpu(), valid.cpu()
    err = (sig - want_sig).abs().max().item()
    print(f"label_pool {what}: max|signal - oracle| = {err:.3e} (bound {LABEL_ATOL})")
    assert torch.equal(valid, want_valid), what
    assert err <= LABEL_ATOL, (what, err)
    for i in nan_ids:
        assert sig[i].item() == 0.0 and not bool(valid[i]), (what, i)
    assert not bool(valid[zero_id]), what
    assert 0.3 < want_valid.float().mean().item()  # (the case is not degenerate)


@pytest.mark.parametrize("C,H,W,S", [(3, 224, 224, 100), (1, 96, 160, 37), (3, 100, 100, 300)])
def test_label_pool_matches_oracle(dev, C, H, W, S):
    node = _label_node(C, H, W, S, 7 * S + C)
    sig, valid = ops.label_pool(node[0].to(dev), node[1].to(dev), S)
    _check_label_node(sig, valid, node, f"C={C} {H}x{W} S={S}")


def test_label_pool_batched_matches_oracle_per_node(dev):
    C, H, W = 3, 96, 160
    n_segs = [37, 5, 100, 64]
    nodes = [_label_node(C, H, W, S, 900 + 13 * i) for i, S in enumerate(n_segs)]
    masks = [n[0].to(dev).contiguous() for n in nodes]
    segs = [n[1].to(torch.int32).to(dev).contiguous() for n in nodes]
    out = ops.label_pool_batched(masks, segs, n_segs)
    for i, (sig, valid) in enumerate(out):
        assert sig.shape == (n_segs[i],) and valid.shape == (n_segs[i],)
        _check_label_node(sig, valid, nodes[i], f"batched node {i} S={n_segs[i]}")


# --------------------------------------------------------------------------------------- fused pooling
SEGPOOL_ATOL = 2e-5   # the project's bound for randn tokens (tests/test_gpu_kernels.py)
BAND_LDS_LIMIT = 48 * 1024


def _band_lds(G, S):
    return 2 * S * G * 8 + 4 * S


@functools.lru_cache(maxsize=None)
def _tokens(G, D):
    return torch.randn(2, G * G, D, generator=g(1000 * G + D))


@functools.lru_cache(maxsize=None)
def _dense(G, H, D):
    tok = _tokens(G, D)
    return OI.upsample_bilinear_ac(tok.reshape(2, G, G, D).permute(0, 3, 1, 2), H)


@functools.lru_cache(maxsize=None)
def _pool_frames(H, n_ids, kind):
    """[2,H,H] int64 maps with ids in [0, n_ids), -1 pixels and ids far beyond any S of the cases planted."""
    if kind == "stripes":   # every segment is whole image rows
        rows = (torch.arange(H) * n_ids) // H
        seg = torch.stack([rows[:, None].expand(H, H), (n_ids - 1 - rows)[:, None].expand(H, H)]).clone()
    else:
        seg = torch.stack([_blobs(H, H, n_ids, 40 + b) for b in range(2)])
    if n_ids > 4:
        seg[1][seg[1] == 3] = 0   # an id without pixels -> NaN row
    seg[0, H // 3, :] = -1
    seg[1, :, H // 2] = -1
    seg[0, H - 1, 1:H // 2] = 1000
    seg[1, 0, 0] = 1 << 30
    drop = torch.rand(2, H, H, generator=g(41))
    seg[drop < 0.01] = -1
    seg[(drop >= 0.01) & (drop < 0.02)] = 1000
    return seg


def _pool_want(G, H, S, D, seg):
    dense = _dense(G, H, D)
    want, cnt = [], []
    for b in range(seg.shape[0]):
        sg = seg[b].clone()
        sg[(sg < 0) | (sg >= S)] = -1
        sp = OS.sparsify_features(dense[b:b + 1], sg)
        want.append(torch.cat([sp, torch.full((S - sp.shape[0], D), NAN)]))
        cnt.append(torch.bincount(sg[sg >= 0].reshape(-1), minlength=S))
    return torch.stack(want), torch.stack(cnt)


def _check_pool(got, cnt, want, want_cnt, what):
    got = got.cpu()
    err = (got - want).nan_to_num().abs().max().item()
    print(f"segpool {what}: max|err| = {err:.3e} (bound {SEGPOOL_ATOL})")
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    assert not bool(torch.isnan(want).all(-1).all())
    assert torch.allclose(got, want, atol=SEGPOOL_ATOL, rtol=0, equal_nan=True), (what, err)
    if cnt is not None:
        assert torch.equal(cnt.cpu().long(), want_cnt), what


# (G, H, S, D, ids drawn from [0, n_ids), map kind, band kernel?)
SEGPOOL_CASES = [
    (14, 224, 100, 24, 100, "blobs", True),     # ViT/16 grid
    (32, 448, 90, 16, 90, "blobs", True),       # DINOv2/14 grid, 2*S*G*8 + 4*S = 46 440 <= 48 K
    (32, 448, 100, 16, 90, "blobs", False),     # the same frames past the limit: 51 600 > 48 K
    (14, 100, 33, 65, 33, "blobs", True),       # non-integer ratio, W % 64 != 0, D one past a wave
    (7, 50, 3, 1, 3, "blobs", True),            # D = 1
    (56, 448, 100, 8, 100, "stripes", False),   # runs of whole image rows: every wave boundary lies inside a run
    (14, 100, 220, 5, 220, "blobs", False),     # per-pixel kernel with W % 64 != 0: waves straddle image rows
]


@pytest.mark.parametrize("G,H,S,D,n_ids,kind,band", SEGPOOL_CASES, ids=[f"G{c[0]}-H{c[1]}-S{c[2]}-D{c[3]}-{c[5]}" for c in SEGPOOL_CASES])
def test_segpool_bilinear_mean_matches_oracle(dev, G, H, S, D, n_ids, kind, band):
    assert (_band_lds(G, S) <= BAND_LDS_LIMIT) == band   # the case sits on the side of the kernel switch it is meant for
    seg = _pool_frames(H, n_ids, kind)
    want, want_cnt = _pool_want(G, H, S, D, seg)
    got, cnt = ops.segpool_bilinear_mean(seg.to(dev), _tokens(G, D).to(dev), G, S, return_counts=True)
    _check_pool(got, cnt.reshape(2, S), want, want_cnt, f"G={G} H={H} S={S} D={D} {kind}")


def test_segpool_reads_strided_tokens_and_never_the_padding(dev):
    G, H, S, D, pad = 14, 224, 100, 24, 8
    seg = _pool_frames(H, S, "blobs")
    want, want_cnt = _pool_want(G, H, S, D, seg)
    buf = torch.full((2, G * G, D + pad), NAN)
    buf[:, :, :D] = _tokens(G, D)
    buf = buf.to(dev)
    d_seg = seg.to(torch.int32).to(dev).contiguous()
    feat = torch.empty(2, S, D, dtype=torch.float32, device=dev)
    wbuf = torch.empty(2 * S * G * G, dtype=torch.int64, device=dev)
    cnt = torch.empty(2 * S, dtype=torch.int32, device=dev)
    rc = lib().wvn_segpool_bilinear_mean(ptr(d_seg), ptr(buf), D + pad, ptr(feat), ptr(wbuf), ptr(cnt), 2, H, H, G, S, D, stream())
    assert rc == 0
    nonempty = want_cnt > 0
    assert not bool(torch.isnan(feat.cpu()[nonempty]).any())
    _check_pool(feat, cnt.reshape(2, S), want, want_cnt, "ld = D + 8")


def test_segpool_channel_limit(dev):
    """D = 1024 (one channel per thread of the largest workgroup) is served; D = 1025 is refused."""
    G, H, S, D = 4, 16, 2, 1024
    seg = (torch.rand(2, H, H, generator=g(3)) < 0.4).long()
    seg[0, 2, :] = -1
    seg[1, :, 5] = 7
    seg[1][seg[1] == 1] = 0
    want, want_cnt = _pool_want(G, H, S, D, seg)
    got, cnt = ops.segpool_bilinear_mean(seg.to(dev), _tokens(G, D).to(dev), G, S, return_counts=True)
    _check_pool(got, cnt.reshape(2, S), want, want_cnt, "D = 1024")
    D = 1025
    tok = torch.zeros(2, G * G, D, device=dev)
    d_seg = seg.to(torch.int32).to(dev).contiguous()
    feat = torch.empty(2, S, D, dtype=torch.float32, device=dev)
    wbuf = torch.empty(2 * S * G * G, dtype=torch.int64, device=dev)
    cnt = torch.empty(2 * S, dtype=torch.int32, device=dev)
    rc = lib().wvn_segpool_bilinear_mean(ptr(d_seg), ptr(tok), D, ptr(feat), ptr(wbuf), ptr(cnt), 2, H, H, G, S, D, stream())
    assert rc == WVN_ERR_ARG


@pytest.mark.parametrize("H,W", [(64, 96), (96, 64)])
def test_segpool_rejects_non_square_frames(dev, H, W):
    """Both axes use the tap scale (G-1)/(H-1): a frame with W > H would index past its row of the weight table."""
    G, S, D = 8, 4, 8
    seg = torch.zeros(1, H, W, dtype=torch.int32, device=dev)
    tok = torch.zeros(1, G * G, D, device=dev)
    with pytest.raises(_lib.WvnError, match="square frames only"):
        ops.segpool_bilinear_mean(seg, tok, G, S)
    feat = torch.full((1, S, D), 5.0, device=dev)
    wbuf = torch.full((S * G * G,), 5, dtype=torch.int64, device=dev)
    cnt = torch.full((S,), 5, dtype=torch.int32, device=dev)
    rc = lib().wvn_segpool_bilinear_mean(ptr(seg), ptr(tok), D, ptr(feat), ptr(wbuf), ptr(cnt), 1, H, W, G, S, D, stream())
    assert rc == WVN_ERR_ARG
    torch.cuda.synchronize()
    assert bool((feat == 5).all()) and bool((wbuf == 5).all()) and bool((cnt == 5).all())  # refused before any memset or launch
