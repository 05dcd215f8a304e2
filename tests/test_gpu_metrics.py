"""The metric kernels (csrc/metrics.hip) against tests/metrics_ref.py on the GPU.

Everything integer -- histograms, confusion matrices, counters, per-segment counts, U2, P, N -- is held BIT-IDENTICAL to the
reference.  So are the fp64 results: tpr / fpr are single IEEE divisions of exactly converted integers, the binned AUROC is a
fixed-order sum of separately rounded operations (the unit is compiled without contraction), the exact AUROC one division."""
import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_ref as MR
from wild_visual_navigation_amd import ops
from wild_visual_navigation_amd.ops import PerSegment
from wild_visual_navigation_amd.utils import BinaryAccuracy, BinaryAUROC, BinaryROC, MetricLogger, Data

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return PerSegment(torch.from_numpy(x[1]).to(dev)) if isinstance(x, tuple) else torch.from_numpy(x).to(dev)


def _run(dev, T, scores, targets, seg=None, S=None, seg_off=None, tau=0.5, ignore_index=None, rows=None, state=None, ref=True):
    """One fused pass on the GPU and in the reference -> (gpu state, gpu counts, ref states, ref counts)."""
    th = MR.thresholds(T)
    n = len(scores) * len(targets)
    if state is None:
        state = (ops.metric_state(n, T, dev), [MR.empty_state(T) for _ in range(n)])
    gst, rst = state
    cnt = None
    if seg is not None and rows is not None:
        cnt = torch.zeros(rows, len(targets), 2, dtype=torch.int32, device=dev)
    ops.metric_accumulate(gst, torch.from_numpy(th).to(dev), [_t(s, dev) for s in scores], [_t(t, dev) for t in targets],
                          seg=None if seg is None else torch.from_numpy(seg).to(dev),
                          seg_off=None if seg_off is None else torch.from_numpy(seg_off).to(dev), tau=tau, ignore_index=ignore_index,
                          seg_counts=cnt)
    rcnt = None
    if ref:
        rcnt = MC.ref_accumulate(rst, th, scores, targets, seg=seg, S=S, seg_off=seg_off, tau=tau, ignore_index=ignore_index, rows=rows)
    return (gst, rst), cnt, rcnt


def _assert_states(state):
    gst, rst = state
    got = gst.cpu().numpy()
    for i, r in enumerate(rst):
        want = MC.pack(r)
        assert np.array_equal(got[i, :len(want)], want), f"pair {i}: {np.flatnonzero(got[i, :len(want)] != want)[:8]}"


def _edge_scores(T):
    th = MR.thresholds(T)
    v = np.concatenate([th, np.nextafter(th, np.float32(2)), np.nextafter(th, np.float32(-1))]).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, -1e-30, -3.0, 1.0000001, 7.5, 1.0, np.nan], np.float32)
    return v, special


@pytest.mark.parametrize("T", [5000, 2])
def test_threshold_edges(dev, T):
    v5000, special = _edge_scores(5000)
    assert v5000.shape == (15000,)
    maps = [v5000.reshape(1, 1, 15000)] if T == 5000 else [v5000.reshape(1, 1, 15000), np.resize(_edge_scores(2)[0], 15000).reshape(1, 1, 15000)]
    state = None
    for m in maps:
        tgt = (np.arange(m.size) % 2).astype(np.uint8).reshape(m.shape)
        state, _, _ = _run(dev, T, [m], [tgt], state=state)
    state, _, _ = _run(dev, T, [special], [(np.arange(special.size) % 2).astype(np.uint8)], state=state)
    _assert_states(state)
    r = state[1][0]
    assert r["n_nan"] == 2 and r["n_out_of_range"] >= 5 and r["hist"][0].sum() > 0 and r["hist"][T].sum() > 0


def test_contention_and_counter_width(dev):
    """70 225 pixels (> 65 535) in ONE counter, then split over two bins and both classes."""
    n = 265
    one = np.full((1, n, n), 0.3, np.float32)
    state, _, _ = _run(dev, 5000, [one], [np.ones((1, n, n), np.uint8)])
    _assert_states(state)
    assert state[1][0]["hist"].max() == n * n
    two = one.copy()
    two.reshape(-1)[1::2] = 0.7
    tgt = (np.arange(n * n) % 3 == 0).astype(np.uint8).reshape(1, n, n)
    state, _, _ = _run(dev, 5000, [one, two], [np.ones((1, n, n), np.uint8), tgt])
    _assert_states(state)


def _ragged(seed, B=3, H=37, W=53, S=11):
    g = np.random.default_rng(seed)
    seg = g.integers(-1, S + 1, (B, H, W)).astype(np.int32)                # -1 and S occur: skipped
    seg[seg == 4] = 5                                                       # id 4 never occurs
    tab = (np.round(g.random((B, S)) * 64) / 64).astype(np.float32)
    tab[1, 2] = np.nan
    dense = g.random((B, H, W)).astype(np.float32) * 1.2 - 0.1              # some scores outside [0, 1]
    dense[0, 1, :] = np.nan
    ytab = g.integers(0, 2, (B, S)).astype(np.float32)
    ytab[2, 1], ytab[0, 3] = 2.0, np.nan
    return seg, tab, dense, ytab, g


@pytest.mark.parametrize("kind,T,ignore_index", [("u8", 5000, None), ("i32", 5000, 1), ("f32", 5000, None), ("f32", 8192, 0), ("u8", 37, 255)])
def test_ragged_geometry_two_scores_two_targets(dev, kind, T, ignore_index):
    B, H, W, S = 3, 37, 53, 11
    seg, tab, dense, ytab, g = _ragged(11)
    if kind == "u8":
        tgt = g.integers(0, 2, (B, H, W)).astype(np.uint8)
        tgt[0, 1, :7] = 255
    elif kind == "i32":
        tgt = g.integers(-1, 3, (B, H, W)).astype(np.int32)
    else:
        tgt = g.integers(0, 2, (B, H, W)).astype(np.float32)
        tgt[0, 0, :6] = [0.7, 2.0, np.nan, 1.9, -0.5, -1.0]                 # 0, ignored, ignored, 1, 0, ignored
    state, cnt, rcnt = _run(dev, T, [("seg", tab), dense], [tgt, ("seg", ytab)], seg=seg, S=S, tau=0.4, ignore_index=ignore_index, rows=B * S)
    _assert_states(state)
    assert np.array_equal(cnt.cpu().numpy(), rcnt)
    assert rcnt[4].sum() == 0 and rcnt.sum() > 0                            # the id that never occurs stays zero
    for r in state[1]:
        assert r["hist"].sum() + r["n_nan"] + r["n_ignored"] == B * H * W and r["n_ignored"] > 0
    assert state[1][0]["n_nan"] > 0 and state[1][2]["n_nan"] > 0 and state[1][2]["n_out_of_range"] > 0
    # dense sources only: the segment ids skip nothing, the counts are still taken
    state, cnt, rcnt = _run(dev, T, [dense], [tgt], seg=seg, S=S, rows=B * S, ignore_index=ignore_index)
    _assert_states(state)
    assert np.array_equal(cnt.cpu().numpy(), rcnt)


@pytest.mark.parametrize("T,n_targets", [(2, 1), (5000, 2)])
def test_segment_counts_beyond_the_lds_window(dev, T, n_targets):
    """The counting slice keeps a window of rows in LDS (4096 rows at T = 2 with one target, 5005 at T = 5000 with two) and adds the
    others to global memory directly: more segments than the window, ids all over the range."""
    g = np.random.default_rng(51)
    B, H, W, S = 2, 64, 64, 6000
    seg = g.integers(0, S, (B, H, W)).astype(np.int32)
    seg[0, :8] = 4095 + g.integers(0, 3, (8, W))                            # around the window's edge
    tab = g.random((B, S)).astype(np.float32)
    tgts = [g.integers(0, 2, (B, H, W)).astype(np.uint8), g.integers(0, 3, (B, H, W)).astype(np.int32)][:n_targets]
    state, cnt, rcnt = _run(dev, T, [("seg", tab)], tgts, seg=seg, S=S, rows=B * S)
    _assert_states(state)
    assert np.array_equal(cnt.cpu().numpy(), rcnt) and rcnt[S + 4096:].sum() > 0


@pytest.mark.parametrize("view", ["sliced", "transposed", "expanded", "int64", "int64_sliced"])
def test_segment_maps_that_are_views_or_int64(dev, view):
    """A seg that is no contiguous int32 tensor -- a strided slice, a transposed view, one map expanded over the batch, int64 ids
    (read by the kernel as they are) -- gives what its VALUES say."""
    g = np.random.default_rng(61)
    B, H, W, S = 3, 19, 23, 7
    big = torch.from_numpy(g.integers(-1, S + 1, (B, 2 * H, 2 * W)).astype(np.int32)).to(dev)
    if view == "sliced":
        seg = big[:, ::2, ::2]
    elif view == "transposed":
        seg = big[:, :W, :H].transpose(1, 2)
    elif view == "expanded":
        seg = big[:1, :H, :W].expand(B, H, W)
    elif view == "int64":
        seg = big[:, :H, :W].long()
    else:
        seg = big.long()[:, 1::2, ::2]
    assert tuple(seg.shape) == (B, H, W) and (seg.dtype == torch.int64 or not seg.is_contiguous())
    tab = g.random((B, S)).astype(np.float32)
    tgt = g.integers(0, 2, (B, H, W)).astype(np.uint8)
    th = MR.thresholds(5000)
    gst = ops.metric_state(1, 5000, dev)
    cnt = torch.zeros(B * S, 1, 2, dtype=torch.int32, device=dev)
    ops.metric_accumulate(gst, torch.from_numpy(th).to(dev), [PerSegment(torch.from_numpy(tab).to(dev))], [torch.from_numpy(tgt).to(dev)],
                          seg=seg, seg_counts=cnt)
    rst = [MR.empty_state(5000)]
    rcnt = MC.ref_accumulate(rst, th, [("seg", tab)], [tgt], seg=seg.cpu().numpy(), S=S, rows=B * S)
    _assert_states((gst, rst))
    assert np.array_equal(cnt.cpu().numpy(), rcnt) and rst[0]["n_ignored"] > 0


def test_ragged_tables_must_agree_in_their_rows(dev):
    graph, res, conf = MC.make_batch(3)
    N = graph.y.numel()
    th = torch.from_numpy(MR.thresholds(16)).to(dev)
    gst = ops.metric_state(1, 16, dev)
    kw = dict(seg=graph.seg.to(dev), seg_off=graph.ptr.to(dev))
    with pytest.raises(ops._lib.WvnError, match="rows"):
        ops.metric_accumulate(gst, th, [PerSegment(res[:-1].to(dev))], [PerSegment(graph.y.to(dev))], **kw)
    with pytest.raises(ops._lib.WvnError, match="rows"):
        ops.metric_accumulate(gst, th, [PerSegment(res.to(dev))], [graph.label.to(dev)],
                              seg_counts=torch.zeros(N + 1, 1, 2, dtype=torch.int32, device=dev), **kw)
    assert gst.sum().item() == 0


def test_ragged_graph_offsets_and_strided_table(dev):
    graph, res, conf = MC.make_batch(3)
    seg, off = graph.seg.numpy().astype(np.int32), graph.ptr.numpy()
    seg[0, 0, :3] = [-1, 99, int(off[1] - off[0])]
    N = int(off[-1])
    th = torch.from_numpy(MR.thresholds(5000)).to(dev)
    gst = ops.metric_state(2, 5000, dev)
    cnt = torch.zeros(N, 2, 2, dtype=torch.int32, device=dev)
    r = res.to(dev)
    ops.metric_accumulate(gst, th, [PerSegment(r)], [graph.label.to(dev), PerSegment(graph.y.to(dev))], seg=torch.from_numpy(seg).to(dev),
                          seg_off=graph.ptr.to(dev), seg_counts=cnt)
    rst = [MR.empty_state(5000) for _ in range(2)]
    rcnt = MC.ref_accumulate(rst, MR.thresholds(5000), [("seg", res[:, 0].numpy())], [graph.label.numpy(), ("seg", graph.y.numpy())],
                             seg=seg, seg_off=off, rows=N)
    _assert_states((gst, rst))
    assert np.array_equal(cnt.cpu().numpy(), rcnt) and rst[0]["n_ignored"] == 3


def test_accumulation_is_additive_and_reproducible(dev):
    """Three updates = one update of the concatenation; the same call twice gives the same bytes; more pixels than one sweep of the
    grid (5 x 512 x 512 > 512 workgroups x 512 threads x 4)."""
    g = np.random.default_rng(21)
    B, H, W = 5, 512, 512
    p = (g.random((B, H, W)) ** 2).astype(np.float32)
    p[:, 100:300, 50:400] = 0.25                                             # a region in one bin
    tgt = (g.random((B, H, W)) < 0.3).astype(np.uint8)
    whole, _, _ = _run(dev, 5000, [p], [tgt])
    _assert_states(whole)
    again, _, _ = _run(dev, 5000, [p], [tgt], ref=False)
    assert torch.equal(whole[0], again[0])
    parts = None
    for lo, hi in ((0, 1), (1, 4), (4, 5)):
        parts, _, _ = _run(dev, 5000, [p[lo:hi]], [tgt[lo:hi]], state=parts, ref=False)
    assert torch.equal(whole[0], parts[0])


def test_classes_on_gpu_and_reset(dev):
    g = np.random.default_rng(22)
    p = g.random(4097).astype(np.float32)
    y = (g.random(4097) < 0.2 + 0.5 * p).astype(np.float32)
    th = MR.thresholds(5000)
    want = MR.accumulate(MR.empty_state(5000), p, MR.target_class(y), th, 0.3)
    fpr, tpr, thr, P, N = MR.roc(want["hist"], th)
    roc, au, acc = BinaryROC(5000), BinaryAUROC(5000), BinaryAccuracy(0.3)
    for rep in range(2):                                                      # the states survive reset: the second epoch equals the first
        for m in (roc, au, acc):
            m.update(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev))
        got = roc.compute()
        assert all(t.is_cuda and t.dtype == torch.float64 for t in got)
        for a, b in zip(got, (fpr, tpr, thr)):
            assert np.array_equal(a.cpu().numpy(), b)
        assert au.compute().item() == MR.auroc_binned(fpr, tpr, P, N)[0]
        assert acc.compute().item() == MR.accuracy(want["cm"])
        assert np.array_equal(acc.confusion_matrix().cpu().numpy(), want["cm"])
        for m in (roc, au, acc):
            m.reset()
        assert roc.acc.state.sum().item() == 0
    with pytest.raises(ValueError, match="out of scope"):
        BinaryAUROC().update(torch.rand(1, 4, 4, device=dev), torch.zeros(1, 4, 4, device=dev))


def _weighted(dev, score, pos, neg):
    scal, cnt = ops.metric_auroc_weighted(torch.from_numpy(np.asarray(score, np.float32)).to(dev), torch.from_numpy(np.asarray(pos, np.int64)).to(dev),
                                          torch.from_numpy(np.asarray(neg, np.int64)).to(dev))
    want = MR.auroc_exact(score, pos, neg)
    got = (scal[0].item(), bool(cnt[3].item()), cnt[0].item(), cnt[1].item(), cnt[2].item())
    assert got == want, (got, want)
    return got


def test_exact_auroc_cases(dev):
    g = np.random.default_rng(31)
    assert _weighted(dev, [0.5] * 40, g.integers(1, 9, 40), g.integers(1, 9, 40))[0] == 0.5            # all tied
    assert _weighted(dev, [0.9, 0.8, 0.2, 0.1], [3, 5, 0, 0], [0, 0, 7, 2])[0] == 1.0                  # perfectly separated
    assert _weighted(dev, [0.3], [4], [6])[0] == 0.5                                                     # E = 1
    assert _weighted(dev, [0.3, 0.6], [4, 1], [0, 0])[:2] == (0.0, True)                                # no negatives
    assert _weighted(dev, [0.3, 0.6], [0, 0], [4, 1])[:2] == (0.0, True)                                # no positives
    _weighted(dev, [0.2, np.nan, 0.7, 0.2, np.nan], [1, 50, 2, 3, 0], [4, 60, 0, 1, 9])                 # NaN entries count nothing
    score = (np.round(g.random(100000) * 3000) / 3000).astype(np.float32)                               # ties across the rounds of the kernel
    pos, neg = g.integers(0, 3000, 100000), g.integers(0, 3000, 100000)
    pos[::5] = 0
    _weighted(dev, score, pos, neg)
    _weighted(dev, g.random(4097).astype(np.float32), g.integers(0, 2, 4097), g.integers(0, 2, 4097))   # one entry past a round


def test_exact_auroc_per_segment_ties_across_frames_and_empty_segments(dev):
    seg, tab, dense, ytab, g = _ragged(12)
    B, H, W, S = 3, 37, 53, 11
    tab[1, 2] = 0.5
    tab[:, 7] = 0.25                                                          # equal scores in different frames: one group
    label = g.integers(0, 2, (B, H, W)).astype(np.uint8)
    m = BinaryAUROC()
    m.update(torch.from_numpy(tab).to(dev), torch.from_numpy(label).to(dev), seg=torch.from_numpy(seg).to(dev))
    row, valid = MR.segment_rows(seg, S=S)
    cnt = MR.segment_counts(MR.target_class(label), row, valid, B * S)
    assert cnt[4].sum() == 0                                                  # the empty segment's entry: contributes nothing
    want = MR.auroc_exact(tab.ravel(), cnt[:, 1], cnt[:, 0])
    keep = np.arange(B * S) % S != 4
    assert want[0] == MR.auroc_exact(tab.ravel()[keep], cnt[keep, 1], cnt[keep, 0])[0]
    assert m.compute().is_cuda and m.compute().item() == want[0] and m.degenerate().item() == 0


@pytest.mark.parametrize("T", [5000, 2, 8192])
def test_curve_kernel(dev, T):
    g = np.random.default_rng(41)
    th = MR.thresholds(T)
    p = g.random(30000).astype(np.float32)
    for name, y in (("mixed", (g.random(30000) < p).astype(np.uint8)), ("P=0", np.zeros(30000, np.uint8)), ("N=0", np.ones(30000, np.uint8))):
        st = MR.accumulate(MR.empty_state(T), p, y, th)
        fpr, tpr, thr, scal, cnt = ops.metric_curve(torch.from_numpy(MC.pack(st)).to(dev), torch.from_numpy(th).to(dev))
        wf, wt, wth, P, N = MR.roc(st["hist"], th)
        for a, b in zip((fpr, tpr, thr), (wf, wt, wth)):
            assert np.array_equal(a.cpu().numpy(), b), name
        auroc, degenerate = MR.auroc_binned(wf, wt, P, N)
        assert scal.tolist() == [auroc, MR.accuracy(st["cm"])], name
        assert cnt.tolist() == [P, N, int(degenerate)] and degenerate == (name != "mixed")
    empty = ops.metric_curve(ops.metric_state(1, T, dev)[0], torch.from_numpy(th).to(dev))
    assert empty[3].tolist() == [0.0, 0.0] and empty[4].tolist() == [0, 0, 1]


@pytest.mark.parametrize("log_roc_image", [False, True])
def test_metric_logger_end_to_end(dev, log_roc_image):
    ml = MetricLogger(None, log_roc_image)
    ex = MC.Expected()
    for seed in (0, 1):
        graph, res, conf = MC.make_batch(seed)
        gd = MC.graph_to(graph, dev)
        ml.log_image(gd, res.to(dev), "test", threshold=0.45)
        ml.log_confidence(gd, res.to(dev), conf.to(dev), "test")
        ex.log_image(graph, res, 0.45)
        ex.log_confidence(graph, conf)
        nodes = Data(label=(torch.arange(graph.y.numel()) % 3 == 0), y=graph.y)
        ml.log_segment(Data(label=nodes.label.to(dev), y=nodes.y.to(dev)), res[:, 0].to(dev), "test")
        ex.log_segment(nodes, res[:, 0], nodes.label)
    MC.assert_results_equal(ml.get_epoch_results("test"), ex.results("test", log_roc_image))
    ml.reset("test")
    MC.assert_results_equal(ml.get_epoch_results("test"), MC.Expected().results("test", log_roc_image))


def test_log_maps_equals_log_image_of_the_same_data(dev):
    g = np.random.default_rng(7)
    B, S, H, W = 2, 7, 32, 32
    seg = torch.from_numpy(g.integers(0, S, (B, H, W))).to(dev)
    trav = torch.from_numpy((np.round(g.random((B, S)) * 16) / 16).astype(np.float32)).to(dev)
    conf = torch.from_numpy(g.random((B, S)).astype(np.float32)).to(dev)
    y = torch.from_numpy((g.random((B, S)) < 0.5).astype(np.float32)).to(dev)
    label = torch.from_numpy(g.random((B, H, W)) < 0.5).to(dev)
    graph = Data(label=label, seg=seg, ptr=torch.arange(B + 1) * S, y=y.reshape(-1))
    a, b, c = MetricLogger(), MetricLogger(), MetricLogger()
    a.log_image(graph, trav.reshape(-1, 1), "test")
    a.log_confidence(graph, None, conf.reshape(-1), "test")
    b.log_maps(trav, conf, label, self_label=y, seg=seg, mode="test")
    rows = (torch.arange(B, device=dev).view(B, 1, 1) * S + seg).reshape(-1)
    dense = [t.reshape(-1)[rows].view(B, H, W) for t in (trav, conf, y)]
    c.log_maps(dense[0], dense[1], label, self_label=dense[2], mode="test")
    ra, rb, rc = (m.get_epoch_results("test") for m in (a, b, c))
    MC.assert_results_equal(rb, ra)
    assert ra["test_auroc_binned_gt_image"] > 0
    for k, v in ra.items():
        if "auroc_binned" in k or "_acc_" in k:
            assert rc[k] == v, k
    assert rc["test_auroc_gt_image"] is None
