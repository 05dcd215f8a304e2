"""Evaluation metrics without a GPU: the definitions (tests/metrics_ref.py) against scikit-learn and brute force, the CPU route of
BinaryROC / BinaryAUROC / BinaryAccuracy and of MetricLogger against the definitions, the argument checks of the three C entry points.

Parity with the torchmetrics package is unpinned (the package is absent): metrics_ref.py restates its published behaviour."""
import ctypes as C

import numpy as np
import pytest
import sklearn.metrics as sk
import torch

import metrics_cases as MC
import metrics_ref as MR
from wild_visual_navigation_amd import _lib, ops
from wild_visual_navigation_amd.utils import BinaryAccuracy, BinaryAUROC, BinaryROC, MetricLogger, Data


def _scores(n, seed):
    g = np.random.default_rng(seed)
    p = g.random(n).astype(np.float32)
    y = (g.random(n) < 0.3 + 0.4 * p).astype(np.int64)
    return p, y


# ---- the definitions ----
def test_exact_auroc_equals_sklearn_weighted_with_ties():
    g = np.random.default_rng(0)
    E = 1000
    score = (np.round(g.random(E) * 50) / 50).astype(np.float32)          # 51 distinct values: many ties
    pos, neg = g.integers(0, 200, E), g.integers(0, 200, E)
    pos[::7] = 0
    neg[::11] = 0
    pos[::77] = neg[::77] = 0                                             # entries that contribute nothing
    got, degenerate, U2, P, N = MR.auroc_exact(score, pos, neg)
    y = np.concatenate([np.ones(E), np.zeros(E)])
    s = np.concatenate([score, score]).astype(np.float64)
    w = np.concatenate([pos, neg]).astype(np.float64)
    want = sk.roc_auc_score(y[w > 0], s[w > 0], sample_weight=w[w > 0])
    print("exact AUROC: |ref - sklearn| =", abs(got - want))
    assert not degenerate and P == pos.sum() and N == neg.sum()
    assert abs(got - want) <= 1e-12


def test_binned_auroc_equals_sklearn_auc_of_the_same_curve():
    p, y = _scores(20000, 1)
    th = MR.thresholds(5000)
    st = MR.accumulate(MR.empty_state(5000), p, y, th)
    fpr, tpr, thr, P, N = MR.roc(st["hist"], th)
    got, degenerate = MR.auroc_binned(fpr, tpr, P, N)
    want = sk.auc(fpr, tpr)
    print("binned AUROC: |ref - sklearn.auc| =", abs(got - want))
    assert not degenerate and abs(got - want) <= 1e-12                    # ~ T 2^-52 of accumulated rounding, with margin
    assert np.all(np.diff(fpr) >= 0) and thr[0] == 1.0 and thr[-1] == 0.0


def test_tps_fps_equal_brute_force_counts():
    g = np.random.default_rng(2)
    for T in (2, 37, 5000):
        th = MR.thresholds(T)
        n = 3000
        p = g.random(n).astype(np.float32)
        p[:T if T < n else n] = th[:n]                                     # scores exactly on thresholds
        p[-4:] = [-0.5, 1.5, -np.inf, np.inf]
        y = g.integers(0, 2, n)
        st = MR.accumulate(MR.empty_state(T), p, y, th)
        sfx = np.cumsum(st["hist"][::-1], axis=0)[::-1]
        for t in range(0, T, max(1, T // 200)):
            ge = p >= th[t]
            assert sfx[t + 1, 1] == int((ge & (y == 1)).sum()) and sfx[t + 1, 0] == int((ge & (y == 0)).sum())
        assert st["n_out_of_range"] == 4 and st["hist"].sum() == n


def test_bins_follow_the_table_not_the_formula():
    """floor(p (T - 1)) + 1 is only a first guess: k(p) is defined by fp32 comparisons against the torch.linspace table."""
    th = MR.thresholds(5000)
    p = np.random.default_rng(3).random(200000).astype(np.float32)
    k = MR.bin_of(p, th)
    assert np.all(th[np.maximum(k - 1, 0)] <= p) and np.all((k == 5000) | (th[np.minimum(k, 4999)] > p))
    assert (k != np.floor(p * np.float32(4999)).astype(np.int64) + 1).any()


def test_target_classes():
    t = np.array([0.0, 0.7, 1.0, 1.9, 2.0, -0.5, -1.0, np.nan, np.inf], np.float32)
    assert MR.target_class(t).tolist() == [0, 0, 1, 1, 2, 0, 2, 2, 2]
    assert MR.target_class(np.array([0, 1, 2, -1, 255], np.int32), ignore_index=1).tolist() == [0, 2, 2, 2, 2]
    assert MR.target_class(np.array([True, False])).tolist() == [1, 0]


# ---- the CPU route of the classes ----
def test_classes_on_cpu_equal_the_definitions():
    p, y = _scores(5000, 4)
    p[:5] = [np.nan, -0.25, 1.25, 0.5, 0.5]
    yt = y.astype(np.float32)
    yt[5:9] = [0.7, 2.0, np.nan, 1.0]
    th = MR.thresholds(5000)
    roc, au, acc = BinaryROC(5000), BinaryAUROC(5000), BinaryAccuracy(0.5)
    want = MR.empty_state(5000)
    for lo, hi in ((0, 1700), (1700, 1701), (1701, 5000)):                 # three updates
        for m in (roc, au, acc):
            m.update(torch.from_numpy(p[lo:hi]), torch.from_numpy(yt[lo:hi]))
        MR.accumulate(want, p[lo:hi], MR.target_class(yt[lo:hi]), th)
    fpr, tpr, thr, P, N = MR.roc(want["hist"], th)
    got = roc.compute()
    for a, b in zip(got, (fpr, tpr, thr)):
        assert a.dtype == torch.float64 and np.array_equal(a.numpy(), b)
    assert au.compute().item() == MR.auroc_binned(fpr, tpr, P, N)[0]
    assert acc.compute().item() == MR.accuracy(want["cm"])
    assert np.array_equal(acc.confusion_matrix().numpy(), want["cm"])
    assert roc.counters().tolist() == [want["n_nan"], want["n_ignored"], want["n_out_of_range"]] == [1, 2, 2]
    roc.reset()
    assert roc.acc.state.sum().item() == 0


def test_exact_auroc_class_on_cpu_per_segment_and_vectors():
    g = np.random.default_rng(5)
    B, S, H, W = 2, 6, 9, 11
    seg = g.integers(-1, S + 1, (B, H, W))                                  # -1 and S: skipped
    seg[seg == 3] = 2                                                       # id 3 never occurs
    preds = (np.round(g.random((B, S)) * 4) / 4).astype(np.float32)         # ties across frames
    label = g.integers(0, 2, (B, H, W)).astype(np.uint8)
    m = BinaryAUROC()
    m.update(torch.from_numpy(preds), torch.from_numpy(label), seg=torch.from_numpy(seg))
    row, valid = MR.segment_rows(seg, S=S)
    cnt = MR.segment_counts(MR.target_class(label), row, valid, B * S)
    assert cnt[3].sum() == 0 and cnt[S + 3].sum() == 0
    want = MR.auroc_exact(preds.ravel(), cnt[:, 1], cnt[:, 0])
    assert m.compute().item() == want[0] and m.degenerate().item() == 0
    v = BinaryAUROC()
    p, y = _scores(300, 6)
    p = np.round(p * 10) / 10
    v.update(torch.from_numpy(p), torch.from_numpy(y))
    assert v.compute().item() == MR.auroc_exact(p, y == 1, y == 0)[0]
    with pytest.raises(ValueError, match="out of scope"):
        BinaryAUROC().update(torch.rand(1, 4, 4), torch.zeros(1, 4, 4))


def test_degenerate_epochs_on_cpu():
    p = torch.tensor([0.2, 0.9, 0.4])
    for tgt, acc_want in ((torch.zeros(3), 2 / 3), (torch.ones(3), 1 / 3)):    # no positives / no negatives
        au, ex, ac, roc = BinaryAUROC(100), BinaryAUROC(), BinaryAccuracy(), BinaryROC(100)
        for m in (au, ex, ac, roc):
            m.update(p, tgt)
        assert au.compute().item() == 0.0 and au.degenerate().item() == 1
        assert ex.compute().item() == 0.0 and ex.degenerate().item() == 1
        assert ac.compute().item() == acc_want
        fpr, tpr, _ = roc.compute()
        assert (fpr if tgt.sum() > 0 else tpr).abs().sum().item() == 0.0
    for m in (BinaryAUROC(100), BinaryAUROC(), BinaryAccuracy()):               # nothing logged, and an empty update
        assert m.compute().item() == 0.0
        m.update(torch.zeros(0), torch.zeros(0))
        assert m.compute().item() == 0.0


# ---- MetricLogger on the CPU ----
@pytest.mark.parametrize("log_roc_image", [False, True])
def test_metric_logger_on_cpu_every_method_and_key(log_roc_image):
    logged = []
    ml = MetricLogger(lambda name, metric, **kw: logged.append((name, metric, kw)), log_roc_image)
    ex = MC.Expected()
    for seed, thr in ((0, 0.5), (1, 0.5)):
        graph, res, conf = MC.make_batch(seed)
        ml.log_image(graph, res, "val", threshold=thr)
        ml.log_confidence(graph, res, conf, "val")
        ex.log_image(graph, res, thr)
        ex.log_confidence(graph, conf)
        nodes = Data(label=(torch.arange(graph.y.numel()) % 3 == 0), y=graph.y)
        ml.log_segment(nodes, res[:, 0], "val")
        ex.log_segment(nodes, res[:, 0], nodes.label)
    got = ml.get_epoch_results("val")
    assert all(f"val_{k}" in got for k in MC.REFERENCE_KEYS)
    MC.assert_results_equal(got, ex.results("val", log_roc_image))
    names = {n for n, _, _ in logged}
    assert {"val_metric_auroc_gt_image", "val_metric_acc_self_image", "val_metric_auroc_anomaly_gt_image", "val_metric_auroc_gt_seg"} <= names
    by_name = {n: m for n, m, _ in logged}
    assert by_name["val_metric_auroc_gt_image"].compute().item() == got["val_auroc_gt_image"]
    assert all(kw == {"on_epoch": True, "on_step": False, "batch_size": kw["batch_size"]} for _, _, kw in logged)
    # the other modes are untouched; reset empties the mode
    MC.assert_results_equal(ml.get_epoch_results("test"), MC.Expected().results("test", log_roc_image))
    ml.reset("val")
    MC.assert_results_equal(ml.get_epoch_results("val"), MC.Expected().results("val", log_roc_image))
    with pytest.raises(ValueError):
        ml.reset("eval")


def test_log_maps_on_cpu_equals_log_image_of_the_same_data():
    g = np.random.default_rng(7)
    B, S, H, W = 2, 7, 32, 32
    seg = torch.from_numpy(g.integers(0, S, (B, H, W)))
    trav = torch.from_numpy((np.round(g.random((B, S)) * 16) / 16).astype(np.float32))
    conf = torch.from_numpy(g.random((B, S)).astype(np.float32))
    y = torch.from_numpy((g.random((B, S)) < 0.5).astype(np.float32))
    label = torch.from_numpy(g.random((B, H, W)) < 0.5)
    graph = Data(label=label, seg=seg, ptr=torch.arange(B + 1) * S, y=y.reshape(-1))
    a, b, c = MetricLogger(), MetricLogger(), MetricLogger()
    a.log_image(graph, trav.reshape(-1, 1), "test")
    a.log_confidence(graph, None, conf.reshape(-1), "test")
    b.log_maps(trav, conf, label, self_label=y, seg=seg, mode="test")            # per-segment sources: every key
    rows = (torch.arange(B).view(B, 1, 1) * S + seg).reshape(-1)
    dense = [t.reshape(-1)[rows].view(B, H, W) for t in (trav, conf, y)]
    c.log_maps(dense[0], dense[1], label, self_label=dense[2], mode="test")      # the painted maps: the binned keys
    ra, rb, rc = (m.get_epoch_results("test") for m in (a, b, c))
    MC.assert_results_equal(rb, ra)
    for k, v in ra.items():
        if "auroc_binned" in k or "_acc_" in k:
            assert rc[k] == v, k
    assert rc["test_auroc_gt_image"] is None and rc["test_auroc_anomaly_self_image"] is None


# ---- the C entry points and ops, without a GPU ----
def test_c_entry_points_refuse_bad_arguments():
    h = _lib.lib()
    words = (C.c_longlong * 64)()
    p = C.addressof(words)

    def desc(**kw):
        d = _lib.MetricDesc()
        d.score[0], d.target[0], d.thresholds, d.state = p, p, p, p
        d.n_scores = d.n_targets = 1
        d.B, d.H, d.W, d.T, d.state_stride = 1, 4, 4, 5000, 2 * 5001 + 8
        d.target_dtype[0] = _lib.METRIC_F32
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    call = lambda d: h.wvn_metric_accumulate(C.byref(d), None)   # noqa: E731
    assert h.wvn_metric_accumulate(None, None) == 1001
    for bad in (dict(T=1), dict(T=8193), dict(B=0), dict(B=1 << 15, H=1 << 8, W=1 << 8), dict(thresholds=None), dict(state=None),
                dict(state=p + 4), dict(thresholds=p + 2), dict(score=(0, None)), dict(target=(0, None)), dict(score=(0, p + 1)),
                dict(score_kind=(0, _lib.METRIC_PER_SEGMENT)), dict(target_kind=(0, _lib.METRIC_PER_SEGMENT)),
                dict(target_dtype=(0, 3)), dict(n_scores=3), dict(n_targets=0), dict(state_stride=2 * 5001),
                dict(seg_counts=p), dict(seg=p + 2, S=4, seg_bytes=4), dict(seg=p + 4, S=4, seg_bytes=8), dict(seg=p, S=4, seg_bytes=2),
                dict(seg=p, S=0, seg_bytes=4)):
        assert call(desc(**bad)) == 1001, bad
    assert all(w == 0 for w in words)
    assert h.wvn_metric_curve(None, p, 5000, p, p, p, p, p, None) == 1001
    assert h.wvn_metric_curve(p, p, 1, p, p, p, p, p, None) == 1001
    assert h.wvn_metric_curve(p, p, 8193, p, p, p, p, p, None) == 1001
    assert h.wvn_metric_curve(p, p, 5000, p + 4, p, p, p, p, None) == 1001
    assert h.wvn_metric_curve(p, p, 5000, p, p, p, p, None, None) == 1001
    assert h.wvn_metric_auroc_weighted(None, p, p, 4, p, p, None) == 1001
    assert h.wvn_metric_auroc_weighted(p, p, p, 0, p, p, None) == 1001
    assert h.wvn_metric_auroc_weighted(p, p, p, (1 << 24) + 1, p, p, None) == 1001
    assert h.wvn_metric_auroc_weighted(p, p + 4, p, 4, p, p, None) == 1001


def test_ops_refuse_cpu_tensors():
    th = torch.linspace(0, 1, 16)
    st = torch.zeros(1, ops.metric_state_words(16), dtype=torch.int64)
    with pytest.raises(_lib.WvnError):
        ops.metric_accumulate(st, th, [torch.rand(8)], [torch.zeros(8)])
    with pytest.raises(_lib.WvnError):
        ops.metric_curve(st[0], th)
    with pytest.raises(_lib.WvnError):
        ops.metric_auroc_weighted(torch.rand(4), torch.ones(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64))


def test_dropin_exports_the_metric_logger():
    import wild_visual_navigation_amd.dropin as dropin

    assert dropin.install(force_synthetic=True) == "synthetic"
    from wild_visual_navigation.utils import BinaryROC as R, MetricLogger as M   # the reference's import line

    assert M is MetricLogger and R is BinaryROC
    assert {"MetricLogger", "BinaryROC", "BinaryAUROC", "BinaryAccuracy"} <= set(dropin.UTILS_HOT)   # (with the reference present)
