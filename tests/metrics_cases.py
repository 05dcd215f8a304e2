"""Synthetic graphs and the expected MetricLogger results (from tests/metrics_ref.py) shared by the host and the GPU metric tests."""
import numpy as np
import torch

import metrics_ref as MR
from wild_visual_navigation_amd.utils import Batch, Data

T_ROC = 5000


def make_batch(seed: int, n_graphs: int = 3, H: int = 24, W: int = 40):
    """(graph, res [N,3], confidence [N]): n_graphs graphs of 5 to 9 segments; predictions rounded so that scores tie across graphs."""
    g = np.random.default_rng(seed)
    datas = []
    for _ in range(n_graphs):
        S = int(g.integers(5, 10))
        seg = g.integers(0, S, (1, H, W))
        datas.append(Data(x=torch.from_numpy(g.standard_normal((S, 4)).astype(np.float32)),
                          y=torch.from_numpy((g.random(S) < 0.5).astype(np.float32)),
                          seg=torch.from_numpy(seg.astype(np.int64)),
                          label=torch.from_numpy(g.random((1, H, W)) < 0.4)))
    graph = Batch.from_data_list(datas)
    N = graph.x.shape[0]
    res = torch.from_numpy(g.random((N, 3)).astype(np.float32))
    res[:, 0] = torch.round(res[:, 0] * 20) / 20
    conf = torch.from_numpy(np.round(g.random(N) * 10).astype(np.float32) / 10)
    return graph, res, conf


def graph_to(graph, device):
    out = Batch()
    for k, v in vars(graph).items():
        setattr(out, k, v.to(device) if torch.is_tensor(v) else v)
    return out


def pack(state: dict) -> np.ndarray:
    """A reference state in the word layout of include/wvn_hip.h: hist [T+1][2], cm [2][2], n_nan, n_ignored, n_out_of_range, 0."""
    return np.concatenate([state["hist"].ravel(), state["cm"].ravel(),
                           np.array([state["n_nan"], state["n_ignored"], state["n_out_of_range"], 0], np.int64)])


def ref_accumulate(states, th, scores, targets, seg=None, S=None, seg_off=None, tau=0.5, ignore_index=None, rows=None):
    """The fused pass on numpy sources (a per-segment source is ("seg", table)): adds into states [n_scores * n_targets] and
    returns the per-segment counts [rows][n_targets][2] (None without seg)."""
    any_seg = any(isinstance(x, tuple) for x in list(scores) + list(targets))
    row = valid = None
    if seg is not None:
        row, valid = MR.segment_rows(seg, S=S, seg_off=seg_off)

    def dense(x):
        return x[1].reshape(-1)[row] if isinstance(x, tuple) else x

    raw = [MR.target_class(dense(t), ignore_index) for t in targets]
    classes = [np.where(valid, c, 2) if any_seg else c for c in raw]
    for i, s in enumerate(scores):
        for j, c in enumerate(classes):
            MR.accumulate(states[i * len(targets) + j], dense(s), c, th, tau)
    if seg is None:
        return None
    return np.stack([MR.segment_counts(c, row, valid, rows) for c in raw], axis=1)


class Expected:
    """The four image-space pairs {trav, conf} x {gt, self} and the two segment-space pairs, accumulated with metrics_ref."""

    def __init__(self):
        self.th = MR.thresholds(T_ROC)
        self.img = {(s, t): MR.empty_state(T_ROC) for s in (0, 1) for t in (0, 1)}
        self.ent = {(s, t): ([], [], []) for s in (0, 1) for t in (0, 1)}
        self.seg = {t: MR.empty_state(T_ROC) for t in (0, 1)}
        self.seg_ent = {t: ([], [], []) for t in (0, 1)}

    def _graph(self, graph, table, s, tau):
        seg, off = graph.seg.numpy(), graph.ptr.numpy()
        row, valid = MR.segment_rows(seg, seg_off=off)
        N = int(off[-1])
        classes = (np.where(valid, MR.target_class(graph.label.numpy()), 2), np.where(valid, MR.target_class(graph.y.numpy()[row]), 2))
        p = table[row]
        for t, cls in enumerate(classes):
            MR.accumulate(self.img[s, t], p, cls, self.th, tau)
            cnt = MR.segment_counts(cls, row, valid, N)
            for lst, v in zip(self.ent[s, t], (table, cnt[:, 1], cnt[:, 0])):
                lst.append(v)

    def log_image(self, graph, res, threshold=0.5):
        self._graph(graph, res[:, 0].numpy(), 0, threshold)

    def log_confidence(self, graph, conf):
        self._graph(graph, conf.numpy(), 1, 0.5)

    def log_segment(self, graph, preds, label):
        for t, tgt in enumerate((label.numpy(), graph.y.numpy())):
            cls = MR.target_class(tgt)
            MR.accumulate(self.seg[t], preds.numpy(), cls, self.th, 0.5)
            for lst, v in zip(self.seg_ent[t], (preds.numpy(), (cls == 1).astype(np.int64), (cls == 0).astype(np.int64))):
                lst.append(v)

    @staticmethod
    def _exact(ent):
        if not ent[0]:
            return 0.0
        return MR.auroc_exact(*(np.concatenate(e) for e in ent))[0]

    def results(self, mo: str, log_roc_image: bool) -> dict:
        def curve(st):
            fpr, tpr, thr, P, N = MR.roc(st["hist"], self.th)
            return [fpr, tpr, thr], MR.auroc_binned(fpr, tpr, P, N)[0], MR.accuracy(st["cm"])

        c = {k: curve(st) for k, st in self.img.items()}
        cs = {k: curve(st) for k, st in self.seg.items()}
        none = [None, None, None]
        return {
            f"{mo}_roc_gt_image": c[0, 0][0] if log_roc_image else none,
            f"{mo}_roc_self_image": c[0, 1][0] if log_roc_image else none,
            f"{mo}_auroc_gt_image": self._exact(self.ent[0, 0]),
            f"{mo}_auroc_self_image": self._exact(self.ent[0, 1]),
            f"{mo}_auroc_anomaly_gt_image": self._exact(self.ent[1, 1]),      # (the reference's pairing: fed the self labels)
            f"{mo}_auroc_anomaly_self_image": self._exact(self.ent[1, 0]),    # (fed the hand labels)
            f"{mo}_acc_gt_image": c[0, 0][2],
            f"{mo}_acc_self_image": c[0, 1][2],
            f"{mo}_acc_anomaly_gt_image": c[1, 0][2],
            f"{mo}_acc_anomaly_self_image": c[1, 1][2],
            f"{mo}_auroc_binned_gt_image": c[0, 0][1],
            f"{mo}_auroc_binned_self_image": c[0, 1][1],
            f"{mo}_auroc_binned_anomaly_gt_image": c[1, 1][1],
            f"{mo}_auroc_binned_anomaly_self_image": c[1, 0][1],
            f"{mo}_roc_gt_seg": cs[0][0],
            f"{mo}_roc_self_seg": cs[1][0],
            f"{mo}_auroc_gt_seg": self._exact(self.seg_ent[0]),
            f"{mo}_auroc_self_seg": self._exact(self.seg_ent[1]),
        }


REFERENCE_KEYS = ("roc_gt_image", "roc_self_image", "auroc_gt_image", "auroc_self_image", "auroc_anomaly_gt_image",
                  "auroc_anomaly_self_image", "acc_gt_image", "acc_self_image", "acc_anomaly_gt_image", "acc_anomaly_self_image")


def assert_results_equal(got: dict, want: dict):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, list):
            assert len(g) == 3
            for a, b in zip(g, w):
                assert (a is None) == (b is None), k
                if b is not None:
                    assert np.array_equal(np.asarray(a), b), k
        else:
            assert g == w, (k, g, w)
