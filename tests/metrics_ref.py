"""The evaluation metrics (utils/metrics.py, csrc/metrics.hip) stated once in numpy and Python integers.

Restated from the published behaviour of torchmetrics' binary ROC / AUROC / accuracy, which the reference's MetricLogger uses.
PARITY WITH THE torchmetrics PACKAGE ITSELF IS UNPINNED: the package is absent.  Two deliberate differences: the rule "apply a sigmoid
to every score if any lies outside [0, 1]" is not reproduced (out-of-range scores fall into bin 0 or bin T and are counted), and
invalid targets are skipped and counted where torchmetrics raises.
"""
import numpy as np
import torch


def thresholds(T: int = 5000) -> np.ndarray:
    """The table: torch.linspace on the CPU in float32 (numpy's linspace gives other bits)."""
    return torch.linspace(0, 1, T, dtype=torch.float32).numpy()


def bin_of(p: np.ndarray, th: np.ndarray) -> np.ndarray:
    """k(p) = #{t : th[t] <= p} in float32; NaN entries are meaningless (the caller excludes them)."""
    p = np.asarray(p, np.float32)
    return np.searchsorted(th, np.where(np.isnan(p), np.float32(0), p), side="right").astype(np.int64)


def target_class(t: np.ndarray, ignore_index=None) -> np.ndarray:
    """0 negative, 1 positive, 2 skipped; floats are truncated toward zero as ``.type(torch.long)`` does."""
    t = np.asarray(t)
    if t.dtype.kind == "f":
        ok = np.isfinite(t) & (np.abs(t) < 2.0e9)
        v = np.trunc(np.where(ok, t, 2)).astype(np.int64)
        v = np.where(ok, v, 2)
        bad = ~ok
    else:
        v = t.astype(np.int64)
        bad = np.zeros(t.shape, bool)
    cls = np.where(v == 0, 0, np.where(v == 1, 1, 2))
    if ignore_index is not None:
        cls = np.where(v == int(ignore_index), 2, cls)
    return np.where(bad, 2, cls).astype(np.int64)


def segment_rows(seg: np.ndarray, S=None, seg_off=None):
    """seg [B,H,W] -> (row [B,H,W], valid [B,H,W]): row(b, s) = b S + s, or seg_off[b] + s with seg_off[b+1] - seg_off[b] segments."""
    seg = np.asarray(seg).astype(np.int64)
    B = seg.shape[0]
    if seg_off is None:
        base = (np.arange(B, dtype=np.int64) * int(S)).reshape(B, 1, 1)
        n = np.full((B, 1, 1), int(S), np.int64)
    else:
        off = np.asarray(seg_off, np.int64)
        base = off[:-1].reshape(B, 1, 1)
        n = (off[1:] - off[:-1]).reshape(B, 1, 1)
    valid = (seg >= 0) & (seg < n)
    return np.where(valid, base + seg, 0), valid


def empty_state(T: int) -> dict:
    return {"hist": np.zeros((T + 1, 2), np.int64), "cm": np.zeros((2, 2), np.int64), "n_nan": 0, "n_ignored": 0, "n_out_of_range": 0}


def accumulate(state: dict, p: np.ndarray, cls: np.ndarray, th: np.ndarray, tau: float = 0.5) -> dict:
    """Adds the pixels (p float32, cls in {0, 1, 2}; a segment-skipped pixel arrives as class 2) into the state."""
    p = np.asarray(p, np.float32).ravel()
    cls = np.asarray(cls).ravel()
    T = len(th)
    skipped = cls == 2
    nan = np.isnan(p) & ~skipped
    use = ~skipped & ~nan
    state["n_ignored"] += int(skipped.sum())
    state["n_nan"] += int(nan.sum())
    pu, cu = p[use], cls[use]
    state["n_out_of_range"] += int(((pu < 0) | (pu > 1)).sum())
    k = bin_of(pu, th)
    np.add.at(state["hist"], (k, cu), 1)
    pred = (pu > np.float32(tau)).astype(np.int64)
    np.add.at(state["cm"], (cu, pred), 1)
    assert state["hist"].shape == (T + 1, 2)
    return state


def segment_counts(cls: np.ndarray, row: np.ndarray, valid: np.ndarray, rows: int) -> np.ndarray:
    """[rows, 2]: pixels of each segment row in class 0 / 1."""
    out = np.zeros((rows, 2), np.int64)
    m = valid.ravel() & (cls.ravel() < 2)
    np.add.at(out, (row.ravel()[m], cls.ravel()[m]), 1)
    return out


def roc(hist: np.ndarray, th: np.ndarray):
    """(fpr, tpr, thresholds) float64 in ascending fpr, P, N."""
    hist = np.asarray(hist, np.int64)
    T = len(th)
    sfx = np.cumsum(hist[::-1], axis=0)[::-1]          # sfx[k] = sum over bins >= k
    tps, fps = sfx[1:, 1], sfx[1:, 0]                  # tps[t] = sum over k > t
    P, N = int(hist[:, 1].sum()), int(hist[:, 0].sum())
    tpr = tps.astype(np.float64) / np.float64(P) if P > 0 else np.zeros(T)
    fpr = fps.astype(np.float64) / np.float64(N) if N > 0 else np.zeros(T)
    return fpr[::-1].copy(), tpr[::-1].copy(), th[::-1].astype(np.float64), P, N


def auroc_binned(fpr: np.ndarray, tpr: np.ndarray, P: int, N: int):
    """(value, degenerate): the trapezoid sum in float64, one term after the other in ascending index."""
    if P == 0 or N == 0:
        return 0.0, True
    acc = np.float64(0.0)
    for i in range(1, len(fpr)):
        dx = np.float64(fpr[i]) - np.float64(fpr[i - 1])
        sy = np.float64(tpr[i]) + np.float64(tpr[i - 1])
        acc = acc + (dx * sy) * np.float64(0.5)
    return float(acc), False


def accuracy(cm: np.ndarray) -> float:
    cm = np.asarray(cm, np.int64)
    n = int(cm.sum())
    return float(np.float64(int(cm[1, 1] + cm[0, 0])) / np.float64(n)) if n > 0 else 0.0


def auroc_exact(score, pos, neg):
    """(value, degenerate, U2, P, N) of weighted entries: Mann-Whitney with tie groups, Python integers."""
    score = np.asarray(score, np.float32).ravel()
    pos = [int(v) for v in np.asarray(pos).ravel()]
    neg = [int(v) for v in np.asarray(neg).ravel()]
    keep = [i for i in range(len(score)) if not np.isnan(score[i])]
    keep.sort(key=lambda i: -float(score[i]))
    U2 = above = P = N = 0
    i = 0
    while i < len(keep):
        j = i
        gp = gn = 0
        while j < len(keep) and score[keep[j]] == score[keep[i]]:
            gp += pos[keep[j]]
            gn += neg[keep[j]]
            j += 1
        U2 += gn * (2 * above + gp)
        above += gp
        P += gp
        N += gn
        i = j
    if P == 0 or N == 0:
        return 0.0, True, U2, P, N
    return float(np.float64(U2) / np.float64(2 * P * N)), False, U2, P, N
