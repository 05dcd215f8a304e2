"""Binary ROC / AUROC / accuracy from integer counts -- what the reference's MetricLogger takes from torchmetrics
(``ROC(task="binary", thresholds=5000)``, ``AUROC(task="binary")``, ``Accuracy(task="binary")``).

Definitions: include/wvn_hip.h "evaluation metrics" and tests/metrics_ref.py (DESIGN.md section 4 "Evaluation metrics").  They restate
the published behaviour of torchmetrics; PARITY WITH THE torchmetrics PACKAGE ITSELF IS UNPINNED (the package is not available here).
Two deliberate differences:
  * torchmetrics applies a sigmoid to every score of an update when any of them lies outside [0, 1]; that needs a global decision
    before the pass and is NOT reproduced: out-of-range scores fall into the first or the last bin and are counted (``n_out_of_range``);
  * torchmetrics raises on target values other than 0 / 1 / ignore_index; raising needs a host read: they are skipped and counted
    (``n_ignored``).  NaN scores are excluded and counted (``n_nan``).

On GPU tensors every update is ONE launch of the fused pixel pass (csrc/metrics.hip) and ``compute()`` returns device tensors: only the
caller's ``.item()`` synchronises.  On CPU tensors the same definitions run as torch operations (plumbing for host-side use and tests).

Exact AUROC (``thresholds=None``) is the Mann-Whitney statistic over weighted entries.  Every AUROC the reference logs is over
per-segment predictions, so an entry is a segment with its positive / negative pixel counts: give ``preds [B,S]`` with ``seg``, or a
vector of entries ``preds [N]``, ``target [N]``.  A dense per-pixel score map is refused there: use an integer ``thresholds``.
"""
from typing import List, Optional

import torch

from .. import _lib, ops

STATE_TAIL = _lib.METRIC_STATE_TAIL


def make_thresholds(T: int) -> torch.Tensor:
    """torch.linspace on the CPU in fp32: the table is an input everywhere, never recomputed on a device (other bits)."""
    T = int(T)
    if not 2 <= T <= _lib.METRIC_MAX_T:
        raise ValueError(f"thresholds must be an integer in [2, {_lib.METRIC_MAX_T}], got {T}")
    return torch.linspace(0, 1, T, dtype=torch.float32)


# ---- the definitions as torch operations (CPU route) -------------------------------------------------------------------------
def _class_torch(t: torch.Tensor, ignore_index) -> torch.Tensor:
    """0 negative, 1 positive, 2 skipped."""
    if t.dtype.is_floating_point:
        ok = torch.isfinite(t) & (t.abs() < 2.0e9)
        v = torch.where(ok, t, torch.full_like(t, 2)).trunc().to(torch.int64)
    else:
        ok = torch.ones(t.shape, dtype=torch.bool, device=t.device)
        v = t.to(torch.int64)
    cls = torch.where(v == 0, 0, torch.where(v == 1, 1, 2))
    if ignore_index is not None:
        cls = torch.where(v == int(ignore_index), 2, cls)
    return torch.where(ok, cls, 2)


def _rows_torch(seg: torch.Tensor, S: int, seg_off):
    seg = seg.to(torch.int64)
    B = seg.shape[0]
    if seg_off is None:
        base = (torch.arange(B, device=seg.device) * S).view(B, 1, 1)
        n = torch.full((B, 1, 1), S, dtype=torch.int64, device=seg.device)
    else:
        off = seg_off.to(torch.int64)
        base, n = off[:-1].view(B, 1, 1), (off[1:] - off[:-1]).view(B, 1, 1)
    valid = (seg >= 0) & (seg < n)
    return torch.where(valid, base + seg, 0), valid


def _table(t: "ops.PerSegment", seg_off) -> torch.Tensor:
    tab = t.table
    if seg_off is not None and tab.dim() == 2:
        tab = tab[:, 0]
    return tab.reshape(-1)


def _accumulate_torch(state, th, scores, targets, seg, seg_off, tau, ignore_index, seg_counts):
    T = th.numel()
    any_seg = any(isinstance(t, ops.PerSegment) for t in list(scores) + list(targets))
    row = valid = None
    if seg is not None:
        if seg.dim() == 2:
            seg = seg[None]
        S = 0
        for t in list(scores) + list(targets):
            if isinstance(t, ops.PerSegment) and seg_off is None:
                S = t.table.shape[1]
        if S == 0 and seg_off is None:
            S = 1 if seg_counts is None else seg_counts.shape[0] // seg.shape[0]
        row, valid = _rows_torch(seg, S, seg_off)
        row, valid = row.reshape(-1), valid.reshape(-1)
    elif any_seg:
        raise _lib.WvnError("per-segment sources need seg")

    def dense(t):
        return _table(t, seg_off)[row] if isinstance(t, ops.PerSegment) else t.reshape(-1)

    classes = []
    for t in targets:
        c = _class_torch(dense(t), ignore_index)
        if any_seg:
            c = torch.where(valid, c, 2)
        classes.append(c)
    tau32 = torch.tensor(tau, dtype=torch.float32)
    for i, s in enumerate(scores):
        p = dense(s).to(torch.float32)
        for j, c in enumerate(classes):
            st = state[i * len(targets) + j]
            skipped = c == 2
            nan = torch.isnan(p) & ~skipped
            use = ~skipped & ~nan
            pu, cu = p[use], c[use]
            k = torch.bucketize(pu, th, right=True)
            st[:2 * (T + 1)] += torch.bincount(k * 2 + cu, minlength=2 * (T + 1))
            pred = (pu > tau32).to(torch.int64)
            st[2 * (T + 1):2 * (T + 1) + 4] += torch.bincount(cu * 2 + pred, minlength=4)
            st[2 * (T + 1) + 4] += nan.sum()
            st[2 * (T + 1) + 5] += skipped.sum()
            st[2 * (T + 1) + 6] += ((pu < 0) | (pu > 1)).sum()
    if seg_counts is not None:
        rows = seg_counts.shape[0]
        for j, t in enumerate(targets):
            c = _class_torch(dense(t), ignore_index)   # (the segment's own validity, whatever the sources are)
            m = valid & (c < 2)
            seg_counts[:, j, :] += torch.bincount(row[m] * 2 + c[m], minlength=2 * rows).view(rows, 2).to(seg_counts.dtype)
    return state


def _curve_torch(st: torch.Tensor, th: torch.Tensor):
    T = th.numel()
    hist = st[:2 * (T + 1)].view(T + 1, 2)
    sfx = torch.flip(torch.cumsum(torch.flip(hist, [0]), 0), [0])
    P, N = int(hist[:, 1].sum()), int(hist[:, 0].sum())
    tps, fps = sfx[1:, 1].to(torch.float64), sfx[1:, 0].to(torch.float64)
    tpr = torch.flip(tps / float(P), [0]) if P > 0 else torch.zeros(T, dtype=torch.float64)
    fpr = torch.flip(fps / float(N), [0]) if N > 0 else torch.zeros(T, dtype=torch.float64)
    thr = torch.flip(th, [0]).to(torch.float64)
    degenerate = P == 0 or N == 0
    acc = 0.0
    if not degenerate:
        f, t = fpr.tolist(), tpr.tolist()
        for i in range(1, T):   # Python floats are IEEE doubles: the sum in its defined order
            acc = acc + ((f[i] - f[i - 1]) * (t[i] + t[i - 1])) * 0.5
    cm = st[2 * (T + 1):2 * (T + 1) + 4].tolist()
    n = sum(cm)
    accuracy = (cm[3] + cm[0]) / n if n > 0 else 0.0
    return fpr, tpr, thr, torch.tensor([acc, accuracy], dtype=torch.float64), torch.tensor([P, N, int(degenerate)], dtype=torch.int64)


def _auroc_weighted_torch(score, pos, neg):
    s, order = torch.sort(score.reshape(-1).float(), descending=True)
    s, p, n = s.tolist(), pos.reshape(-1)[order].tolist(), neg.reshape(-1)[order].tolist()
    U2 = above = P = N = 0
    i = 0
    while i < len(s):
        if s[i] != s[i]:
            i += 1
            continue
        j, gp, gn = i, 0, 0
        while j < len(s) and s[j] == s[i]:
            gp += int(p[j])
            gn += int(n[j])
            j += 1
        U2 += gn * (2 * above + gp)
        above += gp
        P += gp
        N += gn
        i = j
    degenerate = P == 0 or N == 0
    val = 0.0 if degenerate else float(U2) / float(2 * P * N)
    return torch.tensor([val], dtype=torch.float64), torch.tensor([U2, P, N, int(degenerate)], dtype=torch.int64)


# ---- the accumulator every metric and the MetricLogger share ------------------------------------------------------------------
class PairAccumulator:
    """States of n_scores x n_targets (score, target) pairs, fed by one fused pass per update.  ``T``: thresholds of the binned
    state; ``tau``: the accuracy threshold (predicted positive iff p > tau); ``exact``: also keep per-segment entries for the exact
    AUROC (per-segment scores with ``seg``, or vectors of entries)."""

    def __init__(self, n_scores: int = 1, n_targets: int = 1, T: int = 5000, tau: float = 0.5, exact: bool = False):
        self.n_scores, self.n_targets, self.T, self.tau, self.exact = int(n_scores), int(n_targets), int(T), float(tau), bool(exact)
        self._th_cpu = make_thresholds(T)
        self.thresholds = self._th_cpu
        self.state: Optional[torch.Tensor] = None
        self.device: Optional[torch.device] = None
        self._entries: List[List[tuple]] = [[] for _ in range(self.n_scores * self.n_targets)]
        self.exact_refused = [False] * (self.n_scores * self.n_targets)   # a dense score map went into this pair

    @property
    def words(self) -> int:
        return 2 * (self.T + 1) + STATE_TAIL

    def to(self, device):
        device = torch.device(device)
        if self.device == device:
            return self
        self.device = device
        self.thresholds = self._th_cpu.to(device)   # (made on the CPU, uploaded)
        self.state = torch.zeros(self.n_scores * self.n_targets, self.words, dtype=torch.int64, device=device) if self.state is None \
            else self.state.to(device)
        self._entries = [[tuple(t.to(device) for t in e) for e in es] for es in self._entries]
        return self

    def reset(self):
        if self.state is not None:
            self.state.zero_()
        self._entries = [[] for _ in self._entries]
        self.exact_refused = [False] * len(self._entries)

    def update(self, scores, targets, seg=None, seg_off=None, ignore_index=None, first_score: int = 0, first_target: int = 0,
               tau: Optional[float] = None):
        """One fused pass.  ``scores`` / ``targets`` may be a run of the accumulator's own (from ``first_score`` / ``first_target``):
        all targets, or one of them.  ``tau``: the accuracy threshold of this update (default: the accumulator's)."""
        scores, targets = list(scores), list(targets)
        ns, nt, fs, ft = len(scores), len(targets), int(first_score), int(first_target)
        if ns < 1 or nt < 1 or fs < 0 or ft < 0 or fs + ns > self.n_scores or ft + nt > self.n_targets or (nt != self.n_targets and nt != 1):
            raise ValueError(f"this accumulator holds {self.n_scores} scores x {self.n_targets} targets; an update takes a run of "
                             "scores and either every target or one")
        first = scores[0].table if isinstance(scores[0], ops.PerSegment) else scores[0]
        if first.numel() == 0:
            return
        if self.device is None or self.state is None or first.device != self.device:
            self.to(first.device)
        dense3 = [not isinstance(s, ops.PerSegment) and s.dim() != 1 for s in scores]
        per_seg = [isinstance(s, ops.PerSegment) for s in scores]
        seg_counts = None
        if self.exact and seg is not None and any(per_seg):
            rows = _table(scores[per_seg.index(True)], seg_off).numel()
            seg_counts = torch.zeros(rows, nt, 2, dtype=torch.int32, device=self.device)
        NT = self.n_targets
        rows = self.state[fs * NT:(fs + ns) * NT] if nt == NT else self.state[fs * NT + ft:(fs + ns) * NT:NT]
        tau = self.tau if tau is None else float(tau)
        if self.device.type == "cuda":
            ops.metric_accumulate(rows, self.thresholds, scores, targets, seg=seg, seg_off=seg_off, tau=tau,
                                  ignore_index=ignore_index, seg_counts=seg_counts)
        else:
            _accumulate_torch(rows, self.thresholds, scores, targets, seg, seg_off, tau, ignore_index, seg_counts)
        if not self.exact:
            return
        for i, s in enumerate(scores):
            for j, t in enumerate(targets):
                pair = (fs + i) * NT + ft + j
                if per_seg[i] and seg_counts is not None:
                    self._entries[pair].append((_table(s, seg_off).float(), seg_counts[:, j, 1], seg_counts[:, j, 0]))
                elif not dense3[i] and not per_seg[i] and not isinstance(t, ops.PerSegment):
                    c = _class_torch(t.reshape(-1), ignore_index)   # a vector of entries: one observation each
                    self._entries[pair].append((s.reshape(-1).float(), (c == 1).to(torch.int32), (c == 0).to(torch.int32)))
                else:
                    self.exact_refused[pair] = True

    def _pair(self, score: int, target: int) -> int:
        return score * self.n_targets + target

    def _empty(self):
        if self.state is None:
            self.to(self.device or "cpu")

    def curve(self, score: int = 0, target: int = 0):
        """(fpr, tpr, thresholds, scal = {binned AUROC, accuracy}, cnt = {P, N, degenerate}) of one pair, on the device."""
        self._empty()
        st = self.state[self._pair(score, target)]
        if self.device.type == "cuda":
            return ops.metric_curve(st, self.thresholds)
        return _curve_torch(st, self.thresholds)

    def counters(self, score: int = 0, target: int = 0) -> torch.Tensor:
        """int64 [3] = {n_nan, n_ignored, n_out_of_range} of one pair, on the device."""
        self._empty()
        o = 2 * (self.T + 1) + 4
        return self.state[self._pair(score, target), o:o + 3]

    def auroc_exact(self, score: int = 0, target: int = 0):
        """(scal fp64 [1], cnt int64 [4] = {U2, P, N, degenerate}) over the entries kept so far; None where a dense per-pixel score
        map went into the pair (no exact AUROC for those)."""
        self._empty()
        pair = self._pair(score, target)
        if not self.exact or self.exact_refused[pair]:
            return None
        es = self._entries[pair]
        if not es:
            return (torch.zeros(1, dtype=torch.float64, device=self.device),
                    torch.tensor([0, 0, 0, 1], dtype=torch.int64, device=self.device))
        s, p, n = (torch.cat([e[k] for e in es]) for k in range(3))
        if self.device.type == "cuda":
            return ops.metric_auroc_weighted(s, p, n)
        return _auroc_weighted_torch(s, p, n)


def _sources(preds, target, seg):
    """The update arguments of the three classes -> sources: [B,S] tables with ``seg`` are per-segment, everything else is dense."""
    if seg is not None and preds.dim() == 2:
        preds = ops.PerSegment(preds)
    elif preds.dim() not in (1, 3):
        raise ValueError(f"preds must be [B,H,W] or [N], or [B,S] with seg; got {tuple(preds.shape)}")
    if seg is not None and target.dim() == 2 and tuple(target.shape) != tuple(seg.shape):
        target = ops.PerSegment(target)
    return preds, target


class _BinaryMetric:
    def __init__(self, T: int, tau: float, exact: bool):
        self.acc = PairAccumulator(1, 1, T, tau, exact)

    def update(self, preds, target, seg=None, ignore_index=None):
        p, t = _sources(preds, target, seg)
        self._check(p)
        self.acc.update([p], [t], seg=seg, ignore_index=ignore_index)

    def _check(self, p):
        pass

    def __call__(self, preds, target, seg=None, ignore_index=None):
        self.update(preds, target, seg=seg, ignore_index=ignore_index)

    def reset(self):
        self.acc.reset()

    def to(self, device):
        self.acc.to(device)
        return self

    def counters(self) -> torch.Tensor:
        return self.acc.counters()


class BinaryROC(_BinaryMetric):
    """``compute()`` -> (fpr, tpr, thresholds), fp64 [T] in ascending fpr, as torchmetrics' binned binary ROC returns them."""

    def __init__(self, thresholds: int = 5000):
        super().__init__(int(thresholds), 0.5, False)

    def compute(self):
        fpr, tpr, thr, _, _ = self.acc.curve()
        return fpr, tpr, thr


class BinaryAUROC(_BinaryMetric):
    """``thresholds=int``: the trapezoid area under the binned ROC.  ``thresholds=None``: the exact AUROC over per-segment entries
    (``preds [B,S]`` with ``seg``, or vectors ``preds [N]``); a dense per-pixel map is refused.  ``degenerate()``: no positives or
    no negatives (the value is then 0)."""

    def __init__(self, thresholds: Optional[int] = None):
        self.exact = thresholds is None
        super().__init__(2 if self.exact else int(thresholds), 0.5, self.exact)

    def _check(self, p):
        if self.exact and not isinstance(p, ops.PerSegment) and p.dim() != 1:
            raise ValueError("BinaryAUROC(thresholds=None): the exact AUROC of a dense per-pixel score map is out of scope; give "
                             "per-segment preds [B,S] with seg, or use BinaryAUROC(thresholds=5000)")

    def _result(self):
        if self.exact:
            scal, cnt = self.acc.auroc_exact()
            return scal[0], cnt[3]
        _, _, _, scal, cnt = self.acc.curve()
        return scal[0], cnt[2]

    def compute(self) -> torch.Tensor:
        return self._result()[0]

    def degenerate(self) -> torch.Tensor:
        return self._result()[1]


class BinaryAccuracy(_BinaryMetric):
    """(cm[1][1] + cm[0][0]) / sum cm with "predicted positive iff p > threshold" (strict, the reference's ``bp > threshold``)."""

    def __init__(self, threshold: float = 0.5):
        super().__init__(2, float(threshold), False)

    def compute(self) -> torch.Tensor:
        return self.acc.curve()[3][1]

    def confusion_matrix(self) -> torch.Tensor:
        """int64 [2][2]: cm[target][predicted], on the device."""
        self.acc._empty()
        o = 2 * (self.acc.T + 1)
        return self.acc.state[0, o:o + 4].view(2, 2)
