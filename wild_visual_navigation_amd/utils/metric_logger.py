"""MetricLogger: how good is a traversability model -- ROC at 5000 thresholds, AUROC and accuracy of the traversability and the
confidence outputs, against hand labels ("gt") and against the self-supervision labels ("self"), in segment space and in image
space.  Same methods and result keys as the MetricLogger of the reference's training code, which stands on torchmetrics; here the
numbers come from utils/metrics.py (integer counts from one fused pixel pass per call; parity with the torchmetrics package itself is
unpinned, see that module).

Per mode ("train" / "val" / "test") one accumulator holds the image-space pairs {traversability, confidence} x {gt, self} and one the
segment-space pairs.  ``log_image`` and ``log_confidence`` are ONE kernel launch each (plus the clear of the per-segment count
buffer): ``res[:, 0]`` / ``confidence`` and ``graph.y`` are gathered through ``graph.seg + graph.ptr`` on load -- ``graph.seg`` as int64
or int32, read as it is -- and no projected map is built.

``log_confidence`` keeps the reference's pairing exactly as it is written there: ``..._auroc_anomaly_gt_image`` is fed the SELF labels
and ``..._auroc_anomaly_self_image`` the HAND labels, while ``..._acc_anomaly_gt_image`` / ``..._acc_anomaly_self_image`` are fed what
their names say.

Keys of ``get_epoch_results`` beyond the reference's: ``{mode}_auroc_binned_*`` (the area under the binned ROC; defined for dense maps
too), ``{mode}_auroc_gt_seg`` / ``{mode}_auroc_self_seg`` and ``{mode}_roc_gt_seg`` / ``{mode}_roc_self_seg`` (the reference only hands
those to its log handle).  The exact AUROC keys need per-segment scores; where a dense score map was logged (``log_maps`` without
per-segment scores) they are None.
"""
from typing import Callable, Optional

import torch

from ..ops import PerSegment
from .metrics import PairAccumulator

MODES = ("train", "val", "test")
T_ROC = 5000
_TRAV, _CONF = 0, 1     # scores of the image-space accumulator
_GT, _SELF = 0, 1       # targets


class _Logged:
    """What the log handle receives in place of a torchmetrics Metric: ``compute()`` -> 0-d tensor on the device."""

    def __init__(self, fn):
        self._fn = fn

    def compute(self) -> torch.Tensor:
        return self._fn()


class MetricLogger:
    def __init__(self, log_handel: Optional[Callable] = None, log_roc_image: bool = False):
        self.log_handel = log_handel
        self.log_roc_image = bool(log_roc_image)
        self._img = {m: PairAccumulator(2, 2, T_ROC, 0.5, exact=True) for m in MODES}
        self._seg = {m: PairAccumulator(1, 2, T_ROC, 0.5, exact=True) for m in MODES}

    def to(self, device):
        for a in list(self._img.values()) + list(self._seg.values()):
            a.to(device)
        return self

    def _mode(self, mode: str) -> str:
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        return mode

    def _log(self, name, fn, batch_size):
        if self.log_handel is not None:
            self.log_handel(name, _Logged(fn), on_epoch=True, on_step=False, batch_size=batch_size)

    @staticmethod
    def _exact(acc: PairAccumulator, score: int, target: int):
        r = acc.auroc_exact(score, target)
        return None if r is None else r[0][0]

    # ---- segment space ----
    @torch.no_grad()
    def log_segment(self, graph, res, mode):
        """res: one prediction per node ([N] or [N,C], column 0); graph.label / graph.y: one hand / self label per node."""
        mode = self._mode(mode)
        acc = self._seg[mode]
        preds = res[:, 0] if res.dim() == 2 else res
        acc.update([preds.reshape(-1)], [graph.label.reshape(-1), graph.y.reshape(-1)])
        n = int(graph.label.shape[0])
        self._log(f"{mode}_metric_auroc_gt_seg", lambda: self._exact(acc, 0, _GT), n)
        self._log(f"{mode}_metric_auroc_self_seg", lambda: self._exact(acc, 0, _SELF), n)

    # ---- image space ----
    def _graph_update(self, graph, table, mode, score, tau):
        acc = self._img[mode]
        acc.update([PerSegment(table)], [graph.label, PerSegment(graph.y)], seg=graph.seg, seg_off=graph.ptr.to(graph.seg.device),
                   first_score=score, tau=tau)
        return acc

    @torch.no_grad()
    def log_image(self, graph, res, mode, threshold=0.5):
        """graph.label [BS,H,W] hand labels, graph.seg [BS,H,W], graph.ptr [BS + 1], graph.y [N] self labels; res [N,C]: column 0 is
        the traversability of every node.  Accuracy: predicted positive iff traversability > threshold."""
        mode = self._mode(mode)
        acc = self._graph_update(graph, res, mode, _TRAV, threshold)
        BS = int(graph.label.shape[0])
        self._log(f"{mode}_metric_auroc_gt_image", lambda: self._exact(acc, _TRAV, _GT), BS)
        self._log(f"{mode}_metric_auroc_self_image", lambda: self._exact(acc, _TRAV, _SELF), BS)
        self._log(f"{mode}_metric_acc_gt_image", lambda: acc.curve(_TRAV, _GT)[3][1], BS)
        self._log(f"{mode}_metric_acc_self_image", lambda: acc.curve(_TRAV, _SELF)[3][1], BS)

    @torch.no_grad()
    def log_confidence(self, graph, res, confidence, mode):
        """confidence [N]: one value per node.  The reference's pairing is kept (module docstring): auroc_anomaly_gt_image <- self
        labels, auroc_anomaly_self_image <- hand labels; the two accuracies as named, at threshold 0.5."""
        mode = self._mode(mode)
        acc = self._graph_update(graph, confidence, mode, _CONF, 0.5)
        BS = int(graph.label.shape[0])
        self._log(f"{mode}_metric_auroc_anomaly_gt_image", lambda: self._exact(acc, _CONF, _SELF), BS)
        self._log(f"{mode}_metric_auroc_anomaly_self_image", lambda: self._exact(acc, _CONF, _GT), BS)
        self._log(f"{mode}_metric_acc_anomaly_gt_image", lambda: acc.curve(_CONF, _GT)[3][1], BS)
        self._log(f"{mode}_metric_acc_anomaly_self_image", lambda: acc.curve(_CONF, _SELF)[3][1], BS)

    @torch.no_grad()
    def log_maps(self, trav, conf, label, self_label=None, seg=None, mode="test", threshold=0.5):
        """The batched outputs of predict_per_pixel / predict_per_segment / predict_and_extract: ``trav`` and ``conf`` are maps
        [B,H,W], or per-segment [B,S] with ``seg`` [B,H,W]; ``label`` [B,H,W] hand labels; ``self_label`` (optional) a map or [B,S].
        One launch for all four pairs; both accuracies use ``threshold``.  ``conf`` may be None."""
        mode = self._mode(mode)
        acc = self._img[mode]

        def src(t):
            return PerSegment(t) if (seg is not None and t.dim() == 2 and tuple(t.shape) != tuple(seg.shape)) else t

        scores = [src(trav)] + ([src(conf)] if conf is not None else [])
        targets = [label] + ([src(self_label)] if self_label is not None else [])
        acc.update(scores, targets, seg=seg, first_score=_TRAV, first_target=_GT, tau=threshold)

    # ---- results ----
    def get_epoch_results(self, mode):
        """Every figure of the epoch as Python floats (ROC curves as numpy arrays): the one place that synchronises."""
        mo = self._mode(mode)
        img, sg = self._img[mo], self._seg[mo]

        def val(t):
            return None if t is None else float(t.item())

        def roc(c, want=True):
            return [a.cpu().numpy() for a in c[:3]] if want else [None, None, None]

        c = {(s, t): img.curve(s, t) for s in (_TRAV, _CONF) for t in (_GT, _SELF)}
        cs = {t: sg.curve(0, t) for t in (_GT, _SELF)}
        return {
            f"{mo}_roc_gt_image": roc(c[_TRAV, _GT], self.log_roc_image),
            f"{mo}_roc_self_image": roc(c[_TRAV, _SELF], self.log_roc_image),
            f"{mo}_auroc_gt_image": val(self._exact(img, _TRAV, _GT)),
            f"{mo}_auroc_self_image": val(self._exact(img, _TRAV, _SELF)),
            f"{mo}_auroc_anomaly_gt_image": val(self._exact(img, _CONF, _SELF)),
            f"{mo}_auroc_anomaly_self_image": val(self._exact(img, _CONF, _GT)),
            f"{mo}_acc_gt_image": val(c[_TRAV, _GT][3][1]),
            f"{mo}_acc_self_image": val(c[_TRAV, _SELF][3][1]),
            f"{mo}_acc_anomaly_gt_image": val(c[_CONF, _GT][3][1]),
            f"{mo}_acc_anomaly_self_image": val(c[_CONF, _SELF][3][1]),
            f"{mo}_auroc_binned_gt_image": val(c[_TRAV, _GT][3][0]),
            f"{mo}_auroc_binned_self_image": val(c[_TRAV, _SELF][3][0]),
            f"{mo}_auroc_binned_anomaly_gt_image": val(c[_CONF, _SELF][3][0]),
            f"{mo}_auroc_binned_anomaly_self_image": val(c[_CONF, _GT][3][0]),
            f"{mo}_roc_gt_seg": roc(cs[_GT]),
            f"{mo}_roc_self_seg": roc(cs[_SELF]),
            f"{mo}_auroc_gt_seg": val(self._exact(sg, 0, _GT)),
            f"{mo}_auroc_self_seg": val(self._exact(sg, 0, _SELF)),
        }

    def reset(self, mode):
        mode = self._mode(mode)
        self._img[mode].reset()
        self._seg[mode].reset()
