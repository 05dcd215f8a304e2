"""One optimisation step of SimpleGCN (TraversabilityLoss, Adam) on HIP kernels (csrc/simple_gcn_train.hip), data-parallel with the
two exchanges of the MLP step (trainer.py):

    phase A  graph + transposed graph, the three layers with h1, h2, out kept, per-row reconstruction loss, LOCAL statistic
             {n_lab, sum, sum^2, N}  (fp64)
       -> all-reduce(sum) of 4 doubles (and a MAX of {max, -min} of the reconstruction loss for moving_average)
    phase B  loss gradient seed, backward layers through A^T, weight and bias gradients -> flat gradient [n_param + 2] fp32
       -> all-reduce(sum) of the gradient (SimpleMLP's length for the same (D, h1, h2))
    phase C  Adam + losses + the commit of the confidence statistic: the MLP step's own kernel

A rank trains on whole graphs (``Batch.edge_index`` addresses this rank's nodes only); local contributions are sums scaled by the
global normalisers inside phase B, so the N-rank trajectory equals the one-rank trajectory on the concatenated batch up to fp32
summation order.  Every sum has one fixed order: a step is bitwise reproducible and does not depend on the order of the edges.
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib
from ..model.simple_gcn import SimpleGCN
from .trainer import TrainerState


class GcnTrainer(TrainerState):
    def __init__(self, model: SimpleGCN, lr: float = 1e-3, std_factor: float = 0.5, w_trav: float = 0.03, w_reco: float = 0.5,
                 process_group=None, method: str = "latest_measurement", anomaly_balanced: bool = True):
        super().__init__(model, lr, method, process_group)
        self.anomaly_balanced = bool(anomaly_balanced)
        # a conf descriptor (device state) for anything but the original configuration, as in MlpTrainer
        self._conf = method != "latest_measurement" or not self.anomaly_balanced
        self.std_factor, self.w_trav, self.w_reco = std_factor, w_trav, w_reco
        self.last_confidence: Optional[torch.Tensor] = None
        self._ws = None
        self._saved = None        # (nodes, capacity) of the last phase A

    def _alloc_extra(self, dev):
        self.minmax = torch.zeros(2, dtype=torch.float32, device=dev)
        self.sync_word = torch.zeros(1, dtype=torch.int32, device=dev)   # arrival counter of phase A's last layer
        self.bad_edges = torch.zeros(1, dtype=torch.int32, device=dev)   # edges the last phase A dropped (an endpoint outside [0, N))
        self._ws = self._saved = None

    def _workspace(self, nodes: int, capacity: int) -> torch.Tensor:
        need = _lib.lib().wvn_gcn_train_workspace_bytes(C.byref(self.model.desc), nodes, capacity)
        if need == 0:
            raise _lib.WvnError(f"no SimpleGCN training workspace for {nodes} nodes and {capacity} neighbour entries (at most 65536 nodes "
                                f"per rank and step)")
        if self._ws is None or self._ws.numel() < need or self._ws.device != self._state_dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self._state_dev)
        return self._ws

    def saved_activations(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Clones of h1 [N, h1] and h2 [N, h2] of the last phase A on this rank.  A test and debug accessor: the values are read out
        of the step's workspace."""
        return self._saved_views()[:2]

    def saved_output(self) -> torch.Tensor:
        """A clone of phase A's ``out`` [N, 1 + D] (a test and debug accessor, as ``saved_activations``)."""
        return self._saved_views()[2]

    def _saved_views(self):
        if self._saved is None:
            raise _lib.WvnError("no phase A has run on this rank's nodes yet")
        N, cap = self._saved
        d = self.model.desc
        offs = (C.c_size_t * 3)()
        _lib.check(_lib.lib().wvn_gcn_train_saved(C.byref(d), N, cap, C.addressof(offs)), "wvn_gcn_train_saved")
        return tuple(self._ws[o:o + 4 * N * w].view(torch.float32).view(N, w).clone() for o, w in zip(offs, (d.H1, d.H2, 1 + d.D)))

    @torch.no_grad()
    def forward_backward(self, x: torch.Tensor, edge_index: torch.Tensor, y: torch.Tensor, y_valid: torch.Tensor,
                         want_confidence: bool = False) -> torch.Tensor:
        """Phases A and B on this rank's graphs (x [N, >= D], edge_index [2, E] int64, y [N], y_valid [N]; N may be 0), with both
        all-reduces: the flat gradient of the loss over all ranks' nodes, in ``flat_params()`` order, with the two loss sums behind
        it.  No Adam step."""
        self._phases_ab(x, edge_index, y, y_valid, want_confidence)
        return self.grads

    @torch.no_grad()
    def train_step(self, x: torch.Tensor, edge_index: torch.Tensor, y: torch.Tensor, y_valid: torch.Tensor,
                   want_confidence: bool = False) -> torch.Tensor:
        """One step on this rank's graphs.  Returns the device tensor losses[5] = {total, loss_trav, loss_reco, conf_mean, conf_std}
        (no host synchronisation here)."""
        return self._phase_c(self._phases_ab(x, edge_index, y, y_valid, want_confidence))

    def _phases_ab(self, x, edge_index, y, y_valid, want_confidence):
        """``forward_backward``; returns the step's ConfDesc (or None) for phase C."""
        _lib.require_cuda(x, "x")
        lib, d = _lib.lib(), self.model.desc
        dev = x.device
        self._state(dev)
        D = self.model.input_size
        if x.dim() != 2 or x.shape[1] < D:
            raise _lib.WvnError(f"x must be [N, >= {D}], got {tuple(x.shape)}")
        edge_index = SimpleGCN._check_edges(edge_index, "edge_index")
        x = x.float()
        N, E = x.shape[0], edge_index.shape[1]
        if N and (x.stride(1) != 1 or x.stride(0) < D):
            x = x.contiguous()
        y = y.float().contiguous()
        yv = y_valid.to(torch.uint8).contiguous()
        if y.shape[0] != N or yv.shape[0] != N:
            raise _lib.WvnError(f"y and y_valid must hold one entry per node ({N}), got {tuple(y.shape)} and {tuple(y_valid.shape)}")
        flat = self.model.flat_params()
        _lib.require_cuda(flat, "parameters")
        st = _lib.stream()
        conf = torch.empty(N, dtype=torch.float32, device=dev) if want_confidence else None
        cd = self._conf_desc()
        cdp = None if cd is None else C.byref(cd)
        cap = E + N
        ws = self._workspace(N, cap) if N else None

        def phase_a():
            _lib.check(lib.wvn_gcn_train_phase_a(C.byref(d), flat.data_ptr(), x.data_ptr(), x.stride(0), edge_index.data_ptr() if E else 0,
                                                 edge_index.stride(0), edge_index.stride(1), E, yv.data_ptr(), N, cap,
                                                 self.stats.data_ptr(), self.bad_edges.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 self.sync_word.data_ptr(), cdp, st), "wvn_gcn_train_phase_a")
            self._saved = (N, cap)

        def phase_b():
            _lib.check(lib.wvn_gcn_train_phase_b(C.byref(d), flat.data_ptr(), x.data_ptr(), x.stride(0), y.data_ptr(), yv.data_ptr(), N, cap,
                                                 self.stats.data_ptr(), self.std_factor, self.w_trav, self.w_reco, self.grads.data_ptr(),
                                                 _lib.ptr(conf), ws.data_ptr(), ws.numel(), cdp, st), "wvn_gcn_train_phase_b")

        if N == 0:
            self.bad_edges.zero_()
        self._exchange(phase_a, phase_b, launch=N > 0)
        self.last_confidence = conf
        return cd
