"""One optimisation step of the online traversability MLP on HIP kernels, with the two tiny
exchanges that make it data-parallel:

    phase A  forward + per-row reconstruction loss + LOCAL statistic {n_lab, sum, sum^2, R}  (fp64)
       -> all-reduce(sum) of 4 doubles      (the loss normalisers / confidence mean,std are GLOBAL)
    phase B  loss gradient + backward GEMMs -> flat gradient [n_param + 2] fp32
       -> all-reduce(sum) of 478 KB (D=384) / 138 KB (D=90)   -- RCCL over xGMI, latency-bound
    phase C  Adam + losses; every rank applies the identical update => replicas stay bit-identical

Local contributions are sums (not means) scaled by the global normalisers inside phase B, so the
N-GPU trajectory equals the 1-GPU trajectory on the concatenated batch up to fp32 summation order.
Reference arithmetic: traversability_estimator.py:464-477, loss.py:93-160, torch.optim.Adam.

ConfidenceGenerator methods other than latest_measurement, and anomaly_balanced=False, run through the *_conf entry points of
the same phases: the statistic's memory is a small persistent device state (``conf_state``, include/wvn_hip.h) that phase B
reads and phase C commits on every rank alike.  moving_average adds one collective between phases A and B: a MAX over the
ranks of {max, -min} of the reconstruction loss (two floats).
"""
import ctypes as C
from typing import Dict, Optional

import torch

from .. import _lib
from ..distributed import allreduce_max_, allreduce_sum_
from ..model.simple_mlp import SimpleMLP


class TrainerState:
    """What the fused trainers (MlpTrainer, GcnTrainer, RnvpTrainer) share: the device buffers of a step, the confidence statistic's
    device state and its exchange with a ConfidenceGenerator, the Adam moments in ``torch.optim.Adam.state_dict()`` shape, and the
    data-parallel skeleton of the step (``_exchange``: phases A and B with the collectives between them; ``_phase_c`` for the two
    trainers of TraversabilityLoss).  A subclass provides the phase calls and, in ``_alloc_extra``, the buffers only it has."""

    GRAD_TAIL = 2     # floats behind the gradient in ``grads``: the two loss sums (RnvpTrainer: 0)
    N_LOSSES = 5      # {total, loss_trav, loss_reco, conf_mean, conf_std} (RnvpTrainer: {loss, conf_mean, conf_std})
    minmax = None     # {max, -min} of the reconstruction loss, exchanged for moving_average by the trainers that allocate it

    def __init__(self, model, lr: float, method: str, process_group):
        if method not in _lib.CONF_METHODS:
            raise ValueError(f"Unknown ConfidenceGenerator method {method!r} (one of {', '.join(_lib.CONF_METHODS)})")
        self.model, self.lr, self.method, self.group = model, lr, method, process_group
        self.step = 0
        self._state_dev = None
        self.comm_events = None   # set to [] to collect (start, end) CUDA-event pairs around the two sum all-reduces of every step

    def _state(self, dev) -> None:
        if self._state_dev == dev:
            return
        n = self.model.flat_params().numel()
        self.grads = torch.zeros(n + self.GRAD_TAIL, dtype=torch.float32, device=dev)
        if self._state_dev is not None:   # change_device in the middle of a mission: moments and statistic move with the model
            self.m, self.v, self.conf_state = self.m.to(dev), self.v.to(dev), self.conf_state.to(dev)
        else:
            self.m = torch.zeros(n, dtype=torch.float32, device=dev)
            self.v = torch.zeros(n, dtype=torch.float32, device=dev)
            self.conf_state = self._initial_conf_state(dev)
        self.stats = torch.zeros(4, dtype=torch.float64, device=dev)
        self.losses = torch.zeros(self.N_LOSSES, dtype=torch.float32, device=dev)
        self._alloc_extra(dev)
        self._state_dev = dev

    def _alloc_extra(self, dev) -> None:
        """Allocate or reset what only the subclass keeps on ``dev`` (called when the state is created or has moved)."""

    def to(self, device) -> "TrainerState":
        """Move the trainer's state after the model has moved (``TraversabilityEstimator.change_device``)."""
        if self._state_dev is not None:
            self._state(torch.device(device))
        return self

    @staticmethod
    def _initial_conf_state(dev) -> torch.Tensor:
        st = torch.zeros(_lib.CONF_STATE_DOUBLES, dtype=torch.float64, device=dev)
        st[_lib.CONF_S_VAR] = 1.0
        st[_lib.CONF_S_STD] = 1.0
        return st

    @torch.no_grad()
    def load_confidence_state(self, cg) -> None:
        """Make the device state equal to a ConfidenceGenerator's (after construction, a load, a reset or a host-side update):
        mean / var / std, the running_mean sums, the moving_average window as per-step sums.  Device copies only."""
        self._state(self.model.flat_params().device)
        st = self.conf_state
        st.zero_()
        st[_lib.CONF_S_MEAN:_lib.CONF_S_MEAN + 1].copy_(cg.mean.detach().reshape(-1))
        st[_lib.CONF_S_VAR:_lib.CONF_S_VAR + 1].copy_(cg.var.detach().reshape(-1))
        st[_lib.CONF_S_STD:_lib.CONF_S_STD + 1].copy_(cg.std.detach().reshape(-1))
        if cg.method == "running_mean":
            for i, name in enumerate(("running_n", "running_sum", "running_sum_of_squares")):
                st[_lib.CONF_S_RUN_N + i:_lib.CONF_S_RUN_N + i + 1].copy_(getattr(cg, name).detach().reshape(-1))
        win = cg.window_sums()[-_lib.CONF_WINDOW:]
        for i, (n, s1, s2) in enumerate(win):
            e = _lib.CONF_S_RING + 3 * i
            st[e] = float(n)
            st[e + 1].copy_(s1)
            st[e + 2].copy_(s2)
        st[_lib.CONF_S_HEAD] = float(len(win) % _lib.CONF_WINDOW)
        st[_lib.CONF_S_FILL] = float(len(win))

    @torch.no_grad()
    def store_confidence_state(self, cg) -> None:
        """The device state into a ConfidenceGenerator's parameters (device copies, no host synchronisation)."""
        st = self.conf_state
        cg.mean.copy_(st[_lib.CONF_S_MEAN:_lib.CONF_S_MEAN + 1])
        cg.var.view(-1).copy_(st[_lib.CONF_S_VAR:_lib.CONF_S_VAR + 1])
        cg.std.copy_(st[_lib.CONF_S_STD:_lib.CONF_S_STD + 1])
        if cg.method == "running_mean":
            cg.running_n.copy_(st[_lib.CONF_S_RUN_N:_lib.CONF_S_RUN_N + 1])
            cg.running_sum.copy_(st[_lib.CONF_S_RUN_SUM:_lib.CONF_S_RUN_SUM + 1])
            cg.running_sum_of_squares.copy_(st[_lib.CONF_S_RUN_SUMSQ:_lib.CONF_S_RUN_SUMSQ + 1])

    # Adam moments in torch.optim.Adam.state_dict() shape, for save/load_checkpoint compatibility
    def optimizer_state_dict(self) -> Dict:
        """``torch.optim.Adam.state_dict()`` shape: empty ``state`` before the first step (as the reference's optimizer),
        and every param-group key ``Adam.load_state_dict`` of current and older torch versions expects."""
        ps = self.model._params_in_order()
        st, off = {}, 0
        if self._state_dev is not None and self.step > 0:
            for i, p in enumerate(ps):
                n = p.numel()
                st[i] = {"step": torch.tensor(float(self.step)), "exp_avg": self.m[off:off + n].view_as(p).clone(),
                         "exp_avg_sq": self.v[off:off + n].view_as(p).clone()}
                off += n
        group = {"lr": self.lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(ps)))}
        return {"state": st, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: Dict) -> None:
        ps = self.model._params_in_order()
        self._state(ps[0].device)
        self.m.zero_()
        self.v.zero_()
        self.step = 0
        off = 0
        for i, p in enumerate(ps):
            n = p.numel()
            if i in sd["state"]:
                self.m[off:off + n] = sd["state"][i]["exp_avg"].reshape(-1).to(self.m.device)
                self.v[off:off + n] = sd["state"][i]["exp_avg_sq"].reshape(-1).to(self.v.device)
                self.step = int(sd["state"][i]["step"])
            off += n
        self.lr = sd["param_groups"][0]["lr"]

    def _timed_allreduce(self, t: torch.Tensor) -> None:
        if self.comm_events is None:
            allreduce_sum_(t, self.group)
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        allreduce_sum_(t, self.group)   # RCCL runs on its own stream; the current stream waits for it, so b brackets it
        b.record()
        self.comm_events.append((a, b))

    def _exchange(self, phase_a, phase_b, launch: bool) -> None:
        """Phases A and B of one step (two callables that enqueue them) with the collectives of the step, in their one order:

            phase A -> SUM of ``stats`` (timed) -> for moving_average MAX of ``minmax`` (untimed) -> phase B -> SUM of ``grads`` (timed)

        Every rank makes this same sequence of collective calls whatever its row count; a rank that made another would leave
        the others hanging in RCCL.  So a rank whose shard is empty this step (ragged frame sharding) takes part in all of them:
        with ``launch`` False it skips both phases and contributes their neutral elements instead (zeros; -inf for the extremes),
        with ``launch`` True its phases are entry points that take zero rows themselves (RnvpTrainer)."""
        moving = self.minmax is not None and self.method == "moving_average"
        if launch:
            phase_a()
        else:
            self.stats.zero_()
            if moving:
                self.minmax.fill_(-float("inf"))
        self._timed_allreduce(self.stats)
        if moving:   # min / max of the reconstruction loss over ALL ranks' rows
            allreduce_max_(self.minmax, self.group)
        if launch:
            phase_b()
        else:
            self.grads.zero_()
        self._timed_allreduce(self.grads)

    def _conf_desc(self) -> Optional[_lib.ConfDesc]:
        """The ConfDesc that phases A, B and C of one MlpTrainer / GcnTrainer step share; None for the original configuration
        (latest_measurement, anomaly_balanced), which keeps its own entry points and no device state."""
        if not self._conf:
            return None
        return _lib.ConfDesc(_lib.CONF_METHODS[self.method], int(self.anomaly_balanced), self.conf_state.data_ptr(),
                             self.minmax.data_ptr())

    def _phase_c(self, cd: Optional[_lib.ConfDesc]) -> torch.Tensor:
        """Adam, the losses and (with a ConfDesc) the commit of the confidence statistic: phase C of MlpTrainer and GcnTrainer."""
        lib, st = _lib.lib(), _lib.stream()
        self.step += 1
        args = (C.byref(self.model.desc), self.model.flat_params().data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                self.v.data_ptr(), self.step, self.lr, self.stats.data_ptr(), self.w_trav, self.w_reco, self.losses.data_ptr())
        if cd is None:
            _lib.check(lib.wvn_mlp_train_phase_c(*args, st), "phase_c")
        else:
            _lib.check(lib.wvn_mlp_train_phase_c_conf(*args, C.byref(cd), st), "phase_c")
        return self.losses


class MlpTrainer(TrainerState):
    def __init__(self, model: SimpleMLP, lr: float = 1e-3, std_factor: float = 0.5, w_trav: float = 0.03,
                 w_reco: float = 0.5, process_group=None, fused: bool = True, method: str = "latest_measurement",
                 anomaly_balanced: bool = True):
        super().__init__(model, lr, method, process_group)
        self.anomaly_balanced = bool(anomaly_balanced)
        # the *_conf entry points (device state) for anything but the original configuration, which keeps its entry points
        self._conf = method != "latest_measurement" or not self.anomaly_balanced
        self.std_factor, self.w_trav, self.w_reco = std_factor, w_trav, w_reco
        self.last_confidence: Optional[torch.Tensor] = None
        # True: the four-launch step of csrc/mlp_train.hip where its geometry applies (256 / 32 hidden units, <= 2048 rows);
        # False: the general path (one kernel per stage, 17-20 launches).  Same arithmetic, other summation orders.
        self.fused = fused

    def _alloc_extra(self, dev):
        self.minmax = torch.zeros(2, dtype=torch.float32, device=dev)
        self.sync_word = torch.zeros(1, dtype=torch.int32, device=dev)   # arrival counter of the fused forward (zero between steps)

    @torch.no_grad()
    def train_step(self, x: torch.Tensor, y: torch.Tensor, y_valid: torch.Tensor,
                   want_confidence: bool = False, rows_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [R,D] fp32, y [R] fp32, y_valid [R] bool (this rank's rows).  Returns the device tensor
        losses[5] = {total, loss_trav, loss_reco, conf_mean, conf_std} (no host sync here).
        ``rows_dev`` (int32 [1] on the device): only the first rows_dev[0] of the R rows are real (a batch compacted by
        ``ops.compact_segment_rows``: its row count never visits the host); the rest contribute nothing."""
        _lib.require_cuda(x, "x")
        lib = _lib.lib()
        dev = x.device
        self._state(dev)
        x = x.float()
        if x.stride(-1) != 1:
            x = x.contiguous()
        y = y.float().contiguous()
        yv = y_valid.to(torch.uint8).contiguous()
        R = x.shape[0]
        d = self.model.desc
        flat = self.model.flat_params()
        ws = self.model._workspace(max(R, 1))
        st = _lib.stream()
        conf = torch.empty(R, dtype=torch.float32, device=dev) if want_confidence else None
        rd = _lib.ptr(rows_dev)
        # one step, two entry-point families: *_conf takes the ConfDesc before the stream, *_rows / phase_c do not know it
        cd = self._conf_desc()
        family, cda = ("_rows", ()) if cd is None else ("_conf", (C.byref(cd),))

        def phase_a():
            _lib.check(getattr(lib, "wvn_mlp_train_phase_a" + family)(
                C.byref(d), flat.data_ptr(), x.data_ptr(), x.stride(0), yv.data_ptr(), R, rd, self.stats.data_ptr(), ws.data_ptr(),
                ws.numel(), self.sync_word.data_ptr() if self.fused else 0, *cda, st), "phase_a")

        def phase_b():
            _lib.check(getattr(lib, "wvn_mlp_train_phase_b" + family)(
                C.byref(d), flat.data_ptr(), x.data_ptr(), x.stride(0), y.data_ptr(), yv.data_ptr(), R, rd, self.stats.data_ptr(),
                self.std_factor, self.w_trav, self.w_reco, self.grads.data_ptr(), _lib.ptr(conf), ws.data_ptr(), ws.numel(),
                int(self.fused), *cda, st), "phase_b")

        self._exchange(phase_a, phase_b, launch=R > 0)
        self.last_confidence = conf
        return self._phase_c(cd)
