"""One optimisation step of the anomaly-detection model (LinearRnvp, AnomalyLoss: loss = -mean(score), Adam) on HIP kernels
(csrc/rnvp_train.hip), data-parallel with the two exchanges of the traversability MLPs' step (trainer.py):

    phase A  forward with saved activations + LOCAL statistic {n, sum x, sum x^2, n} of x = -score  (fp64)
       -> all-reduce(sum) of 4 doubles          (the loss normaliser and the confidence statistic are GLOBAL)
    phase B  backward + weight gradients -> flat gradient fp32 in ``model.parameters()`` order
       -> all-reduce(sum) of 3.1 MB (D = 384, h = 200) / 1.2 MB (D = 90)
    phase C  Adam, loss, commit of the confidence statistic, re-pack of the kernel images; every rank applies the identical
             update, so replicas stay bit-identical

Local contributions are sums scaled by the global 1/N inside phase B, so the N-rank trajectory equals the one-rank trajectory on
the concatenated rows up to fp32 summation order.  Every row is a positive in this mode; the per-row training confidence that
``ConfidenceGenerator.update`` returns is not produced.
"""
import ctypes as C

import torch

from .. import _lib
from ..model.linear_rnvp import LinearRnvp
from .trainer import TrainerState


class RnvpTrainer(TrainerState):
    GRAD_TAIL = 0   # no loss sums behind the gradient: the loss is the statistic's mean
    N_LOSSES = 3
    _conf = True    # the confidence statistic always lives in ``conf_state`` (phase C commits it for every method)

    def __init__(self, model: LinearRnvp, lr: float = 1e-3, method: str = "latest_measurement", process_group=None):
        super().__init__(model, lr, method, process_group)
        self._ws = None
        self._tpacked = None
        self._tpacked_key = None
        self.last_score = None    # phase A's score of the last step's rows (device)

    def _alloc_extra(self, dev):
        self._ws = self._tpacked = self._tpacked_key = None

    def _images(self):
        """(forward blob, transposed images) for the model's current parameters; the stacked masks and permutations phase C re-packs
        from are kept beside them."""
        model, lib = self.model, _lib.lib()
        flat = model.flat_params()
        packed = model.pack()
        if self._tpacked is None or self._tpacked.device != flat.device or self._tpacked_key != model._packed_key:
            n = lib.wvn_rnvp_train_pack_bytes(C.byref(model.desc))
            if n == 0:
                raise _lib.WvnError(f"the LinearRnvp training kernels are built for D in (384, 90) and h <= 256, got D = "
                                    f"{model.input_size}, h = {model.hidden}")
            if self._tpacked is None or self._tpacked.device != flat.device:
                self._tpacked = torch.empty(n, dtype=torch.uint8, device=flat.device)
            self._masks = torch.stack([model.flows[0].mask, model.flows[2].mask]).float().contiguous()
            self._perms = torch.stack([model.flows[1].p, model.flows[3].p]).long().contiguous()
            _lib.check(lib.wvn_rnvp_train_pack(C.byref(model.desc), flat.data_ptr(), packed.data_ptr(), self._tpacked.data_ptr(),
                                               _lib.stream()), "wvn_rnvp_train_pack")
            self._tpacked_key = model._packed_key
        return packed, self._tpacked

    def _workspace(self, R: int) -> torch.Tensor:
        need = _lib.lib().wvn_rnvp_train_workspace_bytes(C.byref(self.model.desc), R)
        if need == 0:
            raise _lib.WvnError(f"no LinearRnvp training workspace for {R} rows (at most 65536 per rank and step)")
        if self._ws is None or self._ws.numel() < need or self._ws.device != self._state_dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self._state_dev)
        return self._ws

    @torch.no_grad()
    def forward_backward(self, x: torch.Tensor) -> torch.Tensor:
        """Phases A and B on this rank's rows x [R, >= D] (R may be 0), with both all-reduces: the flat gradient of
        -mean(score) over all ranks' rows, in ``model.parameters()`` order."""
        _lib.require_cuda(x, "x")
        lib, model = _lib.lib(), self.model
        D = model.input_size
        if x.dim() != 2 or x.shape[1] < D:
            raise _lib.WvnError(f"x must be [R, >= {D}], got {tuple(x.shape)}")
        self._state(x.device)
        x = x.float()
        if x.shape[0] and (x.stride(1) != 1 or x.stride(0) < D):
            x = x.contiguous()
        R = x.shape[0]
        packed, tpacked = self._images()
        ws, st = self._workspace(R), _lib.stream()
        score = torch.empty(R, dtype=torch.float32, device=x.device)

        def phase_a():
            _lib.check(lib.wvn_rnvp_train_phase_a(C.byref(model.desc), packed.data_ptr(), x.data_ptr() if R else 0, x.stride(0) if R else D,
                                                  R, score.data_ptr() if R else 0, self.stats.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       "wvn_rnvp_train_phase_a")

        def phase_b():
            _lib.check(lib.wvn_rnvp_train_phase_b(C.byref(model.desc), packed.data_ptr(), tpacked.data_ptr(), R, self.stats.data_ptr(),
                                                  self.grads.data_ptr(), ws.data_ptr(), ws.numel(), st), "wvn_rnvp_train_phase_b")

        self._exchange(phase_a, phase_b, launch=True)   # the entry points take an empty shard (R = 0) themselves
        self.last_score = score
        return self.grads

    @torch.no_grad()
    def train_step(self, x: torch.Tensor) -> torch.Tensor:
        """One step on this rank's rows.  Returns the device tensor losses[3] = {loss, confidence mean, confidence std}
        (no host synchronisation here)."""
        self.forward_backward(x)
        lib, model = _lib.lib(), self.model
        flat = model.flat_params()
        self.step += 1
        _lib.check(lib.wvn_rnvp_train_phase_c(C.byref(model.desc), flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(),
                                              self.v.data_ptr(), self.step, self.lr, self.stats.data_ptr(),
                                              _lib.CONF_METHODS[self.method], self.conf_state.data_ptr(), self.losses.data_ptr(),
                                              self._masks.data_ptr(), self._perms.data_ptr(), model._packed.data_ptr(),
                                              self._tpacked.data_ptr(), _lib.stream()), "wvn_rnvp_train_phase_c")
        # phase C has re-packed both images for the new parameters; a kernel's in-place update does not move a tensor's
        # _version, so the cache keys are set to the parameters as they are now
        model._packed_key = model._pack_key()
        self._tpacked_key = model._packed_key
        return self.losses
