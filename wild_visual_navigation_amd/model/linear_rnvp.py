"""LinearRnvp -- wild_visual_navigation/model/linear_rnvp.py:216-296, the anomaly-detection model, with its forward flow on a
HIP kernel (csrc/rnvp.hip).

Same constructor and ``state_dict`` keys as upstream (``prior_mean``, ``prior_var``, ``flows.{0,2}.mask``,
``flows.{0,2}.{s,t}.{0,2,4}.{weight,bias}``, ``flows.{1,3}.{p,invp}``), so its checkpoints load with ``strict=True``, and the
parameters are created in upstream's order, so a seed gives upstream's initial values.  ``forward(Data)`` returns
``{"z", "log_det", "logprob"}``: through the kernel when no gradient is asked for (``eval()`` or ``torch.no_grad()``), through
the torch statement of the same flow (``flow_torch``) when one is.  ``TraversabilityEstimator`` trains it on a GPU device with
``RnvpTrainer`` (csrc/rnvp_train.hip), which works on ``flat_params()`` and never calls ``forward``; on the CPU it trains on autograd.

Built: two coupling layers with separate s and t networks D -> h -> h -> D, each followed by a permutation -- what ``get_model``
builds from ``linear_rnvp_cfg`` -- for D = 384 or 90 and h <= 256, any 0/1 mask with D/2 ones.  Refused by name: ``batch_norm``,
``single_function``, ``conditioning_size``, ``use_permutation=False``, other sizes.
"""
import copy
import ctypes as C
import math
from typing import Optional

import torch

from .. import _lib
from ..utils.data import Data

SUPPORTED_D = (384, 90)


class _Coupling(torch.nn.Module):
    """Affine coupling: the masked columns pass and drive s and t, the others become u * exp(tanh(s)) + t."""

    def __init__(self, input_size: int, mask: torch.Tensor, hidden: int):
        super().__init__()
        self.register_buffer("mask", mask)
        self.s = torch.nn.Sequential(torch.nn.Linear(input_size, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden),
                                     torch.nn.ReLU(), torch.nn.Linear(hidden, input_size))
        self.t = copy.deepcopy(self.s)   # separate parameters, equal initial values

    def forward(self, u):
        mu = u * self.mask
        s = torch.tanh(self.s(mu))
        x = mu + (1 - self.mask) * (u * s.exp() + self.t(mu))
        return x, ((1 - self.mask) * s).sum(1)


class _Permutation(torch.nn.Module):
    def __init__(self, n: int):
        super().__init__()
        self.register_buffer("p", torch.randperm(n))
        self.register_buffer("invp", torch.argsort(self.p))

    def forward(self, x):
        return x[:, self.p], 0


class LinearRnvp(torch.nn.Module):
    PER_PIXEL_FP32_TOKENS = True   # FeatureExtractor: forward_per_pixel_exact on the backbone's fp32 tokens, every precision

    def __init__(self, input_size, coupling_topology, flow_n=2, use_permutation=False, batch_norm=False, mask_type="odds",
                 conditioning_size=None, single_function=False, **kwargs):
        super().__init__()
        if batch_norm:
            raise ValueError("batch_norm=True is not implemented for LinearRnvp on the MI355X path")
        if single_function:
            raise ValueError("single_function=True is not implemented for LinearRnvp on the MI355X path (separate s and t networks only)")
        if conditioning_size:
            raise ValueError(f"conditioning_size={conditioning_size} is not implemented for LinearRnvp on the MI355X path (0 only)")
        if not use_permutation:
            raise ValueError("use_permutation=False is not implemented for LinearRnvp on the MI355X path")
        if flow_n != 2:
            raise ValueError(f"flow_n={flow_n} is not implemented for LinearRnvp on the MI355X path (2 only)")
        if input_size not in SUPPORTED_D:
            raise ValueError(f"input_size={input_size} is not implemented for LinearRnvp on the MI355X path (one of {SUPPORTED_D})")
        topo = list(coupling_topology) if coupling_topology is not None else []
        if len(topo) != 1 or not 1 <= int(topo[0]) <= 256:
            raise ValueError(f"coupling_topology={coupling_topology} is not implemented for LinearRnvp on the MI355X path "
                             "(one hidden size h <= 256: networks D -> h -> h -> D)")
        if mask_type == "odds":
            mask = torch.arange(0, input_size).float() % 2
        elif mask_type == "half":
            mask = torch.zeros(input_size)
            mask[: input_size // 2] = 1
        else:
            raise ValueError(f"mask_type={mask_type!r} is not one of 'odds', 'half'")
        self.input_size, self.hidden = input_size, int(topo[0])
        self.register_buffer("prior_mean", torch.zeros(input_size))
        self.register_buffer("prior_var", torch.ones(input_size))   # used as the scale of the normal prior, as upstream does
        blocks = []
        for _ in range(flow_n):
            blocks += [_Coupling(input_size, mask, self.hidden), _Permutation(input_size)]
        self.flows = torch.nn.Sequential(*blocks)
        self.desc = _lib.RnvpDesc(input_size, self.hidden, flow_n)
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self._flat: Optional[torch.Tensor] = None

    # ---- the torch statement of the flow (autograd) ----------------------------------------------------
    def flow_torch(self, x: torch.Tensor):
        """(z, log_det, logprob [R, D]) as differentiable torch ops."""
        log_det = 0
        for block in self.flows:
            x, ld = block(x)
            log_det = log_det + ld
        return x, log_det, torch.distributions.Normal(self.prior_mean, self.prior_var).log_prob(x)

    # ---- packed weights for the kernel -----------------------------------------------------------------
    def _state_tensors(self):
        out = []
        for i in (0, 2):
            c = self.flows[i]
            out += [p for net in (c.s, c.t) for k in (0, 2, 4) for p in (net[k].weight, net[k].bias)]
        return out

    _params_in_order = _state_tensors   # ``model.parameters()`` order: the layout of the flat buffer, gradient and Adam moments

    def flat_params(self) -> torch.Tensor:
        """One flat fp32 buffer that the 24 parameters alias (RnvpTrainer's Adam kernel and gradient all-reduce work on it);
        re-established when ``.to()`` or a load has broken the aliasing."""
        ps = self._state_tensors()
        ok = self._flat is not None and self._flat.device == ps[0].device
        if ok:
            off = 0
            for p in ps:
                if p.data_ptr() != self._flat.data_ptr() + 4 * off or not p.is_contiguous():
                    ok = False
                    break
                off += p.numel()
        if not ok:
            flat = torch.cat([p.detach().reshape(-1).float() for p in ps]).contiguous()
            off = 0
            for p in ps:
                p.data = flat[off: off + p.numel()].view_as(p)
                off += p.numel()
            self._flat = flat
        return self._flat

    def _pack_key(self):
        params = self._state_tensors()
        others = [self.flows[0].mask, self.flows[2].mask, self.flows[1].p, self.flows[3].p, self.prior_mean, self.prior_var]
        return tuple((t.data_ptr(), t._version) for t in params + others)

    def pack(self) -> torch.Tensor:
        """The kernel's weight images, rebuilt when a parameter, mask, permutation or the device has changed since the last
        call (in-place updates -- optimizer steps, ``load_state_dict`` -- move a tensor's version counter; RnvpTrainer's kernels
        do not, and re-pack the images themselves)."""
        key = self._pack_key()
        if self._packed is not None and key == self._packed_key:
            return self._packed
        params = self._state_tensors()
        dev = params[0].device
        _lib.require_cuda(params[0], "parameters")
        masks = torch.stack([self.flows[0].mask, self.flows[2].mask]).float().contiguous()
        perms = torch.stack([self.flows[1].p, self.flows[3].p]).long().contiguous()
        D = self.input_size
        # (one host read per re-pack: a malformed mask or prior would otherwise give silently different numbers)
        ok = torch.stack([((masks == 0) | (masks == 1)).all(), (masks.sum(1) == D // 2).all(),
                          (perms.sort(1).values == torch.arange(D, device=dev)).all(),
                          (self.prior_mean == 0).all(), (self.prior_var == 1).all()]).tolist()
        if not (ok[0] and ok[1]):
            raise _lib.WvnError(f"mask must hold zeros and ones with exactly {D // 2} ones per coupling layer")
        if not ok[2]:
            raise _lib.WvnError("p is not a permutation of the columns")
        if not (ok[3] and ok[4]):
            raise _lib.WvnError("prior_mean / prior_var other than 0 / 1 are not implemented (the kernel scores against the unit normal)")
        h = _lib.lib()
        n = h.wvn_rnvp_pack_bytes(C.byref(self.desc))
        if n == 0:
            raise _lib.WvnError(f"the LinearRnvp kernel is built for D in {SUPPORTED_D} and h <= 256, got D = {D}, h = {self.hidden}")
        flat = torch.cat([p.detach().reshape(-1).float() for p in params]).contiguous()
        if self._packed is None or self._packed.device != dev or self._packed.numel() != n:
            self._packed = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.check(h.wvn_rnvp_pack(C.byref(self.desc), flat.data_ptr(), masks.data_ptr(), perms.data_ptr(), self._packed.data_ptr(),
                                   _lib.stream()), "wvn_rnvp_pack")
        self._packed_key = key
        return self._packed

    @staticmethod
    def _conf_ptr(conf_state):
        if conf_state is None:
            return 0
        _lib.require_cuda(conf_state, "conf_state")
        if conf_state.dtype != torch.float32 or conf_state.numel() < 3 or not conf_state.is_contiguous():
            raise _lib.WvnError("conf_state must be a contiguous fp32 device tensor {mean, std, std_factor}")
        return conf_state.data_ptr()

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor, want_z: bool = True, want_conf: bool = False, mean: float = 0.0, std: float = 1.0,
                     std_factor: float = 0.5, conf_state: Optional[torch.Tensor] = None):
        """The kernel on rows ``x`` [R, >= D] fp32 -> (score [R], log_det [R], z [R, D] | None, conf [R] | None);
        score = logprob.sum(1) + log_det, conf = confidence(-score)."""
        _lib.require_cuda(x, "x")
        D = self.input_size
        if x.dim() != 2 or x.shape[1] < D or x.shape[0] < 1:
            raise _lib.WvnError(f"x must be [R >= 1, >= {D}], got {tuple(x.shape)}")
        x = x.float()
        if x.stride(1) != 1 or x.stride(0) < D:
            x = x.contiguous()
        packed = self.pack()
        R = x.shape[0]
        score = torch.empty(R, dtype=torch.float32, device=x.device)
        log_det = torch.empty_like(score)
        z = torch.empty(R, D, dtype=torch.float32, device=x.device) if want_z else None
        conf = torch.empty_like(score) if want_conf else None
        rc = _lib.lib().wvn_rnvp_forward_rows(C.byref(self.desc), packed.data_ptr(), x.data_ptr(), x.stride(0), R, float(mean),
                                              float(std), float(std_factor), self._conf_ptr(conf_state), score.data_ptr(),
                                              _lib.ptr(conf), log_det.data_ptr(), _lib.ptr(z), D, _lib.stream())
        _lib.check(rc, "wvn_rnvp_forward_rows")
        return score, log_det, z, conf

    def forward(self, data: Data):
        x = data.x
        if self.training and torch.is_grad_enabled():
            z, log_det, logprob = self.flow_torch(x)
        else:
            _, log_det, z, _ = self.forward_rows(x)
            logprob = -0.5 * z * z - 0.5 * math.log(2 * math.pi)
        return {"z": z, "log_det": log_det, "logprob": logprob}

    # ---- live-frame inference ----------------------------------------------------------------------------
    @torch.no_grad()
    def forward_per_pixel_exact(self, tokens: torch.Tensor, batch: int, grid: int, out_hw, mean: float = 0.0, std: float = 1.0,
                                std_factor: float = 0.5, want_loss: bool = False, conf_state: Optional[torch.Tensor] = None,
                                want_z: bool = False):
        """What the live node computes with prediction_per_pixel in this mode -- up-sample, flow, confidence(-score) -- from the
        PATCH tokens, without the dense feature tensor: ``tokens`` [batch*grid*grid, >= D] fp32 ->
        (trav, conf, -score | None) [batch, H, W] fp32 with trav = conf (and z [batch*H*W, D] behind them with ``want_z``)."""
        _lib.require_cuda(tokens, "tokens")
        D = self.input_size
        if tokens.dtype != torch.float32 or tokens.dim() != 2 or tokens.shape[0] != batch * grid * grid or tokens.stride(1) != 1 \
                or tokens.shape[1] < D:
            raise _lib.WvnError(f"tokens must be fp32 [batch*grid*grid, >= {D}], got {tuple(tokens.shape)} {tokens.dtype}")
        packed = self.pack()
        H, W = out_hw
        score = torch.empty(batch, H, W, dtype=torch.float32, device=tokens.device)
        conf = torch.empty_like(score)
        z = torch.empty(batch * H * W, D, dtype=torch.float32, device=tokens.device) if want_z else None
        rc = _lib.lib().wvn_rnvp_forward_pixels(C.byref(self.desc), packed.data_ptr(), tokens.data_ptr(), tokens.stride(0), batch,
                                                grid, H, W, float(mean), float(std), float(std_factor), self._conf_ptr(conf_state),
                                                score.data_ptr(), conf.data_ptr(), 0, _lib.ptr(z), D, _lib.stream())
        _lib.check(rc, "wvn_rnvp_forward_pixels")
        out = (conf, conf, score.neg_() if want_loss else None)
        return out + (z,) if want_z else out

    @torch.no_grad()
    def forward_per_segment(self, feat: torch.Tensor, seg: torch.Tensor, mean: float = 0.0, std: float = 1.0,
                            std_factor: float = 0.5, want_loss: bool = False, conf_state: Optional[torch.Tensor] = None):
        """The same per segment: the flow once per row of ``feat`` [S, D] or [B, S, D], then ``values[seg]`` with torch's id rule
        (ids in [-S, 0) wrap; any other id outside [0, S) gives NaN) -> (trav, conf, -score | None) with the shape of ``seg``."""
        _lib.require_cuda(feat, "feat")
        _lib.require_cuda(seg, "seg")
        D = self.input_size
        if feat.dtype != torch.float32 or feat.dim() not in (2, 3) or feat.shape[-1] < D:
            raise _lib.WvnError(f"feat must be fp32 [S, >= {D}] or [B, S, >= {D}], got {tuple(feat.shape)} {feat.dtype}")
        if seg.dtype not in (torch.int32, torch.int64) or seg.dim() not in (2, 3):
            raise _lib.WvnError(f"seg must be int32 / int64 [H, W] or [B, H, W], got {tuple(seg.shape)} {seg.dtype}")
        f3 = feat if feat.dim() == 3 else feat[None]
        s3 = seg if seg.dim() == 3 else seg[None]
        if f3.shape[0] != s3.shape[0]:
            raise _lib.WvnError(f"feat and seg hold different numbers of frames: {tuple(feat.shape)} vs {tuple(seg.shape)}")
        B, S = f3.shape[0], f3.shape[1]
        score, _, _, conf = self.forward_rows(f3.reshape(B * S, f3.shape[2]), want_z=False, want_conf=True, mean=mean, std=std,
                                              std_factor=std_factor, conf_state=conf_state)
        ids = s3.reshape(B, -1).long()
        ids = torch.where(ids < 0, ids + S, ids)
        bad = (ids < 0) | (ids >= S)
        ids = ids.clamp(0, S - 1)

        def paint(v):
            return torch.gather(v.view(B, S), 1, ids).masked_fill_(bad, float("nan")).view(seg.shape)

        conf_map = paint(conf)
        return conf_map, conf_map, paint(score).neg_() if want_loss else None
