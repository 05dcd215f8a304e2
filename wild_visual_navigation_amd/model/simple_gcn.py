"""SimpleGCN -- wild_visual_navigation/model/simple_gcn.py on HIP kernels (csrc/simple_gcn.hip).

Three graph-convolution layers D -> h1 (ReLU) -> h2 (ReLU) -> 1 + D with the sigmoid on column 0: SimpleMLP's ``[N, 1 + D]``
contract (traversability in column 0, the reconstruction behind it), so the loss, the confidence generator and the per-segment
table apply unchanged.  Upstream's file cannot run as shipped (its ``GCNConv`` import is commented out); a layer here is the
published, closed-form definition of ``torch_geometric.nn.GCNConv`` with its defaults (``add_self_loops``, ``normalize``, not
``improved``, aggregation "add", flow source -> target) on ``x [N, K]``, ``edge_index [2, E]`` (row 0 = source j, row 1 = target i):

    1. every edge with j == i is dropped, then one self loop per node is added; duplicate edges stay duplicated
    2. deg_i = number of edges into i (>= 1);  3. coef_e = deg_j^-1/2 deg_i^-1/2;  4. out_i = sum_{e: j->i} coef_e (x_j W^T) + b

The edge list is used as given (not symmetrised).  ``state_dict`` keys are PyG's (``layers.{0,1,2}.bias``,
``layers.{0,1,2}.lin.weight`` [out, in]); glorot-uniform weights, zero bias.  The six tensors are views into ONE flat fp32 buffer
[W1|b1|W2|b2|W3|b3], SimpleMLP's layout for the same (D, h1, h2).  Parity with the ``torch_geometric`` package itself is not
pinned (it is not a dependency here): tests/simple_gcn_ref.py states the definition in float64.

Training: ``forward`` returns the plain-torch statement whenever a gradient is asked for (autograd, CPU or GPU); the optimisation
step of ``TraversabilityEstimator`` on a GPU device does not go through it but through the fused HIP phases of
``traversability_estimator/gcn_trainer.py`` (csrc/simple_gcn_train.hip), on this model's flat buffer.
"""
import ctypes as C
import math
from typing import List, Optional

import torch

from .. import _lib
from ..utils.data import Data
from .simple_mlp import SimpleMLP


def gcn_conv_torch(x: torch.Tensor, edge_index: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """One layer as plain, differentiable torch (any device, any float dtype): the statement the training forward runs."""
    N = x.shape[0]
    src, dst = edge_index[0].long(), edge_index[1].long()
    keep = (src != dst) & (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    loop = torch.arange(N, device=x.device)
    src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    deg = torch.zeros(N, dtype=x.dtype, device=x.device).index_add_(0, dst, torch.ones(dst.shape[0], dtype=x.dtype, device=x.device))
    dinv = deg.pow(-0.5)
    xw = x @ weight.t()
    out = torch.zeros(N, weight.shape[0], dtype=x.dtype, device=x.device).index_add_(0, dst, xw[src] * (dinv[src] * dinv[dst])[:, None])
    return out + bias


class _GCNConv(torch.nn.Module):
    """Parameter holder with GCNConv's names: ``lin.weight`` [out, in] (glorot uniform), ``bias`` [out] (zeros)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        a = math.sqrt(6.0 / (in_channels + out_channels))
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)

    def forward(self, x, edge_index):
        return gcn_conv_torch(x, edge_index, self.lin.weight, self.bias)


class SimpleGCN(torch.nn.Module):
    NEEDS_GRAPH = True   # FeatureExtractor.predict_per_segment hands forward_per_segment the batched adjacency bitmaps

    def __init__(self, input_size: int = 64, reconstruction: bool = True, hidden_sizes: List[int] = [255]):
        super().__init__()
        hidden_sizes = list(hidden_sizes)
        if len(hidden_sizes) != 3 or hidden_sizes[-1] != 1 or not reconstruction:
            raise ValueError("the MI355X path implements SimpleGCN(D, reconstruction=True, hidden_sizes=[h1, h2, 1])")
        h1, h2 = hidden_sizes[0], hidden_sizes[1]
        if not (1 <= input_size <= 1024 and 1 <= h1 <= 256 and 1 <= h2 <= 256):
            raise ValueError(f"the MI355X path implements SimpleGCN(D <= 1024, hidden_sizes=[h1 <= 256, h2 <= 256, 1]), got D = {input_size}, "
                             f"hidden_sizes = {hidden_sizes}")
        self.nr_sigmoid_layers = hidden_sizes[-1]
        self.input_size = input_size
        self.output_features = 1 + input_size
        self.layers = torch.nn.ModuleList([_GCNConv(input_size, h1), _GCNConv(h1, h2), _GCNConv(h2, self.output_features)])
        self.desc = _lib.MlpDesc(input_size, h1, h2, 0)
        self._flat: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._bad: Optional[torch.Tensor] = None

    # ---- flat parameter storage --------------------------------------------------------------------
    def _params_in_order(self):
        return [p for layer in self.layers for p in (layer.lin.weight, layer.bias)]

    flat_params = SimpleMLP.flat_params   # (works on _params_in_order / _flat)

    @property
    def bad_edges(self) -> Optional[torch.Tensor]:
        """Device int32 [1]: the edges the last graph preparation dropped because an endpoint lay outside [0, N) (None before the
        first HIP forward).  Reading it is the caller's host synchronisation, not the forward's."""
        return self._bad

    # ---- the plain-torch statement (autograd, CPU or GPU; the CPU estimator trains on it) -----------------------------------
    def forward_torch(self, x: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        h = torch.relu(self.layers[0](x, edge_index))
        h = torch.relu(self.layers[1](h, edge_index))
        o = self.layers[2](h, edge_index)
        return torch.cat([torch.sigmoid(o[:, :1]), o[:, 1:]], dim=1)

    # ---- HIP path -------------------------------------------------------------------------------------
    def _prepare(self, dev, nodes: int, capacity: int):
        h = _lib.lib()
        need = h.wvn_gcn_workspace_bytes(C.byref(self.desc), nodes, capacity)
        if need == 0:
            raise _lib.WvnError(f"SimpleGCN on HIP needs 1 <= nodes <= 2^26 and at most 2^30 neighbour entries, got {nodes} and {capacity}")
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if self._bad is None or self._bad.device != dev:
            self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        flat = self.flat_params()
        _lib.require_cuda(flat, "parameters")
        return h, flat

    def _graph_from_edges(self, h, edge_index: torch.Tensor, nodes: int, capacity: int):
        E = edge_index.shape[1]
        rc = h.wvn_gcn_graph_from_edges(edge_index.data_ptr() if E else 0, edge_index.stride(0), edge_index.stride(1), E, nodes, capacity,
                                        self._bad.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream())
        _lib.check(rc, "wvn_gcn_graph_from_edges")

    @staticmethod
    def _check_edges(edge_index: torch.Tensor, name: str) -> torch.Tensor:
        _lib.require_cuda(edge_index, name)
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise _lib.WvnError(f"{name} must be [2, E], got {tuple(edge_index.shape)}")
        return edge_index if edge_index.dtype == torch.int64 else edge_index.long()

    def forward(self, data: Data) -> torch.Tensor:
        x, edge_index = data.x, data.edge_index
        if self.training and torch.is_grad_enabled():
            return self.forward_torch(x, edge_index)
        _lib.require_cuda(x, "data.x")
        edge_index = self._check_edges(edge_index, "data.edge_index")
        x = x.float()
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < self.input_size:
            raise _lib.WvnError(f"data.x must be [N >= 1, >= {self.input_size}], got {tuple(x.shape)}")
        if x.stride(1) != 1 or x.stride(0) < self.input_size:
            x = x.contiguous()
        N, cap = x.shape[0], edge_index.shape[1] + x.shape[0]
        h, flat = self._prepare(x.device, N, cap)
        self._graph_from_edges(h, edge_index, N, cap)
        out = torch.empty(N, self.output_features, dtype=torch.float32, device=x.device)
        rc = h.wvn_gcn_forward(C.byref(self.desc), flat.data_ptr(), x.data_ptr(), x.stride(0), N, cap, out.data_ptr(),
                               self._ws.data_ptr(), self._ws.numel(), _lib.stream())
        _lib.check(rc, "wvn_gcn_forward")
        return out

    # ---- fused per-pixel inference: a pixel has no graph here ------------------------------------------
    def _no_per_pixel(self, *args, **kwargs):
        raise _lib.WvnError("fused per-pixel inference is not implemented for SimpleGCN (per-pixel graphs are out of scope); "
                            "use forward_per_segment / predict_per_segment")

    pack_per_pixel = forward_per_pixel = forward_per_pixel_exact = _no_per_pixel

    # ---- fused per-segment inference ------------------------------------------------------------------
    @torch.no_grad()
    def forward_per_segment(self, feat: torch.Tensor, seg: torch.Tensor, mean: float = 0.0, std: float = 1.0,
                            std_factor: float = 0.5, want_loss: bool = False, conf_state: Optional[torch.Tensor] = None,
                            edges: Optional[torch.Tensor] = None, adjacency: Optional[torch.Tensor] = None):
        """``SimpleMLP.forward_per_segment`` for this model (same shapes, id rule and outputs) on the segment graph: ``edges``
        [2, E] int64 (single frame: ``extract()``'s edges, left id = source, right id = target) or ``adjacency`` [B, S, S] uint8
        (``ops.seg_adjacency_batched``: adj[b, l, r] != 0 is an edge l -> r of frame b; node id b * S + s).  The three layers run
        once per segment row, the last one fills the {trav, conf, loss_reco} table, the paint kernel spreads it."""
        _lib.require_cuda(feat, "feat")
        _lib.require_cuda(seg, "seg")
        D = self.input_size
        if (edges is None) == (adjacency is None):
            raise _lib.WvnError("SimpleGCN.forward_per_segment needs the segment graph: edges [2, E] (single frame) or adjacency [B, S, S], one of them")
        if feat.dtype != torch.float32 or feat.dim() not in (2, 3) or feat.shape[-1] < D:
            raise _lib.WvnError(f"feat must be fp32 [S, >= {D}] or [B, S, >= {D}], got {tuple(feat.shape)} {feat.dtype}")
        if seg.dtype not in (torch.int32, torch.int64) or seg.dim() not in (2, 3):
            raise _lib.WvnError(f"seg must be int32 / int64 [H, W] or [B, H, W], got {tuple(seg.shape)} {seg.dtype}")
        f3 = feat if feat.dim() == 3 else feat[None]
        s3 = seg if seg.dim() == 3 else seg[None]
        if f3.shape[0] != s3.shape[0]:
            raise _lib.WvnError(f"feat and seg hold different numbers of frames: {tuple(feat.shape)} vs {tuple(seg.shape)}")
        B, S = f3.shape[0], f3.shape[1]
        if f3.stride(2) != 1 or f3.stride(1) < D or (B > 1 and f3.stride(0) != S * f3.stride(1)):
            f3 = f3.contiguous()
        s3 = s3.contiguous()
        if conf_state is not None:
            _lib.require_cuda(conf_state, "conf_state")
            if conf_state.dtype != torch.float32 or conf_state.numel() < 3 or not conf_state.is_contiguous():
                raise _lib.WvnError("conf_state must be a contiguous fp32 device tensor {mean, std, std_factor}")
        H, W = s3.shape[1], s3.shape[2]
        if edges is not None:
            if B != 1:
                raise _lib.WvnError(f"edges describe one frame, got {B} frames: pass adjacency [B, S, S] for a batch")
            edges = self._check_edges(edges, "edges")
            cap = edges.shape[1] + S
            h, flat = self._prepare(feat.device, S, cap)
            self._graph_from_edges(h, edges, S, cap)
        else:
            _lib.require_cuda(adjacency, "adjacency")
            if adjacency.dtype not in (torch.uint8, torch.bool) or tuple(adjacency.shape) != (B, S, S):
                raise _lib.WvnError(f"adjacency must be uint8 [{B}, {S}, {S}], got {tuple(adjacency.shape)} {adjacency.dtype}")
            if any(st < 0 for st in adjacency.stride()):
                adjacency = adjacency.contiguous()
            cap = B * S * S
            h, flat = self._prepare(feat.device, B * S, cap)
            rc = h.wvn_gcn_graph_from_bitmaps(adjacency.data_ptr(), adjacency.stride(0), adjacency.stride(1), adjacency.stride(2), B, S, cap,
                                              self._bad.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream())
            _lib.check(rc, "wvn_gcn_graph_from_bitmaps")
        trav = torch.empty(seg.shape, dtype=torch.float32, device=seg.device)
        conf = torch.empty_like(trav)
        loss = torch.empty_like(trav) if want_loss else None
        rc = h.wvn_gcn_segment_predict(C.byref(self.desc), flat.data_ptr(), f3.data_ptr(), f3.stride(1), B, S, cap, s3.data_ptr(),
                                       s3.element_size(), H, W, float(mean), float(std), float(std_factor),
                                       conf_state.data_ptr() if conf_state is not None else 0, trav.data_ptr(), conf.data_ptr(),
                                       loss.data_ptr() if want_loss else 0, self._ws.data_ptr(), self._ws.numel(), _lib.stream())
        _lib.check(rc, "wvn_gcn_segment_predict")
        return trav, conf, loss
