"""DoubleMLP -- wild_visual_navigation/model/simple_mlp.py:42-67 on HIP kernels (csrc/double_mlp.hip).

Two independent three-layer networks that share only the input: ``networks.0`` D -> h1 -> h2 -> 1 (sigmoid) and ``networks.1``
D -> h1 -> h2 -> D.  Same constructor and ``state_dict`` keys (``networks.{0,1}.{0,2,4}.{weight,bias}``) as upstream, same
``forward(Data)`` contract as SimpleMLP ([R, 1+D], sigmoid traversability in column 0, the reconstruction behind it), so the loss,
the confidence generator, the trainer, the weights hand-off and the checkpoints apply unchanged.  The twelve parameter tensors are
views into ONE flat fp32 buffer [W1a|b1a|W2a|b2a|W3a|b3a|W1b|b1b|W2b|b2b|W3b|b3b] (a = networks.0, b = networks.1), which is
``torch.optim.Adam``'s parameter order.
"""
import ctypes as C
from typing import List, Optional

import torch

from .. import _lib
from .simple_mlp import SimpleMLP


class DoubleMLP(torch.nn.Module):
    def __init__(self, input_size: int = 64, hidden_sizes: List[int] = [255]):
        super().__init__()
        hidden_sizes = list(hidden_sizes)
        if len(hidden_sizes) != 3 or hidden_sizes[-1] != 1:
            raise ValueError("the MI355X path implements DoubleMLP(D, [h1, h2, 1])")
        h1, h2 = hidden_sizes[0], hidden_sizes[1]
        if not (1 <= input_size <= 1024 and 1 <= h1 <= 256 and 1 <= h2 <= 256):
            raise ValueError(f"the MI355X path implements DoubleMLP(D <= 1024, [h1 <= 256, h2 <= 256, 1]), got D = {input_size}, "
                             f"hidden_sizes = {hidden_sizes}")
        self.nr_sigmoid_layers = hidden_sizes[-1]
        self.input_size = input_size
        networks = []
        for last in (hidden_sizes[-1], input_size):
            layers, i = [], input_size
            for hs in hidden_sizes[:-1]:
                layers += [torch.nn.Linear(i, hs), torch.nn.ReLU()]
                i = hs
            layers.append(torch.nn.Linear(i, last))
            networks.append(torch.nn.Sequential(*layers))
        self.networks = torch.nn.ModuleList(networks)
        self.output_features = hidden_sizes[-1] + input_size
        self.desc = _lib.MlpDesc(input_size, h1, h2, _lib.MLP_KIND_DOUBLE)
        self._flat: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._seg_ws: Optional[torch.Tensor] = None

    # ---- flat parameter storage --------------------------------------------------------------------
    def _params_in_order(self):
        return [p for net in self.networks for i in (0, 2, 4) for p in (net[i].weight, net[i].bias)]

    flat_params = SimpleMLP.flat_params   # (works on _params_in_order / _flat)

    def _workspace(self, rows: int) -> torch.Tensor:
        need = _lib.lib().wvn_mlp_workspace_bytes(C.byref(self.desc), rows)
        dev = self.networks[0][0].weight.device
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    # ---- forward: one launch, x is read once for both networks ---------------------------------------
    forward = SimpleMLP.forward

    # ---- fused per-pixel inference: not built for this model ------------------------------------------
    def _no_per_pixel(self, *args, **kwargs):
        raise _lib.WvnError("fused per-pixel inference is not implemented for DoubleMLP (csrc/pixel_mlp.hip runs SimpleMLP only); "
                            "use forward_per_segment / predict_per_segment, or SimpleMLP")

    pack_per_pixel = forward_per_pixel = forward_per_pixel_exact = _no_per_pixel

    # ---- fused per-segment inference ------------------------------------------------------------------
    @torch.no_grad()
    def forward_per_segment(self, feat: torch.Tensor, seg: torch.Tensor, mean: float = 0.0, std: float = 1.0,
                            std_factor: float = 0.5, want_loss: bool = False, conf_state: Optional[torch.Tensor] = None):
        """``SimpleMLP.forward_per_segment`` for this model (same arguments, id rule and outputs): the pair runs once per segment
        row (csrc/double_mlp.hip), the results are painted onto the map (csrc/segment_predict.hip)."""
        return SimpleMLP.forward_per_segment(self, feat, seg, mean, std, std_factor, want_loss=want_loss, conf_state=conf_state)
