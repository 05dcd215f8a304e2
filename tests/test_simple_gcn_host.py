"""SimpleGCN without a GPU: config, registry, state dict, the training-mode torch statement and its autograd gradients against the
float64 statement of the definition (tests/simple_gcn_ref.py), refusals, host-only workspace queries.

Measured on the CPU (2^-16 x max|.| = 1.5e-05 x max|.| is the bar): train-mode forward error 2.2e-07 at max|out| 1.17 (1.9e-07 of
it); gradient error per tensor between 1.1e-07 and 3.3e-07 x max|grad|."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simple_gcn_ref as REF  # noqa: E402

from wild_visual_navigation_amd import _lib  # noqa: E402
from wild_visual_navigation_amd.cfg import ExperimentParams  # noqa: E402
from wild_visual_navigation_amd.model import SimpleGCN, get_model  # noqa: E402
from wild_visual_navigation_amd.utils import Data  # noqa: E402


def _graph(N, E, seed):
    g = torch.Generator().manual_seed(seed)
    return 2 * torch.randn(N, 90, generator=g), torch.randint(0, N, (2, E), generator=g)


def test_config_defaults_and_registry():
    cfg = ExperimentParams().model.simple_gcn_cfg
    assert (cfg.input_size, cfg.reconstruction, list(cfg.hidden_sizes)) == (384, True, [256, 128, 1])
    p = ExperimentParams()
    p.model.name = "SimpleGCN"
    p.model.simple_gcn_cfg.input_size = 90     # (callers write it, quick_start.py:131-134)
    m = get_model(p.model)
    assert isinstance(m, SimpleGCN) and m.input_size == 90 and m.output_features == 91
    m = get_model({"name": "SimpleGCN", "simple_gcn_cfg": {"input_size": 5, "reconstruction": True, "hidden_sizes": [7, 3, 1]}})
    assert isinstance(m, SimpleGCN) and (m.desc.D, m.desc.H1, m.desc.H2) == (5, 7, 3)


def test_importable_under_the_alias_package():
    import wild_visual_navigation_amd.dropin as dropin

    dropin.install(force_synthetic=True)
    from wild_visual_navigation.model import SimpleGCN as Aliased, get_model as aliased_get_model

    assert Aliased is SimpleGCN and aliased_get_model is get_model


def test_state_dict_keys_shapes_and_strict_round_trip():
    m = SimpleGCN(90, True, [256, 128, 1])
    sd = m.state_dict()
    assert list(sd) == REF.KEYS
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes == {"layers.0.bias": (256,), "layers.0.lin.weight": (256, 90), "layers.1.bias": (128,),
                      "layers.1.lin.weight": (128, 256), "layers.2.bias": (91,), "layers.2.lin.weight": (91, 128)}
    for l, (i, o) in enumerate(((90, 256), (256, 128), (128, 91))):   # glorot uniform, zero bias
        a = (6.0 / (i + o)) ** 0.5
        w = sd[f"layers.{l}.lin.weight"]
        assert w.abs().max().item() <= a and w.abs().max().item() > 0.9 * a and not sd[f"layers.{l}.bias"].any()
    other = SimpleGCN(90, True, [256, 128, 1])
    want = REF.glorot_state_dict(90, [256, 128, 1], seed=3)
    other.load_state_dict(want, strict=True)
    for k in REF.KEYS:
        assert torch.equal(other.state_dict()[k], want[k])
    # the flat buffer [W1|b1|W2|b2|W3|b3] is SimpleMLP's for the same geometry, and the parameters alias it
    flat = other.flat_params()
    assert flat.numel() == _lib.lib().wvn_mlp_param_count(C.byref(_lib.MlpDesc(90, 256, 128, 0)))
    assert torch.equal(flat[: 256 * 90].view(256, 90), want["layers.0.lin.weight"])
    assert torch.equal(flat[-91:], want["layers.2.bias"])
    assert other.layers[0].lin.weight.data_ptr() == flat.data_ptr()


def test_train_mode_forward_and_gradients_match_float64_statement():
    x, ei = _graph(40, 200, seed=1)
    sd = REF.glorot_state_dict(90, [64, 32, 1], seed=2)
    m = SimpleGCN(90, True, [64, 32, 1])
    m.load_state_dict(sd)
    m.train()
    out = m(Data(x=x, edge_index=ei))
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    ref = REF.forward(sd64, x, ei)
    err = (out.detach().double() - ref.detach()).abs().max().item()
    print(f"train-mode forward: err {err:.3e}, max|out| {ref.abs().max().item():.3f}")
    assert out.shape == (40, 91) and err <= 2.0 ** -16 * ref.abs().max().item()
    w = torch.randn(40, 91, generator=torch.Generator().manual_seed(5))
    (out * w).sum().backward()
    (ref * w.double()).sum().backward()
    got = dict(m.named_parameters())
    for k in REF.KEYS:
        g64 = sd64[k].grad
        e = (got[k].grad.double() - g64).abs().max().item()
        print(f"grad {k}: err {e:.3e}, max|grad| {g64.abs().max().item():.3f}")
        assert e <= 2.0 ** -16 * g64.abs().max().item(), k


def test_eval_mode_on_cpu_tensors_is_refused():
    x, ei = _graph(10, 20, seed=3)
    m = SimpleGCN(90, True, [64, 32, 1])
    m.eval()
    with pytest.raises(_lib.WvnError):
        m(Data(x=x, edge_index=ei))
    m.train()
    with torch.no_grad(), pytest.raises(_lib.WvnError):     # training mode without autograd is the HIP path too
        m(Data(x=x, edge_index=ei))
    with pytest.raises(_lib.WvnError):
        m.forward_per_segment(x, torch.zeros(4, 4, dtype=torch.int32), edges=ei)


@pytest.mark.parametrize("args", [(90, False, [256, 128, 1]), (90, True, [256, 128, 2]), (90, True, [256, 1]), (90, True, [256, 128, 64, 1]),
                                  (1025, True, [256, 128, 1]), (0, True, [256, 128, 1]), (90, True, [257, 128, 1]), (90, True, [256, 0, 1])])
def test_constructor_refusals(args):
    with pytest.raises(ValueError):
        SimpleGCN(*args)


def test_workspace_query_and_argument_checks_without_gpu():
    h = _lib.lib()
    ok = _lib.MlpDesc(384, 256, 128, 0)
    assert h.wvn_gcn_workspace_bytes(C.byref(ok), 100, 700) > 100 * (256 + 128) * 4
    for d in (_lib.MlpDesc(1025, 256, 128, 0), _lib.MlpDesc(0, 256, 128, 0), _lib.MlpDesc(384, 257, 128, 0), _lib.MlpDesc(384, 256, 0, 0),
              _lib.MlpDesc(384, 256, 128, _lib.MLP_KIND_DOUBLE)):
        assert h.wvn_gcn_workspace_bytes(C.byref(d), 100, 700) == 0
    assert h.wvn_gcn_workspace_bytes(C.byref(ok), 0, 700) == 0 and h.wvn_gcn_workspace_bytes(C.byref(ok), 100, 99) == 0
    assert h.wvn_gcn_workspace_bytes(None, 100, 700) == 0
    words = (C.c_longlong * 64)()
    p = (C.addressof(words) + 15) // 16 * 16     # (16-byte aligned; never dereferenced: every call below is refused first)
    assert h.wvn_gcn_graph_from_edges(p, 8, 1, 8, 10, 17, p, p, 1 << 20, None) == 1001        # capacity < E + nodes
    assert h.wvn_gcn_graph_from_edges(p, 8, 1, 8, 10, 18, None, p, 1 << 20, None) == 1001      # no counter
    assert h.wvn_gcn_graph_from_edges(p, 8, 1, 8, 10, 18, p, p, 16, None) == 1002              # short workspace
    assert h.wvn_gcn_graph_from_bitmaps(p, 16, 4, 1, 1, 4, 15, p, p, 1 << 20, None) == 1001    # capacity < B * S * S
    assert h.wvn_gcn_forward(C.byref(_lib.MlpDesc(1025, 256, 128, 0)), p, p, 1025, 4, 8, p, p, 1 << 20, None) == 1001
    assert h.wvn_gcn_forward(C.byref(ok), p, p, 383, 4, 8, p, p, 1 << 30, None) == 1001        # ldx < D
    assert h.wvn_gcn_forward(C.byref(ok), p, p, 384, 4, 8, p, p, 16, None) == 1002
    assert h.wvn_gcn_segment_predict(C.byref(ok), p, p, 384, 1, 4, 16, p, 2, 8, 8, 0.0, 1.0, 0.5, None, p, p, p, p, 1 << 20, None) == 1001
    assert h.wvn_seg_adjacency_batched(None, p, 1, 8, 8, 4, None) == 1001
    assert all(w == 0 for w in words)
