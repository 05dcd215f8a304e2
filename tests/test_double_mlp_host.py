"""DoubleMLP without a GPU: the model registry, the state-dict layout against the reference's (tests/golden/double_mlp_train.pt),
the configuration tree and the C-ABI surface."""
import ctypes as C
import os
import re

import pytest
import torch

from wild_visual_navigation_amd import _lib
from wild_visual_navigation_amd.cfg import ExperimentParams
from wild_visual_navigation_amd.cfg.experiment_params import ModelParams
from wild_visual_navigation_amd.model import DoubleMLP, SimpleMLP, get_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_get_model_returns_a_double_mlp():
    m = get_model({"name": "DoubleMLP", "double_mlp_cfg": {"input_size": 90, "hidden_sizes": [64, 32, 1]}})
    assert isinstance(m, DoubleMLP) and m.input_size == 90 and m.output_features == 91 and m.nr_sigmoid_layers == 1
    p = ExperimentParams()
    p.model.name = "DoubleMLP"
    m = get_model(p.model)
    assert isinstance(m, DoubleMLP) and m.input_size == 384
    assert (m.desc.D, m.desc.H1, m.desc.H2, m.desc.reserved) == (384, 64, 32, _lib.MLP_KIND_DOUBLE)
    p.model.name = "SimpleMLP"
    assert isinstance(get_model(p.model), SimpleMLP)


@pytest.mark.parametrize("key,D", [("d90", 90), ("d384", 384)])
def test_state_dict_equals_the_reference_layout(golden, key, D):
    sd0 = golden("double_mlp_train.pt")[key]["sd0"]
    m = DoubleMLP(D, [64, 32, 1])
    sd = m.state_dict()
    assert list(sd) == list(sd0) == [f"networks.{n}.{i}.{p}" for n in (0, 1) for i in (0, 2, 4) for p in ("weight", "bias")]
    for k, v in sd.items():
        assert v.shape == sd0[k].shape and v.dtype == sd0[k].dtype, k
    m.load_state_dict(sd0, strict=True)
    flat = m.flat_params()
    assert flat.numel() == sum(v.numel() for v in sd0.values())
    assert torch.equal(flat, torch.cat([sd0[k].reshape(-1) for k in sd0]))   # the flat buffer is the keys' order


def test_params_in_order_follow_adam_order():
    m = DoubleMLP(90, [64, 32, 1])
    ps = m._params_in_order()
    assert len(ps) == 12
    assert all(a is b for a, b in zip(ps, m.parameters()))
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    assert all(a is b for a, b in zip(ps, opt.param_groups[0]["params"]))


@pytest.mark.parametrize("hidden", [[255], [64, 32], [64, 32, 2], [64, 32, 16, 1], [300, 32, 1]])
def test_unsupported_hidden_sizes_are_refused(hidden):
    with pytest.raises(ValueError):
        DoubleMLP(90, hidden)


def test_default_model_configuration_is_unchanged():
    mp = ModelParams()
    assert mp.name == "SimpleMLP"
    assert (mp.simple_mlp_cfg.input_size, list(mp.simple_mlp_cfg.hidden_sizes), mp.simple_mlp_cfg.reconstruction) == (90, [256, 32, 1], True)
    assert (mp.double_mlp_cfg.input_size, list(mp.double_mlp_cfg.hidden_sizes)) == (384, [64, 32, 1])
    assert not hasattr(mp.double_mlp_cfg, "reconstruction")


def test_c_abi_declares_and_binds_the_model_switch():
    with open(os.path.join(ROOT, "include", "wvn_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+WVN_MLP_KIND_DOUBLE\s+1\b", hdr)
    for name in ("wvn_double_mlp_row_tile", "wvn_double_mlp_fused_ok"):
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
    # the struct layout is what it was: four ints, the kind in the last one
    body = re.search(r"typedef struct wvn_mlp_desc \{(.*?)\} wvn_mlp_desc;", hdr, re.S).group(1)
    assert re.findall(r"\bint\s+(\w+)\s*;", body) == ["D", "H1", "H2", "reserved"]
    assert C.sizeof(_lib.MlpDesc) == 16 and [f[0] for f in _lib.MlpDesc._fields_] == ["D", "H1", "H2", "reserved"]
    assert SimpleMLP(90, [256, 32, 1], True).desc.reserved == 0


def test_library_exports_the_symbols():
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m wild_visual_navigation_amd.csrc.build)"
    h = C.CDLL(_lib.LIB_PATH)   # (dlopen only: no GPU call)
    for name in ("wvn_double_mlp_row_tile", "wvn_double_mlp_fused_ok"):
        assert hasattr(h, name)
    h.wvn_double_mlp_row_tile.restype = C.c_int
    T = h.wvn_double_mlp_row_tile()
    assert T > 0
    h.wvn_double_mlp_fused_ok.argtypes = [C.c_void_p, C.c_int]
    d = _lib.MlpDesc(384, 64, 32, _lib.MLP_KIND_DOUBLE)
    assert h.wvn_double_mlp_fused_ok(C.byref(d), 2048) == 1 and h.wvn_double_mlp_fused_ok(C.byref(d), 2049) == 0
    assert h.wvn_double_mlp_fused_ok(C.byref(_lib.MlpDesc(384, 48, 16, _lib.MLP_KIND_DOUBLE)), 100) == 0
    assert h.wvn_double_mlp_fused_ok(C.byref(_lib.MlpDesc(384, 64, 32, 0)), 100) == 0
