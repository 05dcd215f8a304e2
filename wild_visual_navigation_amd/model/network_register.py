"""get_model -- wild_visual_navigation/model/network_register.py:44-55 (class-name registry; SimpleMLP, DoubleMLP, LinearRnvp and
SimpleGCN are on the MI355X path)."""
import inspect

from .double_mlp import DoubleMLP
from .linear_rnvp import LinearRnvp
from .simple_gcn import SimpleGCN
from .simple_mlp import SimpleMLP

_REGISTER = {"SimpleMLP": (SimpleMLP, "simple_mlp_cfg"), "DoubleMLP": (DoubleMLP, "double_mlp_cfg"),
             "LinearRnvp": (LinearRnvp, "linear_rnvp_cfg"), "SimpleGCN": (SimpleGCN, "simple_gcn_cfg")}


def _get(cfg, key):
    return cfg[key] if not hasattr(cfg, key) or isinstance(cfg, dict) else getattr(cfg, key)


def get_model(model_cfg):
    name = _get(model_cfg, "name")
    if name not in _REGISTER:
        raise KeyError(f"model '{name}' is not part of the MI355X hot path (available: {list(_REGISTER)})")
    cls, key = _REGISTER[name]
    sub = _get(model_cfg, key)
    # the constructor arguments the cfg node carries (DoubleMLP has no ``reconstruction``; LinearRnvp's cfg leaves flow_n,
    # batch_norm and **kwargs to the constructor's defaults, as upstream's LinearRnvp(**cfg) does)
    args = [a for a in inspect.signature(cls.__init__).parameters if a not in ("self", "kwargs")]
    kw = dict(sub) if isinstance(sub, dict) else {k: getattr(sub, k) for k in args if hasattr(sub, k)}
    for k in ("hidden_sizes", "coupling_topology"):
        if kw.get(k) is not None:
            kw[k] = list(kw[k])
    return cls(**kw)
