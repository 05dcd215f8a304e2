from .simple_mlp import SimpleMLP
from .double_mlp import DoubleMLP
from .linear_rnvp import LinearRnvp
from .simple_gcn import SimpleGCN
from .network_register import get_model

__all__ = ["SimpleMLP", "DoubleMLP", "LinearRnvp", "SimpleGCN", "get_model"]
