from .simple_mlp import SimpleMLP
from .double_mlp import DoubleMLP
from .linear_rnvp import LinearRnvp
from .network_register import get_model

__all__ = ["SimpleMLP", "DoubleMLP", "LinearRnvp", "get_model"]
