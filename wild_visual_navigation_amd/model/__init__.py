from .simple_mlp import SimpleMLP
from .double_mlp import DoubleMLP
from .network_register import get_model

__all__ = ["SimpleMLP", "DoubleMLP", "get_model"]
