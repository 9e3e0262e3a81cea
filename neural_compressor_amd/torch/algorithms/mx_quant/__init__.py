from .experts import MXExperts
from .mx_quant import MXLinear, MXQuantizer, mx_linear_group
from .save_load import load, save

__all__ = ["MXLinear", "MXExperts", "MXQuantizer", "mx_linear_group", "save", "load"]
