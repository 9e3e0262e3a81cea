from .experts import MXExperts, MXGptOssExperts
from .mx_quant import MXLinear, MXQuantizer, mx_linear_group
from .save_load import load, save

__all__ = ["MXLinear", "MXExperts", "MXGptOssExperts", "MXQuantizer", "mx_linear_group", "save", "load"]
