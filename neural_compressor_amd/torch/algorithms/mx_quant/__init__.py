from .experts import MXExperts, MXGptOssExperts, MXWeightOnlyExperts, MXWeightOnlyGptOssExperts
from .mx_quant import MXLinear, MXQuantizer, MXWeightOnlyLinear, mx_linear_group
from .save_load import load, save

__all__ = ["MXLinear", "MXWeightOnlyLinear", "MXExperts", "MXGptOssExperts", "MXWeightOnlyExperts", "MXWeightOnlyGptOssExperts",
           "MXQuantizer", "mx_linear_group", "save", "load"]
