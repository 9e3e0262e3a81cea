from .mx_quant import MXLinear, MXQuantizer
from .save_load import load, save

__all__ = ["MXLinear", "MXQuantizer", "save", "load"]
