from .fp8_quant import FP8Linear, FP8Quantizer
from .save_load import load, save

__all__ = ["FP8Linear", "FP8Quantizer", "save", "load"]
