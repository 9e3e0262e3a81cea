from .experts import FP8Experts  # noqa: F401  (importable from here; __all__ keeps the four names tests/test_fp8_cpu.py pins)
from .fp8_quant import FP8Linear, FP8Quantizer
from .fp8_quant import fp8_gated_pair, fp8_linear_group  # noqa: F401  (importable from here, like FP8Experts)
from .save_load import load, save

__all__ = ["FP8Linear", "FP8Quantizer", "save", "load"]
