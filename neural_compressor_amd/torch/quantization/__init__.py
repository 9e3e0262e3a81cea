from . import algorithm_entry  # registers "rtn" / "gptq" / "awq"  # noqa: F401
from .config import (
    AWQConfig, FP8Config, GPTQConfig, MXQuantConfig, RTNConfig, SmoothQuantConfig, get_default_awq_config, get_default_gptq_config,
    get_default_fp8_config, get_default_mx_config, get_default_rtn_config, get_default_sq_config,
)
from .quantize import convert, prepare, quantize
from ..algorithms.weight_only.save_load import load, save  # reference torch/quantization/save_load_entry.py

__all__ = [
    "prepare", "convert", "quantize", "save", "load", "RTNConfig", "GPTQConfig", "AWQConfig", "SmoothQuantConfig",
    "get_default_sq_config", "MXQuantConfig", "get_default_mx_config", "FP8Config", "get_default_fp8_config",
    "get_default_rtn_config", "get_default_gptq_config", "get_default_awq_config",
]
