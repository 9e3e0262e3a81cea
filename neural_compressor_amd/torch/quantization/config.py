"""RTNConfig / GPTQConfig / AWQConfig with the reference's field names and defaults.

Reference: neural_compressor/torch/quantization/config.py -- RTNConfig :119-300, GPTQConfig :322-510,
AWQConfig :525-690.  Only the weight-only-quant configs exist here (SURVEY.md section 8 scope).
Field names, order and default values are kept verbatim so `GPTQConfig(bits=4, group_size=128, ...)` written
for the reference constructs the same object here; lm_head is excluded unless `quant_lm_head` (reference
config.py:242-245 via LM_HEAD_NAMES).
"""

from typing import List, Optional

import torch

from ...common.base_config import BaseConfig, register_config
from ...common.utils import AWQ, DEFAULT_WHITE_LIST, FP8_QUANT, GPTQ, MX_QUANT, RTN, SMOOTH_QUANT
from ..utils.utility import (
    LM_HEAD_NAMES, PRIORITY_AWQ, PRIORITY_FP8_QUANT, PRIORITY_GPTQ, PRIORITY_MX_QUANT, PRIORITY_RTN, PRIORITY_SMOOTH_QUANT, WOQ_WHITE_LIST, is_fused_experts, is_gpt_oss_experts,
)

FRAMEWORK_NAME = "torch"

__all__ = [
    "RTNConfig", "GPTQConfig", "AWQConfig", "get_default_rtn_config", "get_default_gptq_config",
    "get_default_awq_config", "SmoothQuantConfig", "get_default_sq_config", "MXQuantConfig", "get_default_mx_config", "FP8Config", "get_default_fp8_config", "FRAMEWORK_NAME",
]


class TorchBaseConfig(BaseConfig):
    """Weight-only configs see every nn.Linear / transformers.Conv1D of the model."""

    def __init__(self, white_list=DEFAULT_WHITE_LIST):
        super().__init__(white_list=white_list)
        object.__setattr__(self, "params_list", self.__class__._generate_params_list())

    @staticmethod
    def get_model_info(model: torch.nn.Module):
        return [(name, type(m).__name__) for name, m in model.named_modules() if isinstance(m, WOQ_WHITE_LIST)]

    @classmethod
    def register_supported_configs(cls):
        cls.supported_configs = []

    def _fp32_for_lm_head(self, **extra):
        """Local override that leaves lm_head in floating point (dtype="fp32" => skipped by every algorithm)."""
        return self.__class__(dtype="fp32", **extra)


def _assign(self, local_vars, names):
    for n in names:
        setattr(self, n, local_vars[n])


@register_config(framework_name=FRAMEWORK_NAME, algo_name=RTN, priority=PRIORITY_RTN)
class RTNConfig(TorchBaseConfig):
    """Round-to-nearest weight-only quantization (reference config.py:119)."""

    name = RTN
    supported_configs: List = []

    def __init__(
        self,
        dtype: str = "int",
        bits: int = 4,
        use_sym: bool = True,
        group_size: int = 32,
        group_dim: int = 1,
        use_full_range: bool = False,
        use_mse_search: bool = False,
        use_layer_wise: bool = True,
        model_path: str = "",
        use_double_quant: bool = False,
        double_quant_dtype: str = "int",
        double_quant_bits: int = 8,
        double_quant_use_sym: bool = False,
        double_quant_group_size: int = 256,
        quant_lm_head: bool = False,
        white_list: Optional[List] = DEFAULT_WHITE_LIST,
        **kwargs,
    ):
        super().__init__(white_list=white_list)
        _assign(self, locals(), [
            "dtype", "bits", "use_sym", "group_size", "group_dim", "use_full_range", "use_mse_search",
            "use_layer_wise", "model_path", "use_double_quant", "double_quant_bits", "double_quant_dtype",
            "double_quant_use_sym", "double_quant_group_size", "quant_lm_head",
        ])
        self._post_init()

    def to_config_mapping(self, config_list=None, model_info=None):
        if not self.quant_lm_head:
            self.set_local(LM_HEAD_NAMES, self._fp32_for_lm_head(use_layer_wise=self.use_layer_wise, model_path=self.model_path))
        return super().to_config_mapping(config_list, model_info)

    @staticmethod
    def get_model_info(model: torch.nn.Module):
        """Every Linear / Conv1D, and the fused MoE experts modules (is_fused_experts), which only RTN packs."""
        return [(name, type(m).__name__) for name, m in model.named_modules() if isinstance(m, WOQ_WHITE_LIST) or is_fused_experts(m)]

    @classmethod
    def get_config_set_for_tuning(cls):
        return RTNConfig(dtype=["int4", "nf4"], use_sym=[True, False], group_size=[32, 128], use_mse_search=[False, True])


def get_default_rtn_config(processor_type=None) -> RTNConfig:
    # the reference picks use_layer_wise by CPU brand (config.py:278-288); HBM is 288 GB here: never layer-wise
    return RTNConfig(use_layer_wise=False)


@register_config(framework_name=FRAMEWORK_NAME, algo_name=GPTQ, priority=PRIORITY_GPTQ)
class GPTQConfig(TorchBaseConfig):
    """GPTQ (reference config.py:322)."""

    name = GPTQ
    supported_configs: List = []

    def __init__(
        self,
        dtype: str = "int",
        bits: int = 4,
        use_sym: bool = True,
        group_size: int = 32,
        use_mse_search: bool = False,
        use_layer_wise: bool = False,
        use_block_wise: bool = False,
        model_path: str = "",
        use_double_quant: bool = False,
        double_quant_dtype: str = "int",
        double_quant_bits: int = 8,
        double_quant_use_sym: bool = False,
        double_quant_group_size: int = 256,
        quant_lm_head: bool = False,
        act_order: bool = False,
        hybrid_order: bool = False,
        fp8_aware: bool = False,
        percdamp: float = 0.01,
        block_size: int = 2048,
        static_groups: bool = False,
        true_sequential: bool = False,
        quant_experts: bool = False,
        white_list: Optional[List] = DEFAULT_WHITE_LIST,
        **kwargs,
    ):
        super().__init__(white_list=white_list)
        _assign(self, locals(), [
            "dtype", "bits", "use_sym", "group_size", "use_mse_search", "use_layer_wise", "use_block_wise",
            "model_path", "use_double_quant", "double_quant_bits", "double_quant_dtype", "double_quant_use_sym",
            "double_quant_group_size", "act_order", "hybrid_order", "fp8_aware", "percdamp", "block_size",
            "static_groups", "true_sequential", "quant_lm_head", "quant_experts",
        ])
        self._post_init()

    def extend_model_info(self, model, model_info):
        """`quant_experts=True` (an extension of the reference's fields; off by default): the fused MoE experts modules
        (is_fused_experts) join the Linears, so they get (name, type) keys in the config mapping and GPTQ packs them
        (algorithms/weight_only/experts_gptq.py).  `get_model_info` itself keeps returning the Linears only."""
        if not self.quant_experts:
            return model_info
        have = set(model_info)
        extra = [(name, type(m).__name__) for name, m in model.named_modules() if is_fused_experts(m)]
        return list(model_info) + [e for e in extra if e not in have]

    def to_config_mapping(self, config_list=None, model_info=None):
        if not self.quant_lm_head:
            self.set_local(
                LM_HEAD_NAMES,
                self._fp32_for_lm_head(use_layer_wise=self.use_layer_wise, model_path=self.model_path, use_block_wise=self.use_block_wise),
            )
        return super().to_config_mapping(config_list, model_info)

    @classmethod
    def get_config_set_for_tuning(cls):
        return GPTQConfig(act_order=[True, False], use_sym=[False, True])


def get_default_gptq_config(processor_type=None) -> GPTQConfig:
    return GPTQConfig()


@register_config(framework_name=FRAMEWORK_NAME, algo_name=AWQ, priority=PRIORITY_AWQ)
class AWQConfig(TorchBaseConfig):
    """AWQ (reference config.py:525)."""

    name = AWQ
    supported_configs: List = []

    def __init__(
        self,
        dtype: str = "int",
        bits: int = 4,
        use_sym: bool = True,
        group_size: int = 32,
        group_dim: int = 1,
        use_full_range: bool = False,
        use_mse_search: bool = False,
        use_layer_wise: bool = False,
        model_path: str = "",
        use_double_quant: bool = False,
        double_quant_dtype: str = "int",
        double_quant_bits: int = 8,
        double_quant_use_sym: bool = True,
        double_quant_group_size: int = 256,
        quant_lm_head: bool = False,
        use_auto_scale: bool = True,
        use_auto_clip: bool = True,
        folding: bool = False,
        white_list: Optional[List] = DEFAULT_WHITE_LIST,
        absorb_layer_dict: dict = {},
        **kwargs,
    ):
        super().__init__(white_list=white_list)
        _assign(self, locals(), [
            "dtype", "bits", "use_sym", "group_size", "group_dim", "use_full_range", "use_mse_search",
            "use_layer_wise", "model_path", "use_double_quant", "double_quant_bits", "double_quant_dtype",
            "double_quant_use_sym", "double_quant_group_size", "quant_lm_head", "use_auto_scale", "use_auto_clip",
            "folding", "absorb_layer_dict",
        ])
        self._post_init()

    def to_config_mapping(self, config_list=None, model_info=None):
        if not self.quant_lm_head:
            self.set_local(LM_HEAD_NAMES, self._fp32_for_lm_head(use_layer_wise=self.use_layer_wise, model_path=self.model_path))
        return super().to_config_mapping(config_list, model_info)

    @classmethod
    def get_config_set_for_tuning(cls):
        return AWQConfig(bits=[4, 6])


def get_default_awq_config() -> AWQConfig:
    return AWQConfig()


@register_config(framework_name=FRAMEWORK_NAME, algo_name=SMOOTH_QUANT, priority=PRIORITY_SMOOTH_QUANT)
class SmoothQuantConfig(TorchBaseConfig):
    """SmoothQuant W8A8 (reference config.py:1485-1612): same fields and defaults.  On MI355X the weights are int8 per-channel
    symmetric and the activations one of two cells: the default, uint8 per-tensor asymmetric min/max (static: the range is frozen at
    calibration), or `act_dtype="int8", act_sym=True, act_granularity="per_token"` (dynamic: every token gets its own symmetric scale
    at run time).  A model may mix them per layer through `set_local`.  `alpha` is a number or "auto" (reference
    smooth_quant/utility.py:1232 AutoAlpha: the layer-wise tuner, or the block-wise one with `do_blockwise=True`)."""

    name = SMOOTH_QUANT
    supported_configs: List = []

    def __init__(
        self,
        w_dtype: str = "int8",
        w_sym: bool = True,
        w_granularity: str = "per_channel",
        w_algo: str = "minmax",
        act_dtype: str = "uint8",
        act_sym: bool = False,
        act_granularity: str = "per_tensor",
        act_algo: str = "minmax",
        excluded_precisions: list = [],
        alpha: float = 0.5,
        folding: bool = False,
        scale_sharing: bool = False,
        init_alpha: float = 0.5,
        alpha_min: float = 0.0,
        alpha_max: float = 1.0,
        alpha_step: float = 0.1,
        shared_criterion: str = "max",
        do_blockwise: bool = False,
        auto_alpha_args: dict = None,
        white_list: Optional[List] = DEFAULT_WHITE_LIST,
        **kwargs,
    ):
        super().__init__(white_list=white_list)
        _assign(self, locals(), [
            "w_dtype", "w_sym", "w_granularity", "w_algo", "act_dtype", "act_sym", "act_granularity", "act_algo",
            "excluded_precisions", "alpha", "folding", "scale_sharing", "init_alpha", "alpha_min", "alpha_max",
            "alpha_step", "shared_criterion", "do_blockwise",
        ])
        self.auto_alpha_args = {
            "init_alpha": init_alpha, "alpha_min": alpha_min, "alpha_max": alpha_max, "alpha_step": alpha_step,
            "shared_criterion": shared_criterion, "do_blockwise": do_blockwise,
        }
        self.absorb_to_layer = kwargs.get("absorb_to_layer", None)
        if w_dtype != "fp32":
            unsupported = []
            if w_dtype != "int8" or not w_sym or w_granularity != "per_channel" or w_algo != "minmax":
                unsupported.append("weights must be int8 / symmetric / per_channel / minmax")
            static_cell = act_dtype == "uint8" and not act_sym and act_granularity == "per_tensor"
            token_cell = act_dtype == "int8" and act_sym is True and act_granularity == "per_token"
            if not (static_cell or token_cell) or act_algo != "minmax":
                unsupported.append("activations must be uint8 / asymmetric / per_tensor / minmax")
            if unsupported:
                raise NotImplementedError("SmoothQuant on MI355X: " + "; ".join(unsupported))
        self._post_init()

    @staticmethod
    def get_model_info(model: torch.nn.Module, example_inputs=None):
        return [(name, type(m).__name__) for name, m in model.named_modules() if isinstance(m, torch.nn.Linear)]

    @classmethod
    def register_supported_configs(cls):
        cls.supported_configs = []


def get_default_sq_config() -> SmoothQuantConfig:
    return SmoothQuantConfig()


@register_config(framework_name=FRAMEWORK_NAME, algo_name=MX_QUANT, priority=PRIORITY_MX_QUANT)
class MXQuantConfig(TorchBaseConfig):
    """OCP microscaling linears (reference config.py MXQuantConfig: same fields).  The reference emulates the formats in float and
    defaults to MX-INT8 (`w_dtype="int8", act_dtype="int8"`); the block-scaled matrix instruction of the MI355X has no INT8 operand,
    so the defaults here are `w_dtype="fp8_e4m3", act_dtype="fp8_e4m3"` -- a deliberate deviation.  Supported (w_dtype, act_dtype):
    ("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4"), "fp4" being e2m1; `blocksize=32`, `round_method="nearest"`,
    `weight_only=False`; `out_dtype` is accepted and unused (the output has the activation's type).  `w_dtype="fp32"` (through
    `set_local`) leaves a layer float; lm_head stays float unless `quant_lm_head=True`.  `quant_experts=True` (an extension of the
    reference's fields; off by default) also converts the fused MoE experts modules (is_fused_experts) to MXExperts."""

    name = MX_QUANT
    supported_configs: List = []
    PAIRS = (("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4"))

    def __init__(
        self,
        w_dtype: str = "fp8_e4m3",
        act_dtype: str = "fp8_e4m3",
        out_dtype: str = "bfloat16",
        blocksize: int = 32,
        round_method: str = "nearest",
        weight_only: bool = False,
        quant_lm_head: bool = False,
        quant_experts: bool = False,
        white_list: Optional[List] = DEFAULT_WHITE_LIST,
        **kwargs,
    ):
        super().__init__(white_list=white_list)
        _assign(self, locals(), ["w_dtype", "act_dtype", "out_dtype", "blocksize", "round_method", "weight_only", "quant_lm_head",
                                 "quant_experts"])
        if w_dtype != "fp32":
            unsupported = []
            if (w_dtype, act_dtype) not in self.PAIRS:
                unsupported.append(f"(w_dtype, act_dtype) must be one of {self.PAIRS}, got {(w_dtype, act_dtype)}")
            if blocksize != 32:
                unsupported.append("blocksize must be 32 (the block of the matrix instruction)")
            if round_method != "nearest":
                unsupported.append('round_method must be "nearest"')
            if weight_only:
                unsupported.append("weight_only=True is not built (the instruction takes MX operands on both sides)")
            if unsupported:
                raise NotImplementedError("MXQuant on MI355X: " + "; ".join(unsupported))
        self._post_init()

    def extend_model_info(self, model, model_info):
        """`quant_experts=True`: the fused MoE experts modules join the Linears (as GPTQConfig.extend_model_info), so they get
        (name, type) keys in the config mapping and MXQuantizer converts them (algorithms/mx_quant/experts.py).  `get_model_info`
        itself keeps returning the Linears only."""
        if not self.quant_experts:
            return model_info
        have = set(model_info)
        # GPT-OSS experts (is_gpt_oss_experts: transposed, interleaved, biased, clamped SwiGLU) become MXGptOssExperts
        extra = [(name, type(m).__name__) for name, m in model.named_modules() if is_fused_experts(m) or is_gpt_oss_experts(m)]
        return list(model_info) + [e for e in extra if e not in have]

    def to_config_mapping(self, config_list=None, model_info=None):
        if not self.quant_lm_head:
            self.set_local(LM_HEAD_NAMES, self.__class__(w_dtype="fp32"))
        return super().to_config_mapping(config_list, model_info)

    @staticmethod
    def get_model_info(model: torch.nn.Module, example_inputs=None):
        return [(name, type(m).__name__) for name, m in model.named_modules() if isinstance(m, torch.nn.Linear)]

    @classmethod
    def register_supported_configs(cls):
        cls.supported_configs = []


def get_default_mx_config() -> MXQuantConfig:
    return MXQuantConfig()


@register_config(framework_name=FRAMEWORK_NAME, algo_name=FP8_QUANT, priority=PRIORITY_FP8_QUANT)
class FP8Config(TorchBaseConfig):
    """FP8 linears: OCP e4m3 weights with one fp32 scale per output channel and e4m3 activations with one fp32 scale per token,
    computed at run time ("FP8 dynamic"), on the f8f6f4 matrix instruction of the MI355X.

    The class name is the reference's; the fields are this cell's.  The reference's FP8Config drives a Gaudi workflow (measure / quantize
    modes, scale methods, measurement dump files) that is not reproduced here: this algorithm is data-free and has exactly one cell, so
    the fields name that cell and every other value raises NotImplementedError -- a deliberate deviation, of the same kind as
    MXQuantConfig's defaults.
      fp8_config="E4M3"             the element format ("E5M2" is not built); "fp32" (through `set_local`) leaves a layer float
      act_granularity="per_token"   one activation scale per row of the flattened input, from that row's max |x|
      w_granularity="per_channel"   one weight scale per output channel
      dynamic_quantization=True     activation scales come from the data of the call; static (calibrated) scales are not built
      quant_lm_head=False           lm_head stays float unless set
      moe_experts=False             True also converts the fused MoE experts modules (is_fused_experts: Mixtral / Qwen2-MoE / Qwen3-MoE /
                                    OLMoE `*Experts` with SiLU, up to 512 experts) to FP8Experts; `set_local(name,
                                    FP8Config(fp8_config="fp32"))` keeps one of them float.  GPTQConfig and MXQuantConfig call their
                                    switch `quant_experts`; this one is `moe_experts` -- a deliberate deviation in the name: an
                                    FP8Config has no `quant_experts` attribute (tests/test_fp8_cpu.py pins that).
    Without the flag fused MoE experts modules stay float."""

    name = FP8_QUANT
    supported_configs: List = []

    def __init__(
        self,
        fp8_config: str = "E4M3",
        act_granularity: str = "per_token",
        w_granularity: str = "per_channel",
        dynamic_quantization: bool = True,
        quant_lm_head: bool = False,
        moe_experts: bool = False,
        white_list: Optional[List] = DEFAULT_WHITE_LIST,
        **kwargs,
    ):
        super().__init__(white_list=white_list)
        _assign(self, locals(), ["fp8_config", "act_granularity", "w_granularity", "dynamic_quantization", "quant_lm_head",
                                 "moe_experts"])
        if fp8_config != "fp32":
            unsupported = []
            if fp8_config != "E4M3":
                unsupported.append(f'fp8_config must be "E4M3" (OCP e4m3fn), got {fp8_config!r}')
            if act_granularity != "per_token":
                unsupported.append(f'act_granularity must be "per_token", got {act_granularity!r}')
            if w_granularity != "per_channel":
                unsupported.append(f'w_granularity must be "per_channel", got {w_granularity!r}')
            if dynamic_quantization is not True:
                unsupported.append("dynamic_quantization must be True (static activation scales are not built)")
            if unsupported:
                raise NotImplementedError("FP8 on MI355X: " + "; ".join(unsupported))
        self._post_init()

    def extend_model_info(self, model, model_info):
        """`moe_experts=True`: the fused MoE experts modules join the Linears (as MXQuantConfig.extend_model_info), so they get
        (name, type) keys in the config mapping and FP8Quantizer converts them (algorithms/fp8_quant/experts.py).  `get_model_info`
        itself keeps returning the Linears only."""
        if not self.moe_experts:
            return model_info
        have = set(model_info)
        extra = [(name, type(m).__name__) for name, m in model.named_modules() if is_fused_experts(m)]
        return list(model_info) + [e for e in extra if e not in have]

    def to_config_mapping(self, config_list=None, model_info=None):
        if not self.quant_lm_head:
            self.set_local(LM_HEAD_NAMES, self.__class__(fp8_config="fp32"))
        return super().to_config_mapping(config_list, model_info)

    @staticmethod
    def get_model_info(model: torch.nn.Module, example_inputs=None):
        return [(name, type(m).__name__) for name, m in model.named_modules() if isinstance(m, torch.nn.Linear)]

    @classmethod
    def register_supported_configs(cls):
        cls.supported_configs = []


def get_default_fp8_config() -> FP8Config:
    return FP8Config()
