"""save / load of an FP8 model (`model.save(output_dir)`, `load(output_dir, original_model)`), the files of mx_quant/save_load.py:
  quantized_weight.pt   state_dict: uint8 `qweight`, fp32 `w_scale`, bias of every FP8Linear; the float parameters of everything else
  qconfig.json          {"fp8_quant": {fp8_config, act_granularity, w_granularity}, "fp8_modules": [name, ...],
                         "fp8_experts": {name: [E, H, I]}, "fp8_block_experts": {name: [E, H, I]}}
"fp8_modules" lists FP8Linear and FP8BlockLinear alike; load tells them apart by the rank of `w_scale` ([N] against
[ceil(N/128), Kp/128]), so one model may hold both.  FP8Experts modules save their four buffers under their own names.  The "fp8_experts" key is written only when the model has such
modules; a directory without it (a model without them, or one written before FP8Experts existed) loads as before.  The same holds for
FP8BlockExperts modules and the "fp8_block_experts" key.  The file handling and the per-Linear rebuild are utils/utility.py's
(save_quantized, open_saved, take_linear, finish_load), shared with the other two.
"""

from ...utils.utility import QCONFIG_NAME, WEIGHT_NAME  # noqa: F401  (this module's names for the two files)
from ...utils.utility import _take_experts, finish_load, half_or_fp16, is_fused_experts, open_saved, save_quantized, take_linear
from .block import FP8BlockLinear
from .block_experts import FP8BlockExperts
from .experts import FP8Experts
from .fp8_quant import FP8Linear


def qconfig_of(model):
    """The content of qconfig.json."""
    cfg = {"fp8_quant": dict(getattr(model, "fp8_info", {})),
           "fp8_modules": [n for n, m in model.named_modules() if isinstance(m, (FP8Linear, FP8BlockLinear))]}
    experts = {n: [m.num_experts, m.hidden_dim, m.intermediate_dim] for n, m in model.named_modules() if isinstance(m, FP8Experts)}
    if experts:  # a model without FP8Experts writes the file it always wrote
        cfg["fp8_experts"] = experts
    blocked = {n: [m.num_experts, m.hidden_dim, m.intermediate_dim] for n, m in model.named_modules() if isinstance(m, FP8BlockExperts)}
    if blocked:
        cfg["fp8_block_experts"] = blocked
    return cfg


def save(model, output_dir="./saved_results"):
    save_quantized(model, output_dir, qconfig_of(model))


def load(output_dir, original_model, device="cuda"):
    """Rebuild the FP8 model from the float architecture `original_model` (weights may be on any device, "meta" included)."""
    cfg, state, dev = open_saved(output_dir, device)
    for name in cfg["fp8_modules"]:
        cls = FP8BlockLinear if state[name + ".w_scale"].dim() == 2 else FP8Linear  # [ceil(N/128), Kp/128] against [N]
        take_linear(state, original_model, name, dev, cls)
    for key, cls in (("fp8_experts", FP8Experts), ("fp8_block_experts", FP8BlockExperts)):
        for name, (E, H, I) in cfg.get(key, {}).items():
            _take_experts(state, original_model, name, dev, is_fused_experts,
                          lambda old: cls(E, H, I, act_fn=old.act_fn, device=dev, float_type=half_or_fp16(old.gate_up_proj.dtype)))
    finish_load(original_model, state, dev)
    original_model.fp8_info = cfg.get("fp8_quant", {})
    return original_model
