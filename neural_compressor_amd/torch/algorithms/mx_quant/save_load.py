"""save / load of an MX model (`model.save(output_dir)`, `load(output_dir, original_model)`), the files of smooth_quant/save_load.py:
  quantized_weight.pt   state_dict: uint8 `qweight`, uint8 `w_scale`, bias of every MXLinear; the float parameters of everything else
  qconfig.json          {"mx_quant": {blocksize, round_method}, "mx_modules": {name: [w_dtype, act_dtype]} (act_dtype "bf16": an
                         MXWeightOnlyLinear),
                         "mx_experts": {name: [w_dtype, act_dtype, E, H, I]},
                         "mx_gpt_oss_experts": {name: [w_dtype, act_dtype, E, H, I, alpha, limit]}}
An experts entry whose act_dtype is "bf16" is the weight-only class of its kind (MXWeightOnlyExperts / MXWeightOnlyGptOssExperts: the
same buffers).  MXExperts modules save their four uint8 buffers under their own names, MXGptOssExperts modules those and their two
fp32 biases.  The
"mx_experts" / "mx_gpt_oss_experts" keys are written only when the model has such modules; a directory without them (a model without
them, or one written before the modules existed) loads as before.  The file handling and the per-Linear rebuild are
utils/utility.py's (save_quantized, open_saved, take_linear, finish_load), shared with the other two.
"""

from functools import partial

from ...utils.utility import QCONFIG_NAME, WEIGHT_NAME  # noqa: F401  (this module's names for the two files)
from ...utils.utility import (_take_experts, finish_load, half_or_fp16, is_fused_experts, is_gpt_oss_experts, open_saved,
                              save_quantized, take_linear)
from .experts import MXExperts, MXGptOssExperts, MXWeightOnlyExperts, MXWeightOnlyGptOssExperts
from .mx_quant import MXLinear, MXWeightOnlyLinear


def qconfig_of(model):
    """The content of qconfig.json."""
    mods = {n: [m.w_dtype, m.act_dtype] for n, m in model.named_modules() if isinstance(m, MXLinear)}
    experts = {n: [m.w_dtype, m.act_dtype, m.num_experts, m.hidden_dim, m.intermediate_dim] for n, m in model.named_modules()
               if isinstance(m, MXExperts) and not isinstance(m, MXGptOssExperts)}
    oss = {n: [m.w_dtype, m.act_dtype, m.num_experts, m.hidden_dim, m.intermediate_dim, m.alpha, m.limit]
           for n, m in model.named_modules() if isinstance(m, MXGptOssExperts)}
    cfg = {"mx_quant": dict(getattr(model, "mx_info", {})), "mx_modules": mods}
    if experts:  # a model without MXExperts writes the file it always wrote
        cfg["mx_experts"] = experts
    if oss:
        cfg["mx_gpt_oss_experts"] = oss
    return cfg


def save(model, output_dir="./saved_results"):
    save_quantized(model, output_dir, qconfig_of(model))


def load(output_dir, original_model, device="cuda"):
    """Rebuild the MX model from the float architecture `original_model` (weights may be on any device, "meta" included)."""
    cfg, state, dev = open_saved(output_dir, device)
    for name, (w_dtype, act_dtype) in cfg["mx_modules"].items():
        cls = MXWeightOnlyLinear if act_dtype == "bf16" else MXLinear  # the weight-only cell: same buffers, bf16 activations
        take_linear(state, original_model, name, dev, partial(cls, w_dtype=w_dtype, act_dtype=act_dtype))
    for name, (w_dtype, act_dtype, E, H, I) in cfg.get("mx_experts", {}).items():
        _take_experts(state, original_model, name, dev, is_fused_experts,
                      lambda old: (MXWeightOnlyExperts if act_dtype == "bf16" else MXExperts)(
                          E, H, I, w_dtype=w_dtype, act_dtype=act_dtype, act_fn=old.act_fn, device=dev,
                          float_type=half_or_fp16(old.gate_up_proj.dtype)))
    for name, (w_dtype, act_dtype, E, H, I, alpha, limit) in cfg.get("mx_gpt_oss_experts", {}).items():
        _take_experts(state, original_model, name, dev, is_gpt_oss_experts,
                      lambda old: (MXWeightOnlyGptOssExperts if act_dtype == "bf16" else MXGptOssExperts)(
                          E, H, I, w_dtype=w_dtype, act_dtype=act_dtype, alpha=alpha, limit=limit, device=dev,
                          float_type=half_or_fp16(old.gate_up_proj.dtype)))
    finish_load(original_model, state, dev)
    original_model.mx_info = cfg.get("mx_quant", {})
    return original_model
