"""save / load of an MX model (`model.save(output_dir)`, `load(output_dir, original_model)`), the files of smooth_quant/save_load.py:
  quantized_weight.pt   state_dict: uint8 `qweight`, uint8 `w_scale`, bias of every MXLinear; the float parameters of everything else
  qconfig.json          {"mx_quant": {blocksize, round_method}, "mx_modules": {name: [w_dtype, act_dtype]},
                         "mx_experts": {name: [w_dtype, act_dtype, E, H, I]},
                         "mx_gpt_oss_experts": {name: [w_dtype, act_dtype, E, H, I, alpha, limit]}}
MXExperts modules save their four uint8 buffers under their own names, MXGptOssExperts modules those and their two fp32 biases.  The
"mx_experts" / "mx_gpt_oss_experts" keys are written only when the model has such modules; a directory without them (a model without
them, or one written before the modules existed) loads as before.
"""

import json
import os

import torch

from ...utils.utility import _take, _take_experts, get_module, half_or_fp16, is_fused_experts, is_gpt_oss_experts, set_module
from .experts import MXExperts, MXGptOssExperts
from .mx_quant import MXLinear

WEIGHT_NAME = "quantized_weight.pt"
QCONFIG_NAME = "qconfig.json"


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
    os.makedirs(output_dir, exist_ok=True)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    with open(os.path.join(output_dir, QCONFIG_NAME), "w") as f:
        json.dump(qconfig_of(model), f, indent=2)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(output_dir, WEIGHT_NAME))


def load(output_dir, original_model, device="cuda"):
    """Rebuild the MX model from the float architecture `original_model` (weights may be on any device, "meta" included)."""
    with open(os.path.join(output_dir, QCONFIG_NAME)) as f:
        cfg = json.load(f)
    state = torch.load(os.path.join(output_dir, WEIGHT_NAME), map_location="cpu", weights_only=True)
    dev = torch.device(device)
    for name, (w_dtype, act_dtype) in cfg["mx_modules"].items():
        lin = get_module(original_model, name)
        assert isinstance(lin, torch.nn.Linear), f"{name}: expected nn.Linear in the float architecture, got {type(lin).__name__}"
        ft = state[name + ".bias"].dtype if (name + ".bias") in state else half_or_fp16(lin.weight.dtype)
        new = MXLinear(lin.in_features, lin.out_features, bias=(name + ".bias") in state, w_dtype=w_dtype, act_dtype=act_dtype,
                       device=dev, float_type=ft)
        _take(state, name, new, dev)
        set_module(original_model, name, new)
    for name, (w_dtype, act_dtype, E, H, I) in cfg.get("mx_experts", {}).items():
        _take_experts(state, original_model, name, dev, is_fused_experts,
                      lambda old: MXExperts(E, H, I, w_dtype=w_dtype, act_dtype=act_dtype, act_fn=old.act_fn, device=dev,
                                            float_type=half_or_fp16(old.gate_up_proj.dtype)))
    for name, (w_dtype, act_dtype, E, H, I, alpha, limit) in cfg.get("mx_gpt_oss_experts", {}).items():
        _take_experts(state, original_model, name, dev, is_gpt_oss_experts,
                      lambda old: MXGptOssExperts(E, H, I, w_dtype=w_dtype, act_dtype=act_dtype, alpha=alpha, limit=limit, device=dev,
                                                  float_type=half_or_fp16(old.gate_up_proj.dtype)))
    original_model.load_state_dict(state, strict=False, assign=True)
    original_model.to(dev)
    original_model.eval()
    original_model.mx_info = cfg.get("mx_quant", {})
    return original_model
