"""save / load of an FP8 model (`model.save(output_dir)`, `load(output_dir, original_model)`), the files of mx_quant/save_load.py:
  quantized_weight.pt   state_dict: uint8 `qweight`, fp32 `w_scale`, bias of every FP8Linear; the float parameters of everything else
  qconfig.json          {"fp8_quant": {fp8_config, act_granularity, w_granularity}, "fp8_modules": [name, ...],
                         "fp8_experts": {name: [E, H, I]}}
FP8Experts modules save their four buffers under their own names.  The "fp8_experts" key is written only when the model has such
modules; a directory without it (a model without them, or one written before FP8Experts existed) loads as before.
"""

import json
import os

import torch

from ...utils.utility import _take, _take_experts, get_module, half_or_fp16, is_fused_experts, set_module
from .experts import FP8Experts
from .fp8_quant import FP8Linear

WEIGHT_NAME = "quantized_weight.pt"
QCONFIG_NAME = "qconfig.json"


def qconfig_of(model):
    """The content of qconfig.json."""
    cfg = {"fp8_quant": dict(getattr(model, "fp8_info", {})),
           "fp8_modules": [n for n, m in model.named_modules() if isinstance(m, FP8Linear)]}
    experts = {n: [m.num_experts, m.hidden_dim, m.intermediate_dim] for n, m in model.named_modules() if isinstance(m, FP8Experts)}
    if experts:  # a model without FP8Experts writes the file it always wrote
        cfg["fp8_experts"] = experts
    return cfg


def save(model, output_dir="./saved_results"):
    os.makedirs(output_dir, exist_ok=True)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    with open(os.path.join(output_dir, QCONFIG_NAME), "w") as f:
        json.dump(qconfig_of(model), f, indent=2)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(output_dir, WEIGHT_NAME))


def load(output_dir, original_model, device="cuda"):
    """Rebuild the FP8 model from the float architecture `original_model` (weights may be on any device, "meta" included)."""
    with open(os.path.join(output_dir, QCONFIG_NAME)) as f:
        cfg = json.load(f)
    state = torch.load(os.path.join(output_dir, WEIGHT_NAME), map_location="cpu", weights_only=True)
    dev = torch.device(device)
    for name in cfg["fp8_modules"]:
        lin = get_module(original_model, name)
        assert isinstance(lin, torch.nn.Linear), f"{name}: expected nn.Linear in the float architecture, got {type(lin).__name__}"
        ft = state[name + ".bias"].dtype if (name + ".bias") in state else half_or_fp16(lin.weight.dtype)
        new = FP8Linear(lin.in_features, lin.out_features, bias=(name + ".bias") in state, device=dev, float_type=ft)
        _take(state, name, new, dev)
        set_module(original_model, name, new)
    for name, (E, H, I) in cfg.get("fp8_experts", {}).items():
        _take_experts(state, original_model, name, dev, is_fused_experts,
                      lambda old: FP8Experts(E, H, I, act_fn=old.act_fn, device=dev, float_type=half_or_fp16(old.gate_up_proj.dtype)))
    original_model.load_state_dict(state, strict=False, assign=True)
    original_model.to(dev)
    original_model.eval()
    original_model.fp8_info = cfg.get("fp8_quant", {})
    return original_model
