"""save / load of a SmoothQuant W8A8 model (interface of the reference's smooth_quant/save_load.py:24 -> static_quant
save / load: `model.save(output_dir)`, `load(output_dir, original_model)`).

The reference stores a TorchScript of the IPEX model (`quantized_model.pt`) plus the IPEX qconfig JSON; neither exists here.
The files keep the reference's names where they mean the same thing:
  quantized_weight.pt   state_dict: int8 `qweight`, `w_scale`, `alpha`, `corr`, `act_scale`, `act_zp`, `input_scale`, bias of every
                        W8A8Linear (a per-token module has no `alpha`, `corr`, `act_scale`, `act_zp`: that is how load tells the two
                        activation cells apart), the (possibly folded) float parameters of everything else
  qconfig.json          {"smooth_quant": {alpha, folding, absorb_to_layer}, "w8a8_modules": [names]}
The file handling and the per-Linear rebuild are utils/utility.py's (save_quantized, open_saved, take_linear, finish_load), shared
with mx_quant/save_load.py and fp8_quant/save_load.py.
"""

from functools import partial

from ...utils.utility import QCONFIG_NAME, WEIGHT_NAME  # noqa: F401  (this module's names for the two files)
from ...utils.utility import finish_load, open_saved, save_quantized, take_linear
from .utility import W8A8Linear


def qconfig_of(model):
    """The content of qconfig.json."""
    info = dict(getattr(model, "sq_info", {}))
    info["absorb_to_layer"] = {k: list(v) for k, v in (info.get("absorb_to_layer") or {}).items()}
    return {"smooth_quant": info, "w8a8_modules": [n for n, m in model.named_modules() if isinstance(m, W8A8Linear)]}


def save(model, output_dir="./saved_results"):
    save_quantized(model, output_dir, qconfig_of(model))


def load(output_dir, original_model, device="cuda"):
    """Rebuild the W8A8 model from the float architecture `original_model` (weights may be on any device, "meta" included)."""
    cfg, state, dev = open_saved(output_dir, device)
    for name in cfg["w8a8_modules"]:
        take_linear(state, original_model, name, dev,
                    partial(W8A8Linear, has_input_scale=(name + ".input_scale") in state,
                            act_quant="static" if (name + ".act_scale") in state else "per_token"))
    finish_load(original_model, state, dev)
    original_model.sq_info = cfg.get("smooth_quant", {})
    original_model._smoothquant_optimized = True
    return original_model
