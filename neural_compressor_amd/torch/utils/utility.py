"""Registry + module helpers (the subset of the reference's neural_compressor/torch/utils/utility.py the hot path uses).

  register_algo / algos_mapping   reference utility.py:63-82
  fetch_module / set_module       reference utility.py:84-127
  get_quantizer / postprocess_model  reference utility.py:163-201 (quantizer parked on model.quantizer between phases)
  HIP accelerator                 reference auto_accelerator.py:220-268 ("cuda" device strings ARE HIP on ROCm)
"""

import json
import os

import torch

from ...common.utils import Mode, logger

try:  # transformers.Conv1D is quantisable too (reference torch/quantization/config.py:66-71)
    import transformers

    WOQ_WHITE_LIST = (torch.nn.Linear, transformers.Conv1D)
except Exception:  # pragma: no cover
    transformers = None
    WOQ_WHITE_LIST = (torch.nn.Linear,)

def is_fused_experts(module):
    """A transformers MoE experts module that RTN packs (Mixtral / Qwen2-MoE / Qwen3-MoE / OLMoE `*Experts`), recognised by shape:
    3-D `gate_up_proj [E, 2I, H]` and `down_proj [E, H, I]`, no bias parameters, an `act_fn`.  GPT-OSS experts ([E, H, 2I] with
    `*_bias`) do not match."""
    gu, dn = getattr(module, "gate_up_proj", None), getattr(module, "down_proj", None)
    if not isinstance(gu, torch.Tensor) or not isinstance(dn, torch.Tensor) or gu.dim() != 3 or dn.dim() != 3:
        return False
    E, N2, H = gu.shape
    if N2 % 2 or tuple(dn.shape) != (E, H, N2 // 2):
        return False
    if any("bias" in n for n, _ in module.named_parameters(recurse=False)):
        return False
    return hasattr(module, "act_fn")


def is_gpt_oss_experts(module):
    """A transformers GPT-OSS experts module (`GptOssExperts`), recognised by shape: 3-D `gate_up_proj [E, H, 2I]` (gate = columns
    0::2, up = columns 1::2) and `down_proj [E, I, H]`, parameters `gate_up_proj_bias [E, 2I]` and `down_proj_bias [E, H]`, numeric
    attributes `alpha` and `limit` (the clamped SwiGLU).  MXQuantConfig(quant_experts=True) converts it to MXGptOssExperts."""
    gu, dn = getattr(module, "gate_up_proj", None), getattr(module, "down_proj", None)
    if not isinstance(gu, torch.Tensor) or not isinstance(dn, torch.Tensor) or gu.dim() != 3 or dn.dim() != 3:
        return False
    E, H, N2 = gu.shape
    if N2 % 2 or tuple(dn.shape) != (E, N2 // 2, H):
        return False
    params = dict(module.named_parameters(recurse=False))
    gb, db = params.get("gate_up_proj_bias"), params.get("down_proj_bias")
    if gb is None or db is None or tuple(gb.shape) != (E, N2) or tuple(db.shape) != (E, H):
        return False
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)  # noqa: E731
    return num(getattr(module, "alpha", None)) and num(getattr(module, "limit", None))


LM_HEAD_NAMES = [".*lm_head", ".*output_layer", ".*embed_out"]  # reference torch/utils/constants.py:69
PRIORITY_GPTQ, PRIORITY_RTN, PRIORITY_AWQ = 90, 80, 70  # reference torch/utils/constants.py:45-48
PRIORITY_SMOOTH_QUANT = 60
PRIORITY_MX_QUANT = 50
PRIORITY_FP8_QUANT = 40

algos_mapping = {}


def register_algo(name):
    """Register `fn(model, configs_mapping, mode=Mode.X, *args, **kwargs)` under an algorithm name."""

    def deco(fn):
        algos_mapping[name] = fn
        return fn

    return deco


def fetch_module(model, op_name):
    mod = model
    for part in op_name.split("."):
        if not hasattr(mod, part):
            logger.warning("The %s is not present in the model.", op_name)
            return None
        mod = getattr(mod, part)
    return mod


def get_module(model, op_name):
    """Fetch a sub-module by dotted name (reference smooth_quant/utility.py:349-369)."""
    mod = model
    for part in op_name.split("."):
        if part == "":
            continue
        mod = getattr(mod, part)
    return mod


def set_module(model, op_name, new_module):
    parts = op_name.split(".")
    parent = model if len(parts) == 1 else fetch_module(model, ".".join(parts[:-1]))
    if parent is None:
        logger.warning("Setting skipped as the %s is not present in the model.", op_name)
        return None
    setattr(parent, parts[-1], new_module)


def _take(state, name, new, dev):
    """Load `name.*` of `state` into `new` (strict) and drop those keys."""
    own = {k[len(name) + 1:]: v for k, v in state.items() if k.startswith(name + ".")}
    new.load_state_dict({k: v.to(dev) for k, v in own.items()}, strict=True)
    for k in own:
        state.pop(name + "." + k)


def _take_experts(state, model, name, dev, recognise, build):
    """The experts module `name` of a saved model, rebuilt from the float architecture `model`: the float module must pass `recognise`
    (is_fused_experts / is_gpt_oss_experts), `build(old)` makes the empty quantised module, _take fills it and it takes the old one's
    place."""
    old = get_module(model, name)
    what = "a GPT-OSS experts module" if recognise is is_gpt_oss_experts else "a fused experts module"
    assert recognise(old), f"{name}: expected {what} in the float architecture, got {type(old).__name__}"
    new = build(old)
    _take(state, name, new, dev)
    set_module(model, name, new)


def take_linear(state, model, name, dev, build):
    """The quantised Linear `name` of a saved model, rebuilt from the float architecture `model`: `build(in_features, out_features,
    bias=, device=, float_type=)` (a class, or a partial of one) makes the empty module -- with a bias if one was saved, float_type from
    the saved bias or else the float weight -- _take fills it and it takes the nn.Linear's place."""
    lin = get_module(model, name)
    assert isinstance(lin, torch.nn.Linear), f"{name}: expected nn.Linear in the float architecture, got {type(lin).__name__}"
    ft = state[name + ".bias"].dtype if (name + ".bias") in state else half_or_fp16(lin.weight.dtype)
    new = build(lin.in_features, lin.out_features, bias=(name + ".bias") in state, device=dev, float_type=ft)
    _take(state, name, new, dev)
    set_module(model, name, new)


WEIGHT_NAME = "quantized_weight.pt"
QCONFIG_NAME = "qconfig.json"


def save_quantized(model, output_dir, qconfig):
    """The two files of a saved SmoothQuant / MX / FP8 model: `qconfig` as qconfig.json, the state dict (on the CPU) as
    quantized_weight.pt."""
    os.makedirs(output_dir, exist_ok=True)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    with open(os.path.join(output_dir, QCONFIG_NAME), "w") as f:
        json.dump(qconfig, f, indent=2)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(output_dir, WEIGHT_NAME))


def open_saved(output_dir, device):
    """load's preamble: (the content of qconfig.json, the saved state dict on the CPU, torch.device(device))."""
    with open(os.path.join(output_dir, QCONFIG_NAME)) as f:
        cfg = json.load(f)
    state = torch.load(os.path.join(output_dir, WEIGHT_NAME), map_location="cpu", weights_only=True)
    return cfg, state, torch.device(device)


def finish_load(model, state, dev):
    """load's end: what the _take* calls left of `state` goes to the float modules; the model on `dev`, in eval mode."""
    model.load_state_dict(state, strict=False, assign=True)
    model.to(dev)
    model.eval()
    return model


def half_or_fp16(dtype):
    """The float type a quantised module keeps for a float module of `dtype`: bf16 / fp16 as they are, fp16 for anything else."""
    return dtype if dtype in (torch.float16, torch.bfloat16) else torch.float16


get_attr = fetch_module


def set_attr(model, name, value):
    set_module(model, name, value)


def get_quantizer(model, quantizer_cls, quant_config=None, *args, **kwargs):
    if hasattr(model, "quantizer"):
        return model.quantizer
    return quantizer_cls(quant_config=quant_config, *args, **kwargs)


def postprocess_model(model, mode, quantizer):
    if mode == Mode.PREPARE:
        model.quantizer = quantizer
    elif mode in (Mode.CONVERT, Mode.QUANTIZE) and getattr(model, "quantizer", False):
        del model.quantizer


def get_model_device(model):
    for p in model.parameters():
        return p.device
    for b in model.buffers():
        return b.device
    return torch.device("cpu")


from .auto_accelerator import (  # noqa: E402,F401  (the reference exposes these through torch.utils too)
    Auto_Accelerator,
    HIPAccelerator,
    accelerator_registry,
    auto_detect_accelerator,
    register_accelerator,
)


def get_accelerator(device_name="auto"):
    """Reference environ.get_accelerator (environ.py:172): the selected accelerator object.  `INC_TARGET_DEVICE=cpu` /
    `device="cpu"` raise -- there is no CPU path."""
    return auto_detect_accelerator(device_name)


def batch_broadcastable(obj):
    """True when `obj` (a block-forward argument other than the hidden states: tensor / nested tuples, lists, dicts /
    plain Python value) can be reused unchanged for a STACK of calibration batches: every tensor in it has a leading
    dimension of 1 (or is 0-d / 1-d), i.e. it broadcasts over the batch.  Batch-folded arguments such as Bloom / Falcon / MPT
    `alibi` [batch * heads, 1, T] fail this test, and such models are then run one calibration batch per forward, as
    the reference does."""
    import torch

    if isinstance(obj, torch.Tensor):
        # (a 1-D tensor has no batch dimension at all -- e.g. `cache_position` [T] of transformers 4.38+: stacking batches does not
        # change it; the callers' faithful-stacking probe compares a stacked forward with the per-batch ones anyway)
        return obj.dim() <= 1 or obj.shape[0] == 1
    if isinstance(obj, (tuple, list)):
        return all(batch_broadcastable(o) for o in obj)
    if isinstance(obj, dict):
        return all(batch_broadcastable(o) for o in obj.values())
    return True
