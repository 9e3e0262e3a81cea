"""Registry + module helpers (the subset of the reference's neural_compressor/torch/utils/utility.py the hot path uses).

  register_algo / algos_mapping   reference utility.py:63-82
  fetch_module / set_module       reference utility.py:84-127
  get_quantizer / postprocess_model  reference utility.py:163-201 (quantizer parked on model.quantizer between phases)
  HIP accelerator                 reference auto_accelerator.py:220-268 ("cuda" device strings ARE HIP on ROCm)
"""

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


def half_or_fp16(dtype):
    """The float type a quantised module keeps for a float module of `dtype`: bf16 / fp16 as they are, fp16 for anything else."""
    return dtype if dtype in (torch.float16, torch.bfloat16) else torch.float16


def linear_group_plan(x, mods, cls, max_members, max_rows, key):
    """What `cls` members (FP8Linear / MXLinear) that multiply the same x share, or None where the group is the plain list of forwards:
    (x2d, out_dtype, every member decodes).  2 .. max_members members of one `key(m)` (a tuple that starts with in_features and the
    device), x there and not empty; an fp32 x needs one float_type; the row count decodes on every member or is above max_rows."""
    m0 = mods[0] if mods else None
    ok = (2 <= len(mods) <= max_members and all(isinstance(m, cls) for m in mods) and x.is_cuda and x.numel() > 0
          and x.shape[-1] == m0.in_features and x.device == m0.qweight.device and all(key(m) == key(m0) for m in mods))
    if not ok:
        return None
    half = x.dtype in (torch.float16, torch.bfloat16)
    out_dtype = x.dtype if half else m0.float_type
    x2d = x.reshape(-1, m0.in_features)
    rows = x2d.shape[0]
    decode = [m._decodes(rows) for m in mods]
    if not (half or all(m.float_type == out_dtype for m in mods)) or not (all(decode) or rows > max_rows):
        return None
    return x2d, out_dtype, all(decode)


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
