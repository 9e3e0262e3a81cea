"""Fused elementwise chains inside the block forwards that the GPTQ driver issues (csrc/fwd_elementwise.hip).

A calibration forward of a Llama block spends a quarter of its time in 30-odd elementwise torch kernels: LlamaRMSNorm (6 launches,
two of them over an fp32 copy), apply_rotary_pos_emb (7 per tensor) and act_fn(gate) * up (2).  `FusedForward.around(block)` swaps the
three for one HIP kernel each WHILE THAT FORWARD RUNS, under the same rule as the batch stacking of `_run_block`: only where it is
provably the same computation.

* Recognition is by exact identity of the Hugging Face objects: `type(m) is LlamaRMSNorm`, `type(m) is LlamaMLP` (SiLU activation,
  bias-free projections), and the module global `modeling_llama.apply_rotary_pos_emb` still being the function the module defined.
  Subclasses, other model families, modules that already carry an instance-level `forward` (hub kernels, offload hooks) run eager.
* Bit-identity is enforced at run time: the first time an op meets a new (block class, dtype, shape) in a run it is computed both ways
  on its real inputs and the bit patterns and strides must be equal.  One mismatch turns the feature off for the rest of the run, with
  one warning; that forward hands on the eager values.
* Nothing stays patched: the instance attributes and the module global are put back when the forward returns or raises.
* INC_MI355X_GPTQ_FUSED_FORWARD=0 turns it off.

GEMMs and attention are run, not rewritten; the projections of the MLP are still called as modules, in eager's order (gate, up, down), so
forward pre-hooks (the Hessian hooks, the capture stop) fire exactly as before.
"""

import contextlib
import os
import threading

import torch

from .... import ops
from ....common.utils import logger

ENV_SWITCH = "INC_MI355X_GPTQ_FUSED_FORWARD"
_DTYPES = (torch.bfloat16, torch.float16)

try:  # the objects this module recognises; without transformers (or without its Llama) nothing is ever substituted
    from transformers.models.llama import modeling_llama as _llama

    _ORIG_ROPE = _llama.apply_rotary_pos_emb
    if getattr(_ORIG_ROPE, "__module__", None) != _llama.__name__ or getattr(_ORIG_ROPE, "__name__", None) != "apply_rotary_pos_emb":
        _ORIG_ROPE = None  # already replaced by someone else when this module was imported
except Exception:  # pragma: no cover - transformers is optional
    _llama, _ORIG_ROPE = None, None


def switch_on():
    return os.environ.get(ENV_SWITCH, "1") != "0"


def _usable(*tensors):
    t0 = tensors[0]
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device != t0.device or t.dtype != t0.dtype:
            return False
        if t.requires_grad and torch.is_grad_enabled():
            return False
    return t0.dtype in _DTYPES


def _same_bits(a, b):
    """Equal shape, dtype, strides and bit patterns (NaNs count)."""
    if a.shape != b.shape or a.dtype != b.dtype or a.stride() != b.stride():
        return False
    return bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))


# ---- the three ops: fused where the library takes the call, else None (the caller runs eager) ------------------------------------
def silu_mul(gate, up):
    if not (_usable(gate, up) and gate.is_contiguous() and up.is_contiguous()):
        return None
    return ops.fwd_silu_mul(gate, up)


def rmsnorm(x, weight, eps):
    if not (_usable(x, weight) and x.dim() >= 2 and x.is_contiguous() and weight.is_contiguous()):
        return None
    return ops.fwd_rmsnorm(x, weight, eps)


def rmsnorm_routed(module, x):
    """(LlamaRMSNorm.forward(module, x), "fused" | "eager"): which route the call took."""
    out = rmsnorm(x, module.weight, module.variance_epsilon)
    if out is not None:
        return out, "fused"
    return type(module).forward(module, x), "eager"


_ROPE_STRIDES = {}  # (shapes, strides, dtype) -> strides of eager's q_embed / k_embed


def _eager_rope_strides(q, k, cos, sin):
    """The strides eager's results have for these operands, from a run of the original function on meta tensors (the same stride
    propagation, no kernels); cached."""
    key = (q.shape, q.stride(), k.shape, k.stride(), cos.shape, cos.stride(), sin.stride(), q.dtype)
    got = _ROPE_STRIDES.get(key)
    if got is None:
        mq, mk, mc, ms = (torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device="meta") for t in (q, k, cos, sin))
        eq, ek = _ORIG_ROPE(mq, mk, mc, ms)
        got = (tuple(eq.stride()), tuple(ek.stride())) if eq.shape == q.shape and ek.shape == k.shape else False
        if len(_ROPE_STRIDES) > 256:
            _ROPE_STRIDES.clear()
        _ROPE_STRIDES[key] = got
    return got


def rope(q, k, cos, sin):
    if _ORIG_ROPE is None or not _usable(q, k, cos, sin) or q.dim() != 4 or k.dim() != 4 or cos.dim() != 3 or sin.dim() != 3:
        return None
    if q.stride(3) != 1 or k.stride(3) != 1 or not cos.is_contiguous() or not sin.is_contiguous():
        return None
    strides = _eager_rope_strides(q, k, cos, sin)
    if not strides:
        return None
    return ops.fwd_rope(q, k, cos, sin, strides[0], strides[1])


# ---- the substitution -------------------------------------------------------------------------------------------------------------
_tls = threading.local()  # .active: the FusedForward / block whose forward runs on this thread (read by the patched module global)
_rope_lock = threading.Lock()
_rope_users = 0


def _rope_entry(q, k, cos, sin, *args, **kwargs):
    """What modeling_llama.apply_rotary_pos_emb is while a substituted forward runs."""
    active = getattr(_tls, "active", None)
    unsqueeze_dim = args[0] if args else kwargs.get("unsqueeze_dim", 1)
    if active is None or len(args) > 1 or (kwargs and set(kwargs) != {"unsqueeze_dim"}) or unsqueeze_dim != 1:
        return _ORIG_ROPE(q, k, cos, sin, *args, **kwargs)
    state, block = active

    def check(fused, ref):
        return _same_bits(fused[0], ref[0]) and _same_bits(fused[1], ref[1])

    shape = (tuple(q.shape), tuple(k.shape), tuple(cos.shape)) if isinstance(q, torch.Tensor) and isinstance(k, torch.Tensor) and isinstance(cos, torch.Tensor) else None
    return state.dispatch("rotary embedding", block, getattr(q, "dtype", None), shape, lambda: rope(q, k, cos, sin),
                          lambda: _ORIG_ROPE(q, k, cos, sin, *args, **kwargs), check)


def _is_silu(act):
    if type(act) is torch.nn.SiLU:
        return not act.inplace
    try:
        from transformers.activations import SiLUActivation
    except Exception:  # pragma: no cover
        return False
    return type(act) is SiLUActivation


class FusedForward:
    """Per-run state of the substitution: whether a probe has failed, which (op, block class, dtype, shape) have passed theirs."""

    def __init__(self):
        self.disabled = False
        self.verified = set()
        self.fused_calls = 0  # calls answered by a fused kernel (probe calls included)

    def dispatch(self, op, block, dtype, shape, fused_fn, eager_fn, same=_same_bits):
        if self.disabled or shape is None:
            return eager_fn()
        key = (op, type(block), dtype, shape)
        fused = fused_fn()
        if fused is None:  # declined: not on the device, a shape the kernel does not take, ...
            return eager_fn()
        self.fused_calls += 1
        if key in self.verified:
            return fused
        ref = eager_fn()
        if same(fused, ref):
            self.verified.add(key)
        else:
            self.disabled = True
            logger.warning(f"GPTQ fused forward: the fused {op} kernel does not reproduce eager bit for bit on this model's tensors "
                           f"({dtype}, shape {shape}); the fused forward is off for the rest of the run")
        return ref

    def _norm_forward(self, block, m):
        def forward(hidden_states):
            eager = lambda: type(m).forward(m, hidden_states)  # noqa: E731
            if not isinstance(hidden_states, torch.Tensor):
                return eager()
            return self.dispatch("RMSNorm", block, hidden_states.dtype, tuple(hidden_states.shape),
                                 lambda: rmsnorm(hidden_states, m.weight, m.variance_epsilon), eager)

        return forward

    def _mlp_forward(self, block, m):
        def forward(x):
            g = m.gate_proj(x)
            u = m.up_proj(x)
            eager = lambda: m.act_fn(g) * u  # noqa: E731
            if isinstance(g, torch.Tensor) and isinstance(u, torch.Tensor):
                h = self.dispatch("SiLU-mul", block, g.dtype, tuple(g.shape), lambda: silu_mul(g, u), eager)
            else:
                h = eager()
            return m.down_proj(h)

        return forward

    @contextlib.contextmanager
    def around(self, block):
        """Substitute the three ops for the duration of one forward of `block`; everything is put back on exit, by exception too."""
        global _rope_users
        if self.disabled or _llama is None or not switch_on() or not isinstance(block, torch.nn.Module):
            yield
            return
        patched, rope_on = [], False
        prev_active = getattr(_tls, "active", None)
        try:
            for m in block.modules():
                if "forward" in m.__dict__:
                    continue  # somebody else's instance-level forward: not the HF object any more
                if type(m) is _llama.LlamaRMSNorm:
                    m.forward = self._norm_forward(block, m)
                    patched.append(m)
                elif type(m) is _llama.LlamaMLP:
                    if _is_silu(m.act_fn) and all(getattr(p, "bias", None) is None for p in (m.gate_proj, m.up_proj, m.down_proj)):
                        m.forward = self._mlp_forward(block, m)
                        patched.append(m)
                elif type(m) is _llama.LlamaAttention and _ORIG_ROPE is not None and not rope_on:
                    with _rope_lock:
                        if _llama.apply_rotary_pos_emb is _ORIG_ROPE or (_rope_users > 0 and _llama.apply_rotary_pos_emb is _rope_entry):
                            _llama.apply_rotary_pos_emb = _rope_entry
                            _rope_users += 1
                            rope_on = True
            _tls.active = (self, block)
            yield
        finally:
            _tls.active = prev_active
            for m in patched:
                m.__dict__.pop("forward", None)
            if rope_on:
                with _rope_lock:
                    _rope_users -= 1
                    if _rope_users == 0:
                        _llama.apply_rotary_pos_emb = _ORIG_ROPE
