"""FP8BlockExperts: block-scaled FP8 fused MoE experts for MI355X -- e4m3 weights with one fp32 scale per 128 x 128 block, e4m3
activations with one fp32 scale per token and 128 channels, computed at run time.

This is how DeepSeek-V3 / R1, Qwen3-FP8 and every MoE checkpoint written by transformers' FineGrainedFP8Config store their experts
(`gate_proj` / `up_proj` / `down_proj` `weight` float8_e4m3fn with a `weight_scale_inv` fp32 per 128 x 128 block): `from_finegrained`
runs such tensors, stacked over the experts, byte for byte with nothing re-quantised.  The module replaces a transformers `*Experts`
module (`gate_up_proj [E, 2I, H]`, `down_proj [E, H, I]`, `forward(hidden_states, top_k_index, top_k_weights)`) and forward is six HIP
launches with no host synchronisation: route -> `inc_fp8_quant_groups(x)` -> gate_up product with the SiLU product
(`inc_fp8_block_moe_gemm` mode 0) -> `inc_fp8_quant_groups(h)` -> down product with the routing weight (mode 1) -> combine
(include/inc_mi355x.h, K18e).  The gate half and the up half of gate_up are blocked each from its own row 0, as the
checkpoint's two tensors are.  The forward contract and the dense route's loop are FusedExperts' (fused_experts.py).

`convert_block_experts(model)` is the model-level entry; FP8Quantizer / FP8Config do not reach this module yet (under the block cell
the quantiser leaves experts in floating point, with a warning).
"""

import torch

from .... import ops
from ....common.utils import logger
from ...utils.utility import half_or_fp16, is_fused_experts, set_module
from ..quant_linear import e4m3_table
from .experts import _FP8ExpertsBase, experts_unsupported_reason

BLOCK = ops.FP8_BLOCK


def _blocks(n):
    return (n + BLOCK - 1) // BLOCK


class FP8BlockExperts(_FP8ExpertsBase):
    """Buffers (Kp = K rounded up to 128; the padding columns are zero codes): gate_up_qweight uint8 [E, 2I, Kp(H)], gate_up_w_scale
    fp32 [E, 2, ceil(I/128), Kp(H)/128] (index 1: gate, up), down_qweight uint8 [E, H, Kp(I)], down_w_scale fp32 [E, ceil(H/128),
    Kp(I)/128].  bf16 / fp16 compute in their own dtype, fp32 computes in float_type and is cast back.  The dense route (the referee)
    runs FP8BlockLinear's own kernels (inc_fp8_quant_groups, inc_fp8_block_gemv / inc_fp8_block_gemm) on the gate, up and down slices
    of every expert that was hit."""

    # the fused route serves up to this many routed rows per expert on average (T * top_k <= MOE_MAX_ROWS * E); larger batches take the
    # dense route.  Measured (scripts/fp8_block_moe_time.py, profiles/fp8/fp8_block_moe_time.log; the rule is the script's last line):
    # Qwen3-30B-A3B experts (E 128, k 8) fused 14.5 x faster than dense at T = 4096 (256 rows per expert), a DeepSeek-V3 shaped layer
    # (E 256, k 8) 6.6 x at T = 4096 (128 per expert); the dense route wins at no measured point, and nothing above 256 was measured
    MOE_MAX_ROWS = 256
    _quant = staticmethod(ops.fp8_quant_groups)
    _moe_gemm = "fp8_block_moe_gemm"

    def __init__(self, num_experts, hidden_dim, intermediate_dim, act_fn=None, device="cuda", float_type=torch.float16):
        super().__init__(num_experts, hidden_dim, intermediate_dim, act_fn, device, float_type)
        E, H, I, dev = num_experts, hidden_dim, intermediate_dim, torch.device(device)
        self.register_buffer("gate_up_qweight", torch.zeros((E, 2 * I, self.kp_h), dtype=torch.uint8, device=dev))
        self.register_buffer("gate_up_w_scale", torch.zeros((E, 2, _blocks(I), self.kp_h // BLOCK), dtype=torch.float32, device=dev))
        self.register_buffer("down_qweight", torch.zeros((E, H, self.kp_i), dtype=torch.uint8, device=dev))
        self.register_buffer("down_w_scale", torch.zeros((E, _blocks(H), self.kp_i // BLOCK), dtype=torch.float32, device=dev))

    @classmethod
    @torch.no_grad()
    def from_float(cls, module, device="cuda"):
        """inc_fp8_quant_blocks on every expert's gate, up and down matrix (a block never spans two experts or the two halves).
        Convert-time: a loop of 3 E launches."""
        E, N2, H = module.gate_up_proj.shape
        I = N2 // 2
        new = cls(E, H, I, act_fn=module.act_fn, device=device, float_type=half_or_fp16(module.gate_up_proj.dtype))
        dev = new.gate_up_qweight.device
        gu, dn = module.gate_up_proj.detach().to(dev), module.down_proj.detach().to(dev)
        for e in range(E):
            for half in range(2):
                codes, scale = ops.fp8_quant_blocks(gu[e, half * I:(half + 1) * I], new.kp_h)
                new.gate_up_qweight[e, half * I:(half + 1) * I].copy_(codes)
                new.gate_up_w_scale[e, half].copy_(scale)
            codes, scale = ops.fp8_quant_blocks(dn[e], new.kp_i)
            new.down_qweight[e].copy_(codes)
            new.down_w_scale[e].copy_(scale)
        return new

    @classmethod
    @torch.no_grad()
    def from_finegrained(cls, gate, gate_scale_inv, up, up_scale_inv, down, down_scale_inv, act_fn=None, float_type=torch.bfloat16,
                         device="cuda"):
        """A checkpoint's experts as they are, stacked over the experts: `gate` / `up` float8_e4m3fn (or its uint8 bytes) [E, I, H]
        with `*_scale_inv` fp32 [E, ceil(I/128), ceil(H/128)], `down` [E, H, I] with [E, ceil(H/128), ceil(I/128)] (the factor a code
        is multiplied by, despite its name).  The bytes are zero-padded to Kp and the scales need no padding; nothing is re-quantised."""
        E, I, H = gate.shape
        new = cls(E, H, I, act_fn=act_fn, device=device, float_type=float_type)
        want = {"gate": ((E, I, H), tuple(new.gate_up_w_scale[:, 0].shape)), "up": ((E, I, H), tuple(new.gate_up_w_scale[:, 1].shape)),
                "down": ((E, H, I), tuple(new.down_w_scale.shape))}
        for name, w, s in (("gate", gate, gate_scale_inv), ("up", up, up_scale_inv), ("down", down, down_scale_inv)):
            if w.dtype not in (torch.float8_e4m3fn, torch.uint8):
                raise TypeError(f"{name} must be float8_e4m3fn (or its uint8 bytes), got {w.dtype}")
            if tuple(w.shape) != want[name][0]:
                raise ValueError(f"{name} must be {want[name][0]} beside a gate of {tuple(gate.shape)}, got {tuple(w.shape)}")
            if tuple(s.shape) != want[name][1]:
                raise ValueError(f"{name}_scale_inv must be {want[name][1]} for a {want[name][0]} weight in 128 x 128 blocks, "
                                 f"got {tuple(s.shape)}")
        new.gate_up_qweight[:, :I, :H].copy_(gate.contiguous().view(torch.uint8))
        new.gate_up_qweight[:, I:, :H].copy_(up.contiguous().view(torch.uint8))
        new.down_qweight[:, :, :I].copy_(down.contiguous().view(torch.uint8))
        new.gate_up_w_scale[:, 0].copy_(gate_scale_inv.to(torch.float32))
        new.gate_up_w_scale[:, 1].copy_(up_scale_inv.to(torch.float32))
        new.down_w_scale.copy_(down_scale_inv.to(torch.float32))
        return new

    def recover(self, dtype=None, expert=None):
        """Dequantised weights (gate_up [E, 2I, H], down [E, H, I]) in `dtype` or float_type, or expert `expert`'s two matrices
        [2I, H], [H, I]: the code table times the block's scale, one fp32 multiply per element (FP8BlockLinear.recover per slice and
        half)."""
        dtype = self.float_type if dtype is None else dtype
        sel = slice(None) if expert is None else slice(int(expert), int(expert) + 1)
        I, H = self.intermediate_dim, self.hidden_dim
        table = e4m3_table(self.gate_up_qweight.device)
        gs = self.gate_up_w_scale[sel].repeat_interleave(BLOCK, 2)[:, :, :I].reshape(-1, 2 * I, self.kp_h // BLOCK)
        ds = self.down_w_scale[sel].repeat_interleave(BLOCK, 1)[:, :H]
        out = []
        for q, s, K in ((self.gate_up_qweight[sel], gs, H), (self.down_qweight[sel], ds, I)):
            w = (table[q.long()] * s.repeat_interleave(BLOCK, 2))[..., :K].to(dtype)
            out.append(w if expert is None else w[0])
        return tuple(out)

    @staticmethod
    def _product(a, kp, wq, ws, cdt):
        aq, as_ = ops.fp8_quant_groups(a, kp)
        product = ops.fp8_block_gemv if a.shape[0] <= ops.FP8_GEMV_MAX_M else ops.fp8_block_gemm
        return product(aq, as_, wq, ws, None, cdt)

    def _expert_mlp(self, rows, e, cdt):
        I = self.intermediate_dim
        gate = self._product(rows, self.kp_h, self.gate_up_qweight[e, :I], self.gate_up_w_scale[e, 0], cdt)
        up = self._product(rows, self.kp_h, self.gate_up_qweight[e, I:], self.gate_up_w_scale[e, 1], cdt)
        return self._product((self.act_fn(gate) * up).contiguous(), self.kp_i, self.down_qweight[e], self.down_w_scale[e], cdt)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, "
                f"fp8_config=E4M3, act_granularity=per_group, w_granularity=per_block, block={BLOCK}")


def block_unsupported_reason(module):
    """Why convert_block_experts leaves the fused-experts `module` in floating point (None = it converts it)."""
    return experts_unsupported_reason(module)


@torch.no_grad()
def convert_block_experts(model, names=None, device="cuda"):
    """Swap every fused-experts module of `model` (utility.is_fused_experts; of `names` only when given) for an FP8BlockExperts, in
    place; a module whose activation is not SiLU or that has more than 512 experts stays as it is, with one warning.  Nothing else of
    the model is touched (its Linears are FP8Config's business).  Returns the model."""
    picked = [(n, m) for n, m in model.named_modules() if is_fused_experts(m) and (names is None or n in names)]
    for name, mod in picked:
        why = block_unsupported_reason(mod)
        if why is None:
            set_module(model, name, FP8BlockExperts.from_float(mod, device=device))
        else:
            logger.warning("FP8: experts module %s stays in floating point: %s", name, why)
    return model
