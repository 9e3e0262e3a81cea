"""FP8Linear / FP8Quantizer: per-token / per-channel FP8 linears (the "FP8 dynamic" cell).

The weight is quantised once to OCP e4m3 codes with one fp32 scale per output channel, the activation rows are quantised at run time
with one fp32 scale per token (`inc_fp8_quant_rows` for both), and `inc_fp8_gemm` multiplies the codes on v_mfma_f32_32x32x64_f8f6f4
and applies `row_scale[m] * w_scale[n]` in its epilogue; a decode-sized batch (up to 16 rows) takes `inc_fp8_gemv` on the 16x16x128
form of the instruction.  The specification in bits is the comment of the entry points in include/inc_mi355x.h.
The algorithm is data-free: `prepare` returns the model unchanged and `convert` swaps every selected nn.Linear and, under
`FP8Config(moe_experts=True)`, every selected fused MoE experts module (FP8Experts, experts.py).
`fp8_linear_group` and `fp8_gated_pair` run modules that multiply the same activation as one decode launch (`inc_fp8_gemv_multi`,
`inc_fp8_gemv_gated`).  The forward contract, `_decodes` and `from_float` are QuantLinear's, the group body is `linear_group` and the
quantizer's `_selected` / `convert` are DataFreeQuantizer's (quant_linear.py).
"""

import torch

from .... import ops
from ...utils.utility import is_fused_experts
from ..fused_experts import is_silu
from ..quant_linear import DataFreeQuantizer, QuantLinear, e4m3_table, linear_group, linear_group_plan
from .block import FP8BlockLinear

BLOCK_CELL = ("per_group", "per_block")  # (act_granularity, w_granularity) of the block-scaled cell (block.py)


def is_block_cell(cfg):
    """Whether a layer's dict (fp8_quant_entry) names the block-scaled cell; a dict without the two keys is the per-token cell."""
    return (cfg.get("act_granularity"), cfg.get("w_granularity")) == BLOCK_CELL


class FP8Linear(QuantLinear):
    """nn.Linear with e4m3 weights (per output channel) and e4m3 activations (per token).  Buffers: qweight uint8 [N, Kp], w_scale
    fp32 [N], bias.  Kp = in_features rounded up to 128; the padding columns are zero codes.  forward = inc_fp8_quant_rows(x) ->
    inc_fp8_gemv up to DECODE_MAX_M rows (while DECODE_GEMV is on), inc_fp8_gemm above; nothing is read back to the host."""

    # True = up to DECODE_MAX_M rows go through the decode GEMV (inc_fp8_gemv: one workgroup per 16 weight rows, K split over its waves);
    # False = every batch takes the 256 x 256 tile kernel.  Times of both: profiles/fp8/fp8_gemm_time.log, DESIGN section 8c.
    DECODE_GEMV = True
    DECODE_MAX_M, GEMV_LIMIT = ops.FP8_GEMV_MAX_M, "FP8_GEMV_MAX_M"

    def __init__(self, in_features, out_features, bias=False, device="cuda", float_type=torch.float16):
        dev = self._hip_device(device)
        super().__init__(in_features, out_features, float_type)
        self.register_buffer("qweight", torch.zeros((out_features, self.kp), dtype=torch.uint8, device=dev))
        self.register_buffer("w_scale", torch.zeros(out_features, dtype=torch.float32, device=dev))
        self._register_bias(bias, dev)

    def _quantize_weight(self, w):
        codes, scale = ops.fp8_quant_rows(w, None, self.kp)
        self.qweight.copy_(codes)
        self.w_scale.copy_(scale)

    def _product(self, x2d, out_dtype):
        xq, row_scale = ops.fp8_quant_rows(x2d, None, self.kp)
        product = ops.fp8_gemv if self._decodes(x2d.shape[0]) else ops.fp8_gemm
        return product(xq, row_scale, self.qweight, self.w_scale, self.bias, out_dtype)

    def _group_key(self):
        return self.in_features, self.qweight.device

    def _quantize_rows(self, x2d):
        return ops.fp8_quant_rows(x2d, None, self.kp)

    def _gemm(self, xq, row_scale, out_dtype):
        return ops.fp8_gemm(xq, row_scale, self.qweight, self.w_scale, self.bias, out_dtype)

    @staticmethod
    def _gemv_multi(xq, row_scale, mods, out_dtype):
        return ops.fp8_gemv_multi(xq, row_scale, [m.qweight for m in mods], [m.w_scale for m in mods], [m.bias for m in mods], out_dtype)

    def recover(self, dtype=None):
        """Dequantised weight [N, K]: the code table times w_scale (one fp32 multiply per element), in `dtype` or float_type."""
        w = e4m3_table(self.qweight.device)[self.qweight.long()] * self.w_scale[:, None]
        return w[:, : self.in_features].to(self.float_type if dtype is None else dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"fp8_config=E4M3, act_granularity=per_token, w_granularity=per_channel")


def fp8_linear_group(x, modules):
    """[m(x) for m in modules], bit for bit, for FP8Linear modules that multiply the SAME activation -- q / k / v of an attention block,
    gate / up of an MLP: x is quantised ONCE (each member's own forward quantises it again), and up to FP8Linear.DECODE_MAX_M rows the
    products are ONE launch over the strips of all members (inc_fp8_gemv_multi: the strip body of inc_fp8_gemv); above that,
    inc_fp8_gemm per member on the shared codes.  Every member keeps its buffers and state-dict keys.  Anything else -- a member that
    is not an FP8Linear, mixed widths, fewer than 2 or more than 8 members, x elsewhere or empty, a decode-sized x with DECODE_GEMV off
    -- is the plain list of single forwards."""
    return linear_group(x, list(modules), FP8Linear, ops.FP8_GEMV_MAX_MEMBERS, ops.FP8_GEMV_MAX_M)


# gate / up of a dense gated MLP: True = fp8_gated_pair forms silu(gate(x)) * up(x) inside the decode launch (inc_fp8_gemv_gated),
# False = fp8_linear_group + the activation + the product as torch kernels.  Times of both: profiles/fp8/fp8_group_time.log, DESIGN
# section 8c
GATED_FUSED = True


def fp8_gated_pair(x, gate, up, act_fn=None):
    """act_fn(gate(x)) * up(x) -- the first half of a gated MLP (transformers' LlamaMLP.forward) -- in ONE product launch for a
    decode-sized batch (inc_fp8_gemv_gated): x is quantised once, both products and the SiLU product are one kernel, the product is
    formed in fp32 from the two fp32 values and rounded once.  The unfused form rounds three times (g, u, silu(g)) before its last
    rounding, so the two agree within output rounding, not bit for bit.  act_fn: None (SiLU) or a SiLU module.

    Fused when both members are FP8Linear of one in_features, out_features, device and float_type, x is on that device with
    x.shape[-1] == in_features, the row count decodes on both, act_fn is None or SiLU and GATED_FUSED is on.  Otherwise exactly
    act(g) * u with g, u = fp8_linear_group(x, [gate, up]) and act = F.silu by default.  fp32 x and the reshape: FP8Linear.forward's."""
    if GATED_FUSED and (act_fn is None or is_silu(act_fn)):
        plan = linear_group_plan(x, [gate, up], FP8Linear, ops.FP8_GEMV_MAX_MEMBERS, ops.FP8_GEMV_MAX_M)
        if (plan is not None and plan[2] and gate.out_features == up.out_features and gate.float_type == up.float_type):
            x2d, out_dtype, _ = plan
            xq, row_scale = gate._quantize_rows(x2d)
            h = ops.fp8_gemv_gated(xq, row_scale, gate.qweight, gate.w_scale, gate.bias, up.qweight, up.w_scale, up.bias, out_dtype)
            if x.dtype == torch.float32:
                h = h.float()
            return h.reshape(*x.shape[:-1], gate.out_features)
    g, u = fp8_linear_group(x, [gate, up])
    return (torch.nn.functional.silu(g) if act_fn is None else act_fn(g)) * u


class FP8Quantizer(DataFreeQuantizer):
    """quant_config: {layer name: {"fp8_config", "act_granularity", "w_granularity"}} (fp8_quant_entry).  A layer whose fp8_config is
    "fp32" stays float; a Linear whose granularities are BLOCK_CELL becomes an FP8BlockLinear, any other an FP8Linear.  Besides
    nn.Linear the names may be fused MoE experts modules (is_fused_experts; they are in the mapping under
    FP8Config(moe_experts=True) only), which become FP8Experts.  _selected / prepare / convert: DataFreeQuantizer's."""

    LOG, STAYS_FLOAT = "FP8", ("fp8_config", "fp32")

    def _is_experts(self, mod, cfg):
        return is_fused_experts(mod)

    def _unsupported_reason(self, mod, cfg):
        from .experts import unsupported_reason

        return unsupported_reason(mod, cfg)

    def _quantized(self, mod, cfg, dev):
        from .experts import FP8Experts

        linear_cls = FP8BlockLinear if is_block_cell(cfg) else FP8Linear
        cls = linear_cls if isinstance(mod, torch.nn.Linear) else FP8Experts
        return cls.from_float(mod, device=dev)

    def _leave_info(self, model, names):
        act, w = BLOCK_CELL if any(is_block_cell(self.quant_config[n]) for n in names) else ("per_token", "per_channel")
        model.fp8_info = {"fp8_config": "E4M3", "act_granularity": act, "w_granularity": w}
