"""FP8Linear / FP8Quantizer: per-token / per-channel FP8 linears (the "FP8 dynamic" cell).

The weight is quantised once to OCP e4m3 codes with one fp32 scale per output channel, the activation rows are quantised at run time
with one fp32 scale per token (`inc_fp8_quant_rows` for both), and `inc_fp8_gemm` multiplies the codes on v_mfma_f32_32x32x64_f8f6f4
and applies `row_scale[m] * w_scale[n]` in its epilogue; a decode-sized batch (up to 16 rows) takes `inc_fp8_gemv` on the 16x16x128
form of the instruction.  The specification in bits is the comment of the entry points in include/inc_mi355x.h.
The algorithm is data-free: `prepare` returns the model unchanged and `convert` swaps every selected nn.Linear and, under
`FP8Config(moe_experts=True)`, every selected fused MoE experts module (FP8Experts, experts.py).
`fp8_linear_group` and `fp8_gated_pair` run modules that multiply the same activation as one decode launch (`inc_fp8_gemv_multi`,
`inc_fp8_gemv_gated`).
"""

import torch

from .... import ops
from ....common.utils import logger
from ...utils.utility import get_module, half_or_fp16, is_fused_experts, linear_group_plan, set_module
from ..base_algorithm import Quantizer
from ..fused_experts import is_silu


class FP8Linear(torch.nn.Module):
    """nn.Linear with e4m3 weights (per output channel) and e4m3 activations (per token).  Buffers: qweight uint8 [N, Kp], w_scale
    fp32 [N], bias.  Kp = in_features rounded up to 128; the padding columns are zero codes.  forward = inc_fp8_quant_rows(x) ->
    inc_fp8_gemv up to DECODE_MAX_M rows (while DECODE_GEMV is on), inc_fp8_gemm above; nothing is read back to the host."""

    # True = up to DECODE_MAX_M rows go through the decode GEMV (inc_fp8_gemv: one workgroup per 16 weight rows, K split over its waves);
    # False = every batch takes the 256 x 256 tile kernel.  Times of both: profiles/fp8/fp8_gemm_time.log, DESIGN section 8c.
    DECODE_GEMV = True
    DECODE_MAX_M = ops.FP8_GEMV_MAX_M

    def __init__(self, in_features, out_features, bias=False, device="cuda", float_type=torch.float16):
        super().__init__()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"FP8Linear needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation.")
        self.in_features, self.out_features = in_features, out_features
        self.kp = ops.mx_padded_k(in_features)
        self.float_type = float_type
        self.register_buffer("qweight", torch.zeros((out_features, self.kp), dtype=torch.uint8, device=dev))
        self.register_buffer("w_scale", torch.zeros(out_features, dtype=torch.float32, device=dev))
        self.register_buffer("bias", torch.zeros(out_features, dtype=float_type, device=dev) if bias else None)

    @classmethod
    @torch.no_grad()
    def from_float(cls, linear, device="cuda"):
        ft = half_or_fp16(linear.weight.dtype)
        new = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, device=device, float_type=ft)
        dev = new.qweight.device
        codes, scale = ops.fp8_quant_rows(linear.weight.detach().to(dev), None, new.kp)
        new.qweight.copy_(codes)
        new.w_scale.copy_(scale)
        if linear.bias is not None:
            new.bias.copy_(linear.bias.detach().to(ft))
        return new

    def forward(self, input):
        x = input
        lead = x.shape[:-1]
        x2d = x.reshape(-1, self.in_features)
        out_dtype = x.dtype if x.dtype in (torch.float16, torch.bfloat16) else self.float_type
        if x2d.shape[0] == 0:
            return torch.empty((*lead, self.out_features), dtype=torch.float32 if x.dtype == torch.float32 else out_dtype, device=x.device)
        xq, row_scale = ops.fp8_quant_rows(x2d, None, self.kp)
        product = ops.fp8_gemv if self._decodes(x2d.shape[0]) else ops.fp8_gemm
        y = product(xq, row_scale, self.qweight, self.w_scale, self.bias, out_dtype)
        if x.dtype == torch.float32:  # an fp32 model keeps seeing fp32 activations (the kernel's epilogue emits 16-bit)
            y = y.float()
        return y.reshape(*lead, self.out_features)

    def _decodes(self, rows):
        return self.DECODE_GEMV and rows <= min(self.DECODE_MAX_M, ops.FP8_GEMV_MAX_M)

    def recover(self, dtype=None):
        """Dequantised weight [N, K]: the code table times w_scale (one fp32 multiply per element), in `dtype` or float_type."""
        table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(self.qweight.device)
        w = table[self.qweight.long()] * self.w_scale[:, None]
        return w[:, : self.in_features].to(self.float_type if dtype is None else dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"fp8_config=E4M3, act_granularity=per_token, w_granularity=per_channel")


def _group_plan(x, mods):
    return linear_group_plan(x, mods, FP8Linear, ops.FP8_GEMV_MAX_MEMBERS, ops.FP8_GEMV_MAX_M, lambda m: (m.in_features, m.qweight.device))


def fp8_linear_group(x, modules):
    """[m(x) for m in modules], bit for bit, for FP8Linear modules that multiply the SAME activation -- q / k / v of an attention block,
    gate / up of an MLP: x is quantised ONCE (each member's own forward quantises it again), and up to FP8Linear.DECODE_MAX_M rows the
    products are ONE launch over the strips of all members (inc_fp8_gemv_multi: the strip body of inc_fp8_gemv); above that,
    inc_fp8_gemm per member on the shared codes.  Every member keeps its buffers and state-dict keys.  Anything else -- a member that
    is not an FP8Linear, mixed widths, fewer than 2 or more than 8 members, x elsewhere or empty, a decode-sized x with DECODE_GEMV off
    -- is the plain list of single forwards."""
    mods = list(modules)
    plan = _group_plan(x, mods)
    if plan is None:
        return [m(x) for m in mods]
    x2d, out_dtype, decode = plan
    xq, row_scale = ops.fp8_quant_rows(x2d, None, mods[0].kp)
    if decode:
        ys = ops.fp8_gemv_multi(xq, row_scale, [m.qweight for m in mods], [m.w_scale for m in mods], [m.bias for m in mods], out_dtype)
    else:
        ys = [ops.fp8_gemm(xq, row_scale, m.qweight, m.w_scale, m.bias, out_dtype) for m in mods]
    if x.dtype == torch.float32:
        ys = [y.float() for y in ys]
    return [y.reshape(*x.shape[:-1], m.out_features) for y, m in zip(ys, mods)]


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
        plan = _group_plan(x, [gate, up])
        if (plan is not None and plan[2] and gate.out_features == up.out_features and gate.float_type == up.float_type):
            x2d, out_dtype, _ = plan
            xq, row_scale = ops.fp8_quant_rows(x2d, None, gate.kp)
            h = ops.fp8_gemv_gated(xq, row_scale, gate.qweight, gate.w_scale, gate.bias, up.qweight, up.w_scale, up.bias, out_dtype)
            if x.dtype == torch.float32:
                h = h.float()
            return h.reshape(*x.shape[:-1], gate.out_features)
    g, u = fp8_linear_group(x, [gate, up])
    return (torch.nn.functional.silu(g) if act_fn is None else act_fn(g)) * u


class FP8Quantizer(Quantizer):
    """quant_config: {layer name: {"fp8_config"}} (fp8_quant_entry).  A layer whose fp8_config is "fp32" stays float.  Besides
    nn.Linear the names may be fused MoE experts modules (is_fused_experts; they are in the mapping under
    FP8Config(moe_experts=True) only), which become FP8Experts."""

    def _selected(self, model):
        from .experts import unsupported_reason

        out = []
        for name, cfg in self.quant_config.items():
            if cfg.get("fp8_config", "fp32") == "fp32":
                continue
            mod = get_module(model, name)
            if isinstance(mod, torch.nn.Linear):
                out.append(name)
            elif is_fused_experts(mod):
                why = unsupported_reason(mod, cfg)
                if why is None:
                    out.append(name)
                else:
                    logger.warning("FP8: experts module %s stays in floating point: %s", name, why)
        return out

    def prepare(self, model, *args, **kwargs):
        return model  # data-free: nothing to calibrate

    @torch.no_grad()
    def convert(self, model, *args, **kwargs):
        from .experts import FP8Experts

        dev = torch.device("cuda", torch.cuda.current_device())
        model.to(dev)
        model.eval()
        names = self._selected(model)
        if not names:
            logger.warning("FP8: no nn.Linear selected, the model is returned unchanged")
        for name in names:
            mod = get_module(model, name)
            cls = FP8Linear if isinstance(mod, torch.nn.Linear) else FP8Experts
            set_module(model, name, cls.from_float(mod, device=dev))
        model.fp8_info = {"fp8_config": "E4M3", "act_granularity": "per_token", "w_granularity": "per_channel"}
        return model
