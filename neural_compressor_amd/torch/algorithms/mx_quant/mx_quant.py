"""MXLinear / MXQuantizer: OCP microscaling linears (interface of the reference's torch/algorithms/mx_quant/mx.py: `MXLinear`,
`MXQuantizer`; formats of its utils.py `ElemFormat`).

The reference emulates MX: it fake-quantises weights and activations in float and calls F.linear.  Here the same configuration
executes: the weight is quantised once to e4m3 / e2m1 codes with one E8M0 scale per 32 elements along in_features
(`inc_mx_quant`), the activation rows are quantised the same way at run time, and `inc_mx_gemm` multiplies the codes on
v_mfma_scale_f32_32x32x64_f8f6f4, which applies both block scales inside the matrix pipe; a decode-sized batch (up to 16 rows) takes
`inc_mx_gemv` on the 16x16x128 form of the instruction, and `mx_linear_group` sends modules that share an activation out in one
launch.  The specification in bits is the comment of the entry points in include/inc_mi355x.h.  The algorithm
is data-free: `prepare` returns the model unchanged and `convert` swaps every selected nn.Linear.
"""

import torch

from .... import ops
from ....common.utils import logger
from ...utils.utility import get_module, half_or_fp16, is_fused_experts, is_gpt_oss_experts, linear_group_plan, set_module
from ..base_algorithm import Quantizer

FORMATS = {"fp8_e4m3": ops.MX_FP8_E4M3, "fp4": ops.MX_FP4_E2M1}
PAIRS = (("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4"))  # (w_dtype, act_dtype) the GEMM takes


def _code_values(fmt):
    """The value of every code: 256 entries for e4m3 (OCP e4m3fn; 0x7f / 0xff are NaN and never stored), 16 for e2m1."""
    if fmt == ops.MX_FP8_E4M3:
        return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    half = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    return torch.cat([half, -half])


class MXLinear(torch.nn.Module):
    """nn.Linear with MX weights and MX activations.  Buffers: qweight uint8 [N, Kp] (fp8) or [N, Kp/2] (fp4, element 2i in the low
    nibble), w_scale uint8 [N, Kp/32] (E8M0 bytes), bias.  Kp = in_features rounded up to 128; the padding columns are zero codes.
    forward = inc_mx_quant(x) -> inc_mx_gemv up to DECODE_MAX_M rows (while DECODE_GEMV is on), inc_mx_gemm above; nothing is read
    back to the host."""

    # True = up to DECODE_MAX_M rows go through the decode GEMV (inc_mx_gemv: one workgroup per 16 weight rows, K split over its waves);
    # False = every batch takes the 256 x 256 tile kernel.  Times of both: profiles/mx/mx_gemv_time.log, DESIGN section 8b.
    DECODE_GEMV = True
    DECODE_MAX_M = ops.MX_GEMV_MAX_M

    def __init__(self, in_features, out_features, bias=False, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", device="cuda",
                 float_type=torch.float16):
        super().__init__()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"MXLinear needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation.")
        if (w_dtype, act_dtype) not in PAIRS:
            raise NotImplementedError(f"MXQuant on MI355X: (w_dtype, act_dtype) must be one of {PAIRS}, got {(w_dtype, act_dtype)}")
        self.in_features, self.out_features = in_features, out_features
        self.w_dtype, self.act_dtype = w_dtype, act_dtype
        self.w_fmt, self.act_fmt = FORMATS[w_dtype], FORMATS[act_dtype]
        self.kp = ops.mx_padded_k(in_features)
        self.float_type = float_type
        cols = self.kp if self.w_fmt == ops.MX_FP8_E4M3 else self.kp // 2
        self.register_buffer("qweight", torch.zeros((out_features, cols), dtype=torch.uint8, device=dev))
        self.register_buffer("w_scale", torch.zeros((out_features, self.kp // 32), dtype=torch.uint8, device=dev))
        self.register_buffer("bias", torch.zeros(out_features, dtype=float_type, device=dev) if bias else None)

    @classmethod
    @torch.no_grad()
    def from_float(cls, linear, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", device="cuda"):
        ft = half_or_fp16(linear.weight.dtype)
        new = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, w_dtype=w_dtype, act_dtype=act_dtype,
                  device=device, float_type=ft)
        dev = new.qweight.device
        codes, scales = ops.mx_quant(linear.weight.detach().to(dev), new.w_fmt, new.kp)
        new.qweight.copy_(codes)
        new.w_scale.copy_(scales)
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
        xq, xs = ops.mx_quant(x2d, self.act_fmt, self.kp)
        product = ops.mx_gemv if self._decodes(x2d.shape[0]) else ops.mx_gemm
        y = product(xq, xs, self.act_fmt, self.qweight, self.w_scale, self.w_fmt, self.bias, out_dtype)
        if x.dtype == torch.float32:  # an fp32 model keeps seeing fp32 activations (the kernel's epilogue emits 16-bit)
            y = y.float()
        return y.reshape(*lead, self.out_features)

    def _decodes(self, rows):
        return self.DECODE_GEMV and rows <= min(self.DECODE_MAX_M, ops.MX_GEMV_MAX_M)

    def recover(self, dtype=None):
        """Dequantised weight [N, K] (a table lookup times 2^(byte - 127); every value is exact in fp32), in `dtype` or float_type."""
        q = self.qweight
        if self.w_fmt == ops.MX_FP4_E2M1:
            q = torch.stack([q & 0xF, q >> 4], dim=2).reshape(q.shape[0], -1)
        vals = _code_values(self.w_fmt).to(q.device)[q.long()]
        scale = torch.ldexp(torch.ones((), dtype=torch.float32, device=q.device), self.w_scale.to(torch.int32) - 127)
        w = (vals.view(self.out_features, self.kp // 32, 32) * scale[:, :, None]).view(self.out_features, self.kp)
        return w[:, : self.in_features].to(self.float_type if dtype is None else dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"w_dtype={self.w_dtype}, act_dtype={self.act_dtype}, blocksize=32")


def mx_linear_group(x, modules):
    """[m(x) for m in modules], bit for bit, for MXLinear modules that multiply the SAME activation -- q / k / v of an attention block,
    gate / up of an MLP: x is quantised ONCE (each member's own forward quantises it again), and up to MXLinear.DECODE_MAX_M rows the
    products are ONE launch over the strips of all members (inc_mx_gemv_multi: the strip body of inc_mx_gemv); above that, inc_mx_gemm
    per member on the shared codes.  Every member keeps its buffers and state-dict keys.  Anything else -- a member that is not an
    MXLinear, mixed formats or widths, fewer than 2 or more than 8 members, x elsewhere or empty, a decode-sized x with DECODE_GEMV off
    -- is the plain list of single forwards."""
    mods = list(modules)
    plan = linear_group_plan(x, mods, MXLinear, ops.MX_GEMV_MAX_MEMBERS, ops.MX_GEMV_MAX_M,
                             lambda m: (m.in_features, m.qweight.device, m.w_dtype, m.act_dtype))
    if plan is None:
        return [m(x) for m in mods]
    x2d, out_dtype, decode = plan
    m0 = mods[0]
    xq, xs = ops.mx_quant(x2d, m0.act_fmt, m0.kp)
    if decode:
        ys = ops.mx_gemv_multi(xq, xs, m0.act_fmt, [m.qweight for m in mods], [m.w_scale for m in mods], m0.w_fmt,
                               [m.bias for m in mods], out_dtype)
    else:
        ys = [ops.mx_gemm(xq, xs, m.act_fmt, m.qweight, m.w_scale, m.w_fmt, m.bias, out_dtype) for m in mods]
    if x.dtype == torch.float32:
        ys = [y.float() for y in ys]
    return [y.reshape(*x.shape[:-1], m.out_features) for y, m in zip(ys, mods)]


class MXQuantizer(Quantizer):
    """quant_config: {layer name: {"w_dtype", "act_dtype", ...}} (mx_quant_entry).  A layer whose w_dtype is "fp32" stays float.
    Besides nn.Linear the names may be fused MoE experts modules (is_fused_experts; they are in the mapping under
    MXQuantConfig(quant_experts=True)), which become MXExperts, and GPT-OSS experts modules (is_gpt_oss_experts), which become
    MXGptOssExperts when their dict carries "gpt_oss_experts": True (mx_quant_entry sets it under quant_experts=True; without the key
    such a module stays float)."""

    def _selected(self, model):
        from .experts import unsupported_reason

        out = []
        for name, cfg in self.quant_config.items():
            if cfg.get("w_dtype", "fp32") == "fp32":
                continue
            mod = get_module(model, name)
            if isinstance(mod, torch.nn.Linear):
                out.append(name)
            elif is_fused_experts(mod) or (is_gpt_oss_experts(mod) and cfg.get("gpt_oss_experts")):
                why = unsupported_reason(mod, cfg)
                if why is None:
                    out.append(name)
                else:
                    logger.warning("MXQuant: experts module %s stays in floating point: %s", name, why)
        return out

    def prepare(self, model, *args, **kwargs):
        return model  # data-free: nothing to calibrate

    @torch.no_grad()
    def convert(self, model, *args, **kwargs):
        from .experts import MXExperts, MXGptOssExperts

        dev = torch.device("cuda", torch.cuda.current_device())
        model.to(dev)
        model.eval()
        names = self._selected(model)
        if not names:
            logger.warning("MXQuant: no nn.Linear selected, the model is returned unchanged")
        for name in names:
            cfg = self.quant_config[name]
            mod = get_module(model, name)
            cls = MXLinear if isinstance(mod, torch.nn.Linear) else MXGptOssExperts if is_gpt_oss_experts(mod) else MXExperts
            set_module(model, name, cls.from_float(mod, cfg["w_dtype"], cfg["act_dtype"], device=dev))
        model.mx_info = {"blocksize": 32, "round_method": "nearest"}
        return model
