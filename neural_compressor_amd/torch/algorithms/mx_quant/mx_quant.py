"""MXLinear / MXQuantizer: OCP microscaling linears (interface of the reference's torch/algorithms/mx_quant/mx.py: `MXLinear`,
`MXQuantizer`; formats of its utils.py `ElemFormat`).

The reference emulates MX: it fake-quantises weights and activations in float and calls F.linear.  Here the same configuration
executes: the weight is quantised once to e4m3 / e2m1 codes with one E8M0 scale per 32 elements along in_features
(`inc_mx_quant`), the activation rows are quantised the same way at run time, and `inc_mx_gemm` multiplies the codes on
v_mfma_scale_f32_32x32x64_f8f6f4, which applies both block scales inside the matrix pipe; a decode-sized batch (up to 16 rows) takes
`inc_mx_gemv` on the 16x16x128 form of the instruction, and `mx_linear_group` sends modules that share an activation out in one
launch.  The specification in bits is the comment of the entry points in include/inc_mi355x.h.  The algorithm
is data-free: `prepare` returns the model unchanged and `convert` swaps every selected nn.Linear.  The forward contract, `_decodes`
and `from_float` are QuantLinear's, the group body is `linear_group` and the quantizer's `_selected` / `convert` are
DataFreeQuantizer's (quant_linear.py); every class names the (w_dtype, act_dtype) it takes in its own `PAIRS`.
"""

import torch

from .... import ops
from ...utils.utility import is_fused_experts, is_gpt_oss_experts
from ..quant_linear import DataFreeQuantizer, QuantLinear, e4m3_table, linear_group

FORMATS = {"fp8_e4m3": ops.MX_FP8_E4M3, "fp6_e2m3": ops.MX_FP6_E2M3, "fp6_e3m2": ops.MX_FP6_E3M2, "fp4": ops.MX_FP4_E2M1}
PAIRS = (("fp8_e4m3", "fp8_e4m3"), ("fp4", "fp8_e4m3"), ("fp4", "fp4"))  # (w_dtype, act_dtype) every MX cell takes: linears and experts
# the MXFP6 pairs, which only MXLinear takes (inc_mx_gemm / inc_mx_gemv); the activation is never narrower than the weight.  They are a
# table of their own because PAIRS is shared with the experts classes, which reject fp6
FP6_PAIRS = (("fp6_e2m3", "fp6_e2m3"), ("fp6_e3m2", "fp6_e3m2"), ("fp6_e2m3", "fp8_e4m3"), ("fp4", "fp6_e2m3"))
WEIGHT_ONLY_PAIRS = (("fp4", "bf16"), ("fp8_e4m3", "bf16"))  # the weight-only cell: MX weights, bf16 activations


def check_pair(owner, w_dtype, act_dtype):
    """The one refusal of a (w_dtype, act_dtype) outside the table of `owner`: a class (or a module of it) that names the pairs it takes
    as PAIRS and, beside them, the CELL its message carries (MXLinear, MXWeightOnlyLinear, MXExperts, ...)."""
    if (w_dtype, act_dtype) not in owner.PAIRS:
        raise NotImplementedError(f"MXQuant on MI355X{owner.CELL}: (w_dtype, act_dtype) must be one of {owner.PAIRS}, "
                                  f"got {(w_dtype, act_dtype)}")


def _code_values(fmt):
    """The value of every code: 256 entries for e4m3 (OCP e4m3fn; 0x7f / 0xff are NaN and never stored), 64 for e2m3 / e3m2 (sign in
    bit 5, no NaN / Inf codes), 16 for e2m1."""
    if fmt == ops.MX_FP8_E4M3:
        return e4m3_table()
    if fmt in (ops.MX_FP6_E2M3, ops.MX_FP6_E3M2):
        mb, bias = (3, 1) if fmt == ops.MX_FP6_E2M3 else (2, 3)
        mag = torch.arange(32)
        e, m = mag >> mb, (mag & ((1 << mb) - 1)).float()
        half = torch.where(e == 0, m * 2.0 ** (1 - bias - mb), torch.ldexp(1 + m / (1 << mb), e - bias))
        return torch.cat([half, -half])
    half = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    return torch.cat([half, -half])


def mx_wo_product(a, decode, qweight, w_scale, w_fmt, bias, out_dtype):
    """The weight-only cell's chain on rows a [M, K]: the cast to bf16, K zero-padded to a multiple of 8, then inc_mx_wo_gemv if
    `decode` else inc_mx_wo_gemm.  MXWeightOnlyLinear's forward and the dense routes of the two weight-only experts classes."""
    a = a.to(torch.bfloat16)
    if a.shape[1] % 8:
        a = torch.nn.functional.pad(a, (0, 8 - a.shape[1] % 8))
    product = ops.mx_wo_gemv if decode else ops.mx_wo_gemm
    return product(a.contiguous(), qweight, w_scale, w_fmt, bias, out_dtype)


class MXLinear(QuantLinear):
    """nn.Linear with MX weights and MX activations.  Buffers: qweight uint8 [N, Kp] (fp8), [N, Kp*3/4] (fp6_e2m3 / fp6_e3m2: 24 bytes
    per block, element j in bits 6j .. 6j+5) or [N, Kp/2] (fp4, element 2i in the low nibble), w_scale uint8 [N, Kp/32] (E8M0 bytes),
    bias.  Beside PAIRS the class takes the MXFP6 pairs FP6_PAIRS (inc_mx_quant_fp6 and the same two products).  Kp = in_features rounded up to 128; the padding columns are zero codes.
    forward = inc_mx_quant(x) -> inc_mx_gemv up to DECODE_MAX_M rows (while DECODE_GEMV is on), inc_mx_gemm above; nothing is read
    back to the host."""

    # True = up to DECODE_MAX_M rows go through the decode GEMV (inc_mx_gemv: one workgroup per 16 weight rows, K split over its waves);
    # False = every batch takes the 256 x 256 tile kernel.  Times of both: profiles/mx/mx_gemv_time.log, DESIGN section 8b.
    DECODE_GEMV = True
    DECODE_MAX_M, GEMV_LIMIT = ops.MX_GEMV_MAX_M, "MX_GEMV_MAX_M"
    PAIRS, CELL = PAIRS, ""  # the (w_dtype, act_dtype) this class takes, and what check_pair's message calls the cell
    FP6_PAIRS = FP6_PAIRS    # taken too, by this class only (subclasses and the experts classes set it empty or do not have it)

    def __init__(self, in_features, out_features, bias=False, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", device="cuda",
                 float_type=torch.float16):
        dev = self._hip_device(device)
        if (w_dtype, act_dtype) not in self.FP6_PAIRS:
            check_pair(self, w_dtype, act_dtype)
        super().__init__(in_features, out_features, float_type)
        self.w_dtype, self.act_dtype = w_dtype, act_dtype
        self.w_fmt, self.act_fmt = FORMATS[w_dtype], FORMATS.get(act_dtype)  # no format for "bf16": nothing quantises the activation
        cols = ops.mx_code_cols(self.w_fmt, self.kp)
        self.register_buffer("qweight", torch.zeros((out_features, cols), dtype=torch.uint8, device=dev))
        self.register_buffer("w_scale", torch.zeros((out_features, self.kp // 32), dtype=torch.uint8, device=dev))
        self._register_bias(bias, dev)

    @classmethod
    def from_float(cls, linear, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", device="cuda"):
        return super().from_float(linear, device=device, w_dtype=w_dtype, act_dtype=act_dtype)

    def _quantize_weight(self, w):
        codes, scales = ops.mx_quant(w, self.w_fmt, self.kp)
        self.qweight.copy_(codes)
        self.w_scale.copy_(scales)

    def _product(self, x2d, out_dtype):
        xq, xs = ops.mx_quant(x2d, self.act_fmt, self.kp)
        product = ops.mx_gemv if self._decodes(x2d.shape[0]) else ops.mx_gemm
        return product(xq, xs, self.act_fmt, self.qweight, self.w_scale, self.w_fmt, self.bias, out_dtype)

    def _group_key(self):
        return self.in_features, self.qweight.device, self.w_dtype, self.act_dtype

    def _quantize_rows(self, x2d):
        return ops.mx_quant(x2d, self.act_fmt, self.kp)

    def _gemm(self, xq, xs, out_dtype):
        return ops.mx_gemm(xq, xs, self.act_fmt, self.qweight, self.w_scale, self.w_fmt, self.bias, out_dtype)

    @staticmethod
    def _gemv_multi(xq, xs, mods, out_dtype):
        return ops.mx_gemv_multi(xq, xs, mods[0].act_fmt, [m.qweight for m in mods], [m.w_scale for m in mods], mods[0].w_fmt,
                                 [m.bias for m in mods], out_dtype)

    def recover(self, dtype=None):
        """Dequantised weight [N, K] (a table lookup times 2^(byte - 127); every value is exact in fp32), in `dtype` or float_type."""
        q = self.qweight
        if self.w_fmt == ops.MX_FP4_E2M1:
            q = torch.stack([q & 0xF, q >> 4], dim=2).reshape(q.shape[0], -1)
        elif self.w_fmt in (ops.MX_FP6_E2M3, ops.MX_FP6_E3M2):  # 3 bytes = one 24-bit little-endian word = 4 codes
            b = q.view(q.shape[0], -1, 3).to(torch.int32)
            word = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16)
            q = torch.stack([(word >> (6 * i)) & 0x3F for i in range(4)], dim=2).reshape(q.shape[0], -1)
        vals = _code_values(self.w_fmt).to(q.device)[q.long()]
        scale = torch.ldexp(torch.ones((), dtype=torch.float32, device=q.device), self.w_scale.to(torch.int32) - 127)
        w = (vals.view(self.out_features, self.kp // 32, 32) * scale[:, :, None]).view(self.out_features, self.kp)
        return w[:, : self.in_features].to(self.float_type if dtype is None else dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"w_dtype={self.w_dtype}, act_dtype={self.act_dtype}, blocksize=32")


class MXWeightOnlyLinear(MXLinear):
    """nn.Linear with MX weights and bf16 activations (MXQuantConfig(weight_only=True, act_dtype="bf16")): MXLinear's buffers and
    state-dict keys, its from_float (inc_mx_quant on the weight) and its recover; the activations are not quantised.
    forward = inc_mx_wo_gemv up to DECODE_MAX_M rows, inc_mx_wo_gemm above (csrc/gemm_mx_wo.hip: the weights are dequantised in
    registers, y = x @ recover(bfloat16)^T accumulated in fp32); nothing is read back to the host.  The product is computed in
    bf16 whatever the input's type: fp16 and fp32 inputs are cast to bf16 and the output is returned in the input's type (the range
    of an E8M0 scale does not fit fp16, so there is no fp16 product).  An in_features that is no multiple of 8 is zero-padded with
    torch, once per call."""

    # rows up to which the decode GEMV is taken: the measured crossover of the two kernels (profiles/mx/mx_wo_time.log)
    DECODE_MAX_M = ops.MX_GEMV_MAX_M
    PAIRS, CELL, FP6_PAIRS = WEIGHT_ONLY_PAIRS, ", weight-only", ()  # no fp6 in the weight-only cell

    def __init__(self, in_features, out_features, bias=False, w_dtype="fp4", act_dtype="bf16", device="cuda", float_type=torch.float16):
        super().__init__(in_features, out_features, bias=bias, w_dtype=w_dtype, act_dtype=act_dtype, device=device, float_type=float_type)

    @classmethod
    def from_float(cls, linear, w_dtype="fp4", act_dtype="bf16", device="cuda"):
        return super().from_float(linear, w_dtype=w_dtype, act_dtype=act_dtype, device=device)

    def _product(self, x2d, out_dtype):
        return mx_wo_product(x2d, self._decodes(x2d.shape[0]), self.qweight, self.w_scale, self.w_fmt, self.bias, out_dtype)


def mx_linear_group(x, modules):
    """[m(x) for m in modules], bit for bit, for MXLinear modules that multiply the SAME activation -- q / k / v of an attention block,
    gate / up of an MLP: x is quantised ONCE (each member's own forward quantises it again), and up to MXLinear.DECODE_MAX_M rows the
    products are ONE launch over the strips of all members (inc_mx_gemv_multi: the strip body of inc_mx_gemv); above that, inc_mx_gemm
    per member on the shared codes.  Every member keeps its buffers and state-dict keys.  Anything else -- a member that is not an
    MXLinear, mixed formats or widths, fewer than 2 or more than 8 members, x elsewhere or empty, a decode-sized x with DECODE_GEMV off
    -- is the plain list of single forwards."""
    mods = list(modules)
    if any(isinstance(m, MXWeightOnlyLinear) for m in mods):  # no one-launch group for the weight-only cell
        return [m(x) for m in mods]
    return linear_group(x, mods, MXLinear, ops.MX_GEMV_MAX_MEMBERS, ops.MX_GEMV_MAX_M)


class MXQuantizer(DataFreeQuantizer):
    """quant_config: {layer name: {"w_dtype", "act_dtype", ...}} (mx_quant_entry).  A layer whose w_dtype is "fp32" stays float.
    Besides nn.Linear the names may be fused MoE experts modules (is_fused_experts; they are in the mapping under
    MXQuantConfig(quant_experts=True)), which become MXExperts, and GPT-OSS experts modules (is_gpt_oss_experts), which become
    MXGptOssExperts when their dict carries "gpt_oss_experts": True (mx_quant_entry sets it under quant_experts=True; without the key
    such a module stays float).  A dict with "weight_only" picks the weight-only class of each kind (MXWeightOnlyLinear,
    MXWeightOnlyExperts, MXWeightOnlyGptOssExperts).  _selected / prepare / convert: DataFreeQuantizer's."""

    LOG, STAYS_FLOAT = "MXQuant", ("w_dtype", "fp32")

    def _is_experts(self, mod, cfg):
        return is_fused_experts(mod) or (is_gpt_oss_experts(mod) and cfg.get("gpt_oss_experts"))

    def _unsupported_reason(self, mod, cfg):
        from .experts import unsupported_reason

        return unsupported_reason(mod, cfg)

    def _quantized(self, mod, cfg, dev):
        from .experts import MXExperts, MXGptOssExperts, MXWeightOnlyExperts, MXWeightOnlyGptOssExperts

        if isinstance(mod, torch.nn.Linear):
            cls = MXWeightOnlyLinear if cfg.get("weight_only") else MXLinear
        elif cfg.get("weight_only"):
            cls = MXWeightOnlyGptOssExperts if is_gpt_oss_experts(mod) else MXWeightOnlyExperts
        else:
            cls = MXGptOssExperts if is_gpt_oss_experts(mod) else MXExperts
        return cls.from_float(mod, cfg["w_dtype"], cfg["act_dtype"], device=dev)

    def _leave_info(self, model, names):
        model.mx_info = {"blocksize": 32, "round_method": "nearest"}
