"""FP8BlockLinear: block-scaled FP8 linears -- e4m3 weights with one fp32 scale per 128 x 128 block, e4m3 activations with one fp32
scale per token and 128 channels, computed at run time.

This is the storage scheme of DeepSeek-V3 / R1, Qwen3-FP8 and every checkpoint written by transformers' FineGrainedFP8Config (`weight`
float8_e4m3fn [N, K], `weight_scale_inv` fp32 [ceil(N/128), ceil(K/128)]): `from_finegrained` runs such tensors byte for byte, with
nothing re-quantised.  `inc_fp8_quant_groups` quantises the activation, `inc_fp8_block_gemm` multiplies the codes on
v_mfma_f32_32x32x64_f8f6f4 and promotes every K-tile's sum with `xs[m, kt] * ws[n / 128, kt]` inside its K loop; a decode-sized batch
(up to 16 rows) takes `inc_fp8_block_gemv` on the 16x16x128 form.  The specification in bits is the comment of the entry points in
include/inc_mi355x.h.  The fused MoE experts of such checkpoints are FP8BlockExperts (block_experts.py), reached
through `convert_block_experts`, not yet through FP8Config.  Not built: group launches and the gated pair (`fp8_linear_group` /
`fp8_gated_pair` see a module that is not an FP8Linear and run the plain forwards), static scales, UE8M0 scales.
The forward contract, `_decodes` and `from_float` are QuantLinear's (quant_linear.py).
"""

import torch

from .... import ops
from ..quant_linear import QuantLinear, e4m3_table

BLOCK = ops.FP8_BLOCK


class FP8BlockLinear(QuantLinear):
    """Buffers: qweight uint8 [N, Kp], w_scale fp32 [ceil(N/128), Kp/128], bias.  Kp = in_features rounded up to 128; the padding
    columns are zero codes.  forward = inc_fp8_quant_groups(x) -> inc_fp8_block_gemv up to DECODE_MAX_M rows (while DECODE_GEMV is on),
    inc_fp8_block_gemm above; nothing is read back to the host."""

    # as FP8Linear's switch.  Times of both routes: profiles/fp8/fp8_block_time.log, DESIGN section 8c
    DECODE_GEMV = True
    DECODE_MAX_M, GEMV_LIMIT = ops.FP8_GEMV_MAX_M, "FP8_GEMV_MAX_M"

    def __init__(self, in_features, out_features, bias=False, device="cuda", float_type=torch.float16):
        dev = self._hip_device(device)
        super().__init__(in_features, out_features, float_type)
        blocks = ((out_features + BLOCK - 1) // BLOCK, self.kp // BLOCK)
        self.register_buffer("qweight", torch.zeros((out_features, self.kp), dtype=torch.uint8, device=dev))
        self.register_buffer("w_scale", torch.zeros(blocks, dtype=torch.float32, device=dev))
        self._register_bias(bias, dev)

    def _quantize_weight(self, w):
        codes, scale = ops.fp8_quant_blocks(w, self.kp)
        self.qweight.copy_(codes)
        self.w_scale.copy_(scale)

    @classmethod
    @torch.no_grad()
    def from_finegrained(cls, weight, weight_scale_inv, bias=None, float_type=torch.bfloat16, device="cuda"):
        """A checkpoint's tensors as they are: `weight` float8_e4m3fn (or its uint8 bytes) [N, K], `weight_scale_inv` fp32
        [ceil(N/128), ceil(K/128)] (the factor a code is multiplied by, despite its name).  The bytes are zero-padded to Kp and the
        scales need no padding (ceil(K/128) = Kp/128); nothing is re-quantised."""
        N, K = weight.shape
        new = cls(K, N, bias=bias is not None, device=device, float_type=float_type)
        if weight.dtype not in (torch.float8_e4m3fn, torch.uint8):
            raise TypeError(f"weight must be float8_e4m3fn (or its uint8 bytes), got {weight.dtype}")
        if tuple(weight_scale_inv.shape) != tuple(new.w_scale.shape):
            raise ValueError(f"weight_scale_inv must be {tuple(new.w_scale.shape)} for a [{N}, {K}] weight in 128 x 128 blocks, "
                             f"got {tuple(weight_scale_inv.shape)}")
        new.qweight[:, :K].copy_(weight.contiguous().view(torch.uint8))
        new.w_scale.copy_(weight_scale_inv.to(torch.float32))
        if bias is not None:
            new.bias.copy_(bias.detach().to(float_type))
        return new

    def _product(self, x2d, out_dtype):
        xq, xs = ops.fp8_quant_groups(x2d, self.kp)
        product = ops.fp8_block_gemv if self._decodes(x2d.shape[0]) else ops.fp8_block_gemm
        return product(xq, xs, self.qweight, self.w_scale, self.bias, out_dtype)

    def recover(self, dtype=None):
        """Dequantised weight [N, K]: the code table times the block's scale (one fp32 multiply per element), in `dtype` or float_type."""
        scale = self.w_scale.repeat_interleave(BLOCK, 0)[: self.out_features].repeat_interleave(BLOCK, 1)
        w = e4m3_table(self.qweight.device)[self.qweight.long()] * scale
        return w[:, : self.in_features].to(self.float_type if dtype is None else dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"fp8_config=E4M3, act_granularity=per_group, w_granularity=per_block, block={BLOCK}")
