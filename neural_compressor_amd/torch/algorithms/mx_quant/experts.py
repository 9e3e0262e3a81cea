"""MX fused MoE experts for MI355X.

transformers (5.x) holds the experts of a Mixtral / Qwen2-MoE / Qwen3-MoE / OLMoE layer in one `*Experts` module with two 3-D
parameters, `gate_up_proj [E, 2I, H]` (gate rows 0..I-1, up rows I..2I-1) and `down_proj [E, H, I]`, and a
`forward(hidden_states, top_k_index, top_k_weights)` that loops over the experts that were hit.  `MXExperts` replaces such a module
under `MXQuantConfig(quant_experts=True)`: every expert's two matrices are MX-quantised as `MXLinear` quantises a weight (slice e of
every buffer is byte for byte what `inc_mx_quant` writes for expert e's matrix), and forward is six HIP launches with no host
synchronisation: route -> quantise x -> gate_up product with the SiLU product (`inc_mx_moe_gemm` mode 0) -> quantise h -> down product
with the routing weight (mode 1) -> combine (include/inc_mi355x.h, K16e).

`MXGptOssExperts` does the same for transformers' `GptOssExperts` (`gate_up_proj [E, H, 2I]` with gate and up interleaved,
`down_proj [E, I, H]`, two biases, a clamped SwiGLU) through `inc_mx_moe_gemm_glu`, and `from_mxfp4` takes the tensors of an MXFP4
checkpoint as they are.  The forward contract and the dense route's loop are FusedExperts' (fused_experts.py).
"""

import torch

from .... import ops
from ...utils.utility import half_or_fp16, is_gpt_oss_experts
from ..fused_experts import MAX_EXPERTS, FusedExperts, is_silu
from .mx_quant import FORMATS, PAIRS, _code_values


def _cols(fmt, kp):
    return kp if fmt == ops.MX_FP8_E4M3 else kp // 2


class MXExperts(FusedExperts):
    """Fused experts with MX weights and MX activations.  Buffers (Kp = K rounded up to 128, uint8): gate_up_qweight [E, 2I, Kp(H)]
    (fp8) or [E, 2I, Kp(H)/2] (fp4), gate_up_w_scale [E, 2I, Kp(H)/32], down_qweight [E, H, Kp(I) or Kp(I)/2], down_w_scale
    [E, H, Kp(I)/32].  bf16 / fp16 compute in their own dtype, fp32 computes in float_type and is cast back (as MXLinear.forward).
    The dense route (the referee) runs MXLinear's own kernels (inc_mx_quant, inc_mx_gemv / inc_mx_gemm) on the slices of every expert
    that was hit."""

    # the fused route serves up to this many routed rows per expert on average (T * top_k <= MOE_MAX_ROWS * E); larger batches take the
    # dense route.  Measured (scripts/mx_moe_time.py, profiles/mx/mx_moe_time.log; the rule is the script's last line): Mixtral
    # (E 8, k 2) fused 1.15 - 1.36 x faster than dense at T = 1024 (256 rows per expert), dense 2.1 - 2.5 x faster at T = 4096 (1024);
    # Qwen3-MoE (E 128, k 8) fused 10.8 - 13.8 x faster at T = 4096 (256 per expert)
    MOE_MAX_ROWS = 256

    def __init__(self, num_experts, hidden_dim, intermediate_dim, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", act_fn=None, device="cuda",
                 float_type=torch.float16):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"MXExperts needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation.")
        if (w_dtype, act_dtype) not in PAIRS:
            raise NotImplementedError(f"MXQuant on MI355X: (w_dtype, act_dtype) must be one of {PAIRS}, got {(w_dtype, act_dtype)}")
        super().__init__(num_experts, hidden_dim, intermediate_dim, act_fn)
        E, H, I = num_experts, hidden_dim, intermediate_dim
        self.w_dtype, self.act_dtype = w_dtype, act_dtype
        self.w_fmt, self.act_fmt = FORMATS[w_dtype], FORMATS[act_dtype]
        self.kp_h, self.kp_i = ops.mx_padded_k(H), ops.mx_padded_k(I)
        self.float_type = float_type
        for prefix, N, kp in (("gate_up", 2 * I, self.kp_h), ("down", H, self.kp_i)):
            self.register_buffer(f"{prefix}_qweight", torch.zeros((E, N, _cols(self.w_fmt, kp)), dtype=torch.uint8, device=dev))
            self.register_buffer(f"{prefix}_w_scale", torch.zeros((E, N, kp // 32), dtype=torch.uint8, device=dev))

    @classmethod
    @torch.no_grad()
    def from_float(cls, module, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", device="cuda"):
        """One inc_mx_quant on the [E * N, K] view of each parameter: MX blocks run along K inside a row, so this is each expert
        quantised on its own."""
        E, N2, H = module.gate_up_proj.shape
        I = N2 // 2
        new = cls(E, H, I, w_dtype=w_dtype, act_dtype=act_dtype, act_fn=module.act_fn, device=device,
                  float_type=half_or_fp16(module.gate_up_proj.dtype))
        dev = new.gate_up_qweight.device
        new._quantize(module.gate_up_proj.detach().to(dev), module.down_proj.detach().to(dev))
        return new

    def _quantize(self, gate_up, down):
        """Float matrices in the kernel's order (gate_up [E, 2I, H], down [E, H, I], on the module's device) -> the four buffers."""
        E, H, I = self.num_experts, self.hidden_dim, self.intermediate_dim
        for prefix, p, N, K, kp in (("gate_up", gate_up, 2 * I, H, self.kp_h), ("down", down, H, I, self.kp_i)):
            codes, scales = ops.mx_quant(p.contiguous().reshape(E * N, K), self.w_fmt, kp)
            self._buffers[f"{prefix}_qweight"].copy_(codes.view(E, N, -1))
            self._buffers[f"{prefix}_w_scale"].copy_(scales.view(E, N, -1))

    def recover(self, dtype=None, expert=None):
        """Dequantised weights (gate_up [E, 2I, H], down [E, H, I]) in `dtype` or float_type, or expert `expert`'s two matrices
        [2I, H], [H, I]: a table lookup times 2^(byte - 127), every value exact in fp32 (MXLinear.recover per slice)."""
        dtype = self.float_type if dtype is None else dtype
        sel = slice(None) if expert is None else slice(int(expert), int(expert) + 1)
        out = []
        for prefix, K, kp in (("gate_up", self.hidden_dim, self.kp_h), ("down", self.intermediate_dim, self.kp_i)):
            q, s = self._buffers[f"{prefix}_qweight"][sel], self._buffers[f"{prefix}_w_scale"][sel]
            if self.w_fmt == ops.MX_FP4_E2M1:
                q = torch.stack([q & 0xF, q >> 4], dim=3).reshape(q.shape[0], q.shape[1], -1)
            vals = _code_values(self.w_fmt).to(q.device)[q.long()]
            scale = torch.ldexp(torch.ones((), dtype=torch.float32, device=q.device), s.to(torch.int32) - 127)
            w = (vals.view(q.shape[0], q.shape[1], kp // 32, 32) * scale[..., None]).view(q.shape[0], q.shape[1], kp)[..., :K].to(dtype)
            out.append(w if expert is None else w[0])
        return tuple(out)

    def _fusable(self):
        # inc_moe_combine stores four columns at a time
        return is_silu(self.act_fn) and self.num_experts <= MAX_EXPERTS and self.hidden_dim % 4 == 0

    def _compute_dtype(self, x):
        return x.dtype if x.dtype in (torch.float16, torch.bfloat16) else self.float_type

    def _fused_forward(self, x2d, idx, w, cdt):
        """Six launches in stream order; every buffer is allocated per call and nothing is kept.  Rows of h past the route's valid
        positions hold whatever torch.empty gave: the quantiser is total on any bit pattern and nothing reads its output there."""
        T, k = idx.shape
        E, af, wf = self.num_experts, self.act_fmt, self.w_fmt
        route = ops.moe_route(idx, E)
        xq, xs = ops.mx_quant(x2d, af, self.kp_h)
        h = ops.mx_moe_gemm(0, xq, xs, af, route, self.gate_up_qweight, self.gate_up_w_scale, wf, T, k, out_dtype=cdt)
        hq, hs = ops.mx_quant(h, af, self.kp_i)
        y = ops.mx_moe_gemm(1, hq, hs, af, route, self.down_qweight, self.down_w_scale, wf, T, k, routing_weights=w)
        return ops.moe_combine(y, route, T, k, E, cdt)

    def _product(self, a, prefix, e, kp, cdt):
        aq, as_ = ops.mx_quant(a, self.act_fmt, kp)
        product = ops.mx_gemv if a.shape[0] <= ops.MX_GEMV_MAX_M else ops.mx_gemm
        return product(aq, as_, self.act_fmt, self._buffers[f"{prefix}_qweight"][e], self._buffers[f"{prefix}_w_scale"][e], self.w_fmt,
                       None, cdt)

    def _expert_mlp(self, rows, e, cdt):
        gate, up = self._product(rows, "gate_up", e, self.kp_h, cdt).chunk(2, dim=-1)
        return self._product((self.act_fn(gate) * up).contiguous(), "down", e, self.kp_i, cdt)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, "
                f"w_dtype={self.w_dtype}, act_dtype={self.act_dtype}, blocksize=32")


def unsupported_reason(module, cfg):
    """Why MXQuant leaves the fused-experts `module` in float under `cfg` (None = it converts it)."""
    E = module.gate_up_proj.shape[0]
    pair = (cfg.get("w_dtype"), cfg.get("act_dtype"))
    if pair not in PAIRS:
        return f"(w_dtype, act_dtype)={pair} is not one of {PAIRS}"
    if is_gpt_oss_experts(module):  # no act_fn: the clamped SwiGLU is the kernel's; there is no dense-only fall-back to keep
        if E > MAX_EXPERTS:
            return f"E={E} must be at most {MAX_EXPERTS}"
        if module.gate_up_proj.shape[1] % 4:
            return f"H={module.gate_up_proj.shape[1]} must be a multiple of 4"
        return None
    if not is_silu(getattr(module, "act_fn", None)):
        return f"activation {type(getattr(module, 'act_fn', None)).__name__} is not SiLU"
    if E > MAX_EXPERTS:
        return f"E={E} must be at most {MAX_EXPERTS}"
    return None


# ---- GPT-OSS experts ----------------------------------------------------------------------------------------------------------------
def gpt_oss_rows(gate_up_proj):
    """transformers' GptOssExperts.gate_up_proj [E, H, 2I] (gate = columns 0::2, up = columns 1::2) -> the kernel's row order
    [E, 2I, H]: gate rows 0..I-1, then up rows I..2I-1."""
    w = gate_up_proj.transpose(1, 2)
    return torch.cat([w[:, 0::2], w[:, 1::2]], 1)


def gpt_oss_rows_inverse(rows):
    """[E, 2I, H] in the kernel's row order -> [E, H, 2I] interleaved (the inverse of gpt_oss_rows)."""
    E, N2, H = rows.shape
    return torch.stack([rows[:, :N2 // 2], rows[:, N2 // 2:]], 2).reshape(E, N2, H).transpose(1, 2)


def gpt_oss_bias_rows(bias):
    """gate_up_proj_bias [E, 2I] interleaved -> gate entries first, then up entries (the reordering of gpt_oss_rows)."""
    return torch.cat([bias[:, 0::2], bias[:, 1::2]], 1)


def gpt_oss_bias_rows_inverse(bias):
    E, N2 = bias.shape
    return torch.stack([bias[:, :N2 // 2], bias[:, N2 // 2:]], 2).reshape(E, N2)


def mxfp4_buffers(blocks, scales, Kp, interleaved=False):
    """MXFP4 checkpoint tensors (openai/gpt-oss-*: `*_blocks [E, R, K/32, 16]` uint8, two e2m1 codes a byte with the low nibble first,
    and `*_scales [E, R, K/32]` uint8 E8M0 with bias 127) -> (qweight [E, R, Kp/2], w_scale [E, R, Kp/32]) of the (w_dtype="fp4") cell
    WITHOUT re-quantising: the format is the same byte for byte.  Columns are padded to Kp with zero bytes and the scales with byte 0,
    which is what inc_mx_quant writes for an all-padding block.  interleaved: the rows R = 2I are gate_up's (gate = rows 0::2) and
    come out de-interleaved, gate rows first."""
    E, R, G, B = blocks.shape
    assert blocks.dtype == torch.uint8 and scales.dtype == torch.uint8 and B == 16 and tuple(scales.shape) == (E, R, G)
    assert Kp % 128 == 0 and Kp >= 32 * G
    q = torch.zeros((E, R, Kp // 2), dtype=torch.uint8, device=blocks.device)
    s = torch.zeros((E, R, Kp // 32), dtype=torch.uint8, device=blocks.device)
    q[:, :, :16 * G] = blocks.reshape(E, R, 16 * G)
    s[:, :, :G] = scales
    if interleaved:
        q, s = torch.cat([q[:, 0::2], q[:, 1::2]], 1), torch.cat([s[:, 0::2], s[:, 1::2]], 1)
    return q.contiguous(), s.contiguous()


class MXGptOssExperts(MXExperts):
    """transformers' GptOssExperts with MX weights and MX activations.  MXExperts' four buffers in the kernel's row order (gate rows
    first, then up rows: the module de-interleaves once, at conversion) plus gate_up_bias [E, 2I] (the same order) and down_bias
    [E, H], fp32.  forward is MXExperts' with inc_mx_moe_gemm_glu in place of inc_mx_moe_gemm: the biases in both products and the
    clamped SwiGLU (alpha, limit) instead of the SiLU product.  GptOssExperts.forward names its arguments (hidden_states,
    router_indices, routing_weights); they are FusedExperts.forward's three, in its order and under its contract (ids outside 0..E-1,
    the router's mask class E among them, contribute nothing on both routes)."""

    # MXExperts' value, kept.  Measured on the GPT-OSS shapes (scripts/mx_gpt_oss_time.py, profiles/mx/mx_gpt_oss_time.log): the fused
    # route is 8.7 - 41.7 x faster than the dense route at every measured point, up to 128 rows per expert (gpt-oss-20b, T = 1024),
    # which is as far as the script goes and hence what its rule prints; between 128 and 256 rows per expert it is not measured
    MOE_MAX_ROWS = 256

    def __init__(self, num_experts, hidden_dim, intermediate_dim, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", alpha=1.702, limit=7.0,
                 device="cuda", float_type=torch.float16):
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"MXGptOssExperts needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation.")
        super().__init__(num_experts, hidden_dim, intermediate_dim, w_dtype=w_dtype, act_dtype=act_dtype, device=device,
                         float_type=float_type)
        del self.act_fn  # the activation is the clamped SwiGLU of the kernel
        self.alpha, self.limit = float(alpha), float(limit)
        dev = self.gate_up_qweight.device
        self.register_buffer("gate_up_bias", torch.zeros((num_experts, 2 * intermediate_dim), dtype=torch.float32, device=dev))
        self.register_buffer("down_bias", torch.zeros((num_experts, hidden_dim), dtype=torch.float32, device=dev))

    @classmethod
    @torch.no_grad()
    def from_float(cls, module, w_dtype="fp8_e4m3", act_dtype="fp8_e4m3", device="cuda"):
        """One inc_mx_quant on the [E * N, K] view of each matrix in the kernel's row order; biases to fp32."""
        E, H, N2 = module.gate_up_proj.shape
        I = N2 // 2
        new = cls(E, H, I, w_dtype=w_dtype, act_dtype=act_dtype, alpha=module.alpha, limit=module.limit, device=device,
                  float_type=half_or_fp16(module.gate_up_proj.dtype))
        dev = new.gate_up_qweight.device
        new._quantize(gpt_oss_rows(module.gate_up_proj.detach().to(dev)), module.down_proj.detach().to(dev).transpose(1, 2))
        new.gate_up_bias.copy_(gpt_oss_bias_rows(module.gate_up_proj_bias.detach().to(dev).float()))
        new.down_bias.copy_(module.down_proj_bias.detach().to(dev).float())
        return new

    @classmethod
    @torch.no_grad()
    def from_mxfp4(cls, gate_up_blocks, gate_up_scales, gate_up_bias, down_blocks, down_scales, down_bias, act_dtype="fp8_e4m3",
                   alpha=1.702, limit=7.0, device="cuda", float_type=torch.bfloat16):
        """The loader for openai/gpt-oss-* checkpoint tensors: gate_up_proj_blocks [E, 2I, H/32, 16], gate_up_proj_scales
        [E, 2I, H/32], gate_up_proj_bias [E, 2I] (rows interleaved), down_proj_blocks [E, H, I/32, 16], down_proj_scales [E, H, I/32],
        down_proj_bias [E, H].  w_dtype = "fp4"; the codes and scale bytes are taken as they are (mxfp4_buffers)."""
        E, N2, GH, _ = gate_up_blocks.shape
        H, I = 32 * GH, N2 // 2
        assert tuple(down_blocks.shape[:2]) == (E, H) and down_blocks.shape[2] * 32 == I
        new = cls(E, H, I, w_dtype="fp4", act_dtype=act_dtype, alpha=alpha, limit=limit, device=device, float_type=float_type)
        dev = new.gate_up_qweight.device
        q, s = mxfp4_buffers(gate_up_blocks.to(dev), gate_up_scales.to(dev), new.kp_h, interleaved=True)
        new.gate_up_qweight.copy_(q)
        new.gate_up_w_scale.copy_(s)
        q, s = mxfp4_buffers(down_blocks.to(dev), down_scales.to(dev), new.kp_i)
        new.down_qweight.copy_(q)
        new.down_w_scale.copy_(s)
        new.gate_up_bias.copy_(gpt_oss_bias_rows(gate_up_bias.to(dev).float()))
        new.down_bias.copy_(down_bias.to(dev).float())
        return new

    def recover(self, dtype=None, expert=None):
        """Dequantised weights in the GPT-OSS layout, so that they drop into a float GptOssExperts: gate_up [E, H, 2I] interleaved and
        down [E, I, H], or expert `expert`'s [H, 2I], [I, H]."""
        gu, dn = super().recover(dtype, expert)
        if expert is not None:
            gu, dn = gu[None], dn[None]
        gu, dn = gpt_oss_rows_inverse(gu).contiguous(), dn.transpose(1, 2).contiguous()
        return (gu, dn) if expert is None else (gu[0], dn[0])

    def recover_biases(self, dtype=None):
        """(gate_up_proj_bias [E, 2I] interleaved, down_proj_bias [E, H]) in `dtype` or float_type."""
        dtype = self.float_type if dtype is None else dtype
        return gpt_oss_bias_rows_inverse(self.gate_up_bias).to(dtype), self.down_bias.to(dtype)

    def _fusable(self):
        # inc_moe_combine stores four columns at a time
        return self.num_experts <= MAX_EXPERTS and self.hidden_dim % 4 == 0

    def _fused_forward(self, x2d, idx, w, cdt):
        T, k = idx.shape
        E, af, wf = self.num_experts, self.act_fmt, self.w_fmt
        route = ops.moe_route(idx, E)
        xq, xs = ops.mx_quant(x2d, af, self.kp_h)
        h = ops.mx_moe_gemm_glu(0, xq, xs, af, route, self.gate_up_qweight, self.gate_up_w_scale, wf, T, k, bias=self.gate_up_bias,
                                alpha=self.alpha, limit=self.limit, out_dtype=cdt)
        hq, hs = ops.mx_quant(h, af, self.kp_i)
        y = ops.mx_moe_gemm_glu(1, hq, hs, af, route, self.down_qweight, self.down_w_scale, wf, T, k, bias=self.down_bias,
                                routing_weights=w)
        return ops.moe_combine(y, route, T, k, E, cdt)

    def _product(self, a, prefix, e, kp, cdt):
        aq, as_ = ops.mx_quant(a, self.act_fmt, kp)
        product = ops.mx_gemv if a.shape[0] <= ops.MX_GEMV_MAX_M else ops.mx_gemm
        return product(aq, as_, self.act_fmt, self._buffers[f"{prefix}_qweight"][e], self._buffers[f"{prefix}_w_scale"][e], self.w_fmt,
                       self._buffers[f"{prefix}_bias"][e].to(cdt), cdt)

    def _expert_mlp(self, rows, e, cdt):
        """GptOssExperts.forward's MLP with MXLinear's products (and their bias add) on expert e's slices, and _apply_gate's
        arithmetic in the compute dtype."""
        I = self.intermediate_dim
        y = self._product(rows, "gate_up", e, self.kp_h, cdt)
        gate, up = y[:, :I].clamp(min=None, max=self.limit), y[:, I:].clamp(min=-self.limit, max=self.limit)
        glu = gate * torch.sigmoid(gate * self.alpha)
        return self._product(((up + 1) * glu).contiguous(), "down", e, self.kp_i, cdt)

    def extra_repr(self):
        return super().extra_repr() + f", alpha={self.alpha}, limit={self.limit}"

