"""FP8 fused MoE experts for MI355X.

transformers (5.x) holds the experts of a Mixtral / Qwen2-MoE / Qwen3-MoE / OLMoE layer in one `*Experts` module with two 3-D
parameters, `gate_up_proj [E, 2I, H]` (gate rows 0..I-1, up rows I..2I-1) and `down_proj [E, H, I]`, and a
`forward(hidden_states, top_k_index, top_k_weights)` that loops over the experts that were hit.  `FP8Experts` replaces such a module
under `FP8Config(moe_experts=True)`: every expert's two matrices are quantised as `FP8Linear` quantises a weight (slice e of every
buffer is byte for byte what `inc_fp8_quant_rows` writes for expert e's matrix), and forward is six HIP launches with no host
synchronisation: route -> quantise x -> gate_up product with the SiLU product (`inc_fp8_moe_gemm` mode 0) -> quantise h -> down
product with the routing weight (mode 1) -> combine (include/inc_mi355x.h, K17e).  The forward contract and the
dense route's loop are FusedExperts' (fused_experts.py).
"""

import torch

from .... import ops
from ...utils.utility import half_or_fp16
from ..fused_experts import MAX_EXPERTS, FusedExperts, is_silu


class FP8Experts(FusedExperts):
    """Fused experts with e4m3 weights (one fp32 scale per output channel of every expert) and e4m3 activations (one fp32 scale per
    token, from the data of the call).  Buffers (Kp = K rounded up to 128): gate_up_qweight uint8 [E, 2I, Kp(H)], gate_up_w_scale fp32
    [E, 2I], down_qweight uint8 [E, H, Kp(I)], down_w_scale fp32 [E, H].  bf16 / fp16 compute in their own dtype, fp32 computes in
    float_type and is cast back (as FP8Linear.forward).  The dense route (the referee) runs FP8Linear's own kernels
    (inc_fp8_quant_rows, inc_fp8_gemv / inc_fp8_gemm) on the slices of every expert that was hit."""

    # the fused route serves up to this many routed rows per expert on average (T * top_k <= MOE_MAX_ROWS * E); larger batches take the
    # dense route.  Measured (scripts/fp8_moe_time.py, profiles/fp8/fp8_moe_time.log; the rule is the script's last line): Mixtral
    # (E 8, k 2) fused 1.09 x faster than dense at T = 1024 (256 rows per expert), dense 2.4 x faster at T = 4096 (1024); Qwen3-MoE
    # (E 128, k 8) fused 12.5 x faster at T = 4096 (256 per expert)
    MOE_MAX_ROWS = 256

    def __init__(self, num_experts, hidden_dim, intermediate_dim, act_fn=None, device="cuda", float_type=torch.float16):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"FP8Experts needs a HIP device ('cuda[:N]'), got '{device}'. There is no CPU implementation.")
        super().__init__(num_experts, hidden_dim, intermediate_dim, act_fn)
        E, H, I = num_experts, hidden_dim, intermediate_dim
        self.kp_h, self.kp_i = ops.mx_padded_k(H), ops.mx_padded_k(I)
        self.float_type = float_type
        for prefix, N, kp in (("gate_up", 2 * I, self.kp_h), ("down", H, self.kp_i)):
            self.register_buffer(f"{prefix}_qweight", torch.zeros((E, N, kp), dtype=torch.uint8, device=dev))
            self.register_buffer(f"{prefix}_w_scale", torch.zeros((E, N), dtype=torch.float32, device=dev))

    @classmethod
    @torch.no_grad()
    def from_float(cls, module, device="cuda"):
        """One inc_fp8_quant_rows on the [E * N, K] view of each parameter: the scale is per row, so this is each expert quantised on
        its own."""
        E, N2, H = module.gate_up_proj.shape
        I = N2 // 2
        new = cls(E, H, I, act_fn=module.act_fn, device=device, float_type=half_or_fp16(module.gate_up_proj.dtype))
        dev = new.gate_up_qweight.device
        for prefix, p, N, K, kp in (("gate_up", module.gate_up_proj, N2, H, new.kp_h), ("down", module.down_proj, H, I, new.kp_i)):
            codes, scale = ops.fp8_quant_rows(p.detach().to(dev).reshape(E * N, K), None, kp)
            new._buffers[f"{prefix}_qweight"].copy_(codes.view(E, N, kp))
            new._buffers[f"{prefix}_w_scale"].copy_(scale.view(E, N))
        return new

    def recover(self, dtype=None, expert=None):
        """Dequantised weights (gate_up [E, 2I, H], down [E, H, I]) in `dtype` or float_type, or expert `expert`'s two matrices
        [2I, H], [H, I]: the code table times the channel's scale, one fp32 multiply per element (FP8Linear.recover per slice)."""
        dtype = self.float_type if dtype is None else dtype
        sel = slice(None) if expert is None else slice(int(expert), int(expert) + 1)
        out = []
        for prefix, K in (("gate_up", self.hidden_dim), ("down", self.intermediate_dim)):
            q, s = self._buffers[f"{prefix}_qweight"][sel], self._buffers[f"{prefix}_w_scale"][sel]
            table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(q.device)
            w = (table[q.long()] * s[..., None])[..., :K].to(dtype)
            out.append(w if expert is None else w[0])
        return tuple(out)

    def _fusable(self):
        # inc_moe_combine stores four columns at a time
        return is_silu(self.act_fn) and self.num_experts <= MAX_EXPERTS and self.hidden_dim % 4 == 0

    def _compute_dtype(self, x):
        return x.dtype if x.dtype in (torch.float16, torch.bfloat16) else self.float_type

    def _fused_forward(self, x2d, idx, w, cdt):
        """Six launches in stream order; every buffer is allocated per call and nothing is kept.  Rows of h past the route's valid
        positions hold whatever torch.empty gave, non-finite values included: the quantiser's contract for such a row is that every
        write stays in bounds (include/inc_mi355x.h), and nothing reads those rows' codes or scales -- inc_fp8_moe_gemm reads neither
        the codes nor the a_scale entry of a row that no valid position names."""
        T, k = idx.shape
        E = self.num_experts
        route = ops.moe_route(idx, E)
        xq, xs = ops.fp8_quant_rows(x2d, None, self.kp_h)
        h = ops.fp8_moe_gemm(0, xq, xs, route, self.gate_up_qweight, self.gate_up_w_scale, T, k, out_dtype=cdt)
        hq, hs = ops.fp8_quant_rows(h, None, self.kp_i)
        y = ops.fp8_moe_gemm(1, hq, hs, route, self.down_qweight, self.down_w_scale, T, k, routing_weights=w)
        return ops.moe_combine(y, route, T, k, E, cdt)

    def _product(self, a, prefix, e, kp, cdt):
        aq, as_ = ops.fp8_quant_rows(a, None, kp)
        product = ops.fp8_gemv if a.shape[0] <= ops.FP8_GEMV_MAX_M else ops.fp8_gemm
        return product(aq, as_, self._buffers[f"{prefix}_qweight"][e], self._buffers[f"{prefix}_w_scale"][e], None, cdt)

    def _expert_mlp(self, rows, e, cdt):
        gate, up = self._product(rows, "gate_up", e, self.kp_h, cdt).chunk(2, dim=-1)
        return self._product((self.act_fn(gate) * up).contiguous(), "down", e, self.kp_i, cdt)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, "
                f"fp8_config=E4M3, act_granularity=per_token, w_granularity=per_channel")


def unsupported_reason(module, cfg):
    """Why FP8Quantizer leaves the fused-experts `module` in float under `cfg` (None = it converts it)."""
    E = module.gate_up_proj.shape[0]
    if not is_silu(getattr(module, "act_fn", None)):
        return f"activation {type(getattr(module, 'act_fn', None)).__name__} is not SiLU"
    if E > MAX_EXPERTS:
        return f"E={E} must be at most {MAX_EXPERTS}"
    return None
