"""Weight-only INT4 fused MoE experts for MI355X.

transformers (5.x) holds the experts of a Mixtral / Qwen2-MoE / Qwen3-MoE / OLMoE layer in one `*Experts` module with two 3-D
parameters, `gate_up_proj [E, 2I, H]` (gate rows 0..I-1, up rows I..2I-1) and `down_proj [E, H, I]`, and a
`forward(hidden_states, top_k_index, top_k_weights)` that loops over the experts that were hit.  `MI355XWeightOnlyExperts` replaces
such a module after RTN: every expert's two matrices are packed in the optimum layout of `MI355XWeightOnlyLinear`, stacked on a
leading expert axis (slice e of every buffer is byte for byte what `MI355XWeightOnlyLinear.pack` writes for expert e), and forward is
four HIP launches with no host synchronisation (ops.WoqMoeCall: route -> gate_up GEMM with the SiLU product -> down GEMM with the
routing weight -> combine; include/inc_mi355x.h, K4e).  The forward contract and the dense route's loop are FusedExperts'
(fused_experts.py).
"""

import math

import torch

from .... import ops
from ....common.utils import logger
from ..fused_experts import MAX_EXPERTS, FusedExperts, is_silu
from .modules import _hip_device

_PARTS = ("qweight", "scales", "qzeros")


class MI355XWeightOnlyExperts(FusedExperts):
    """Packed INT4 experts (optimum layout per expert, stacked on the expert axis) with a fused HIP forward.

    Buffers: gate_up_qweight [E, H/8, 2I] int32, gate_up_scales [E, G_H, 2I] fp16, gate_up_qzeros [E, G_H, 2I/8] int32,
    down_qweight [E, I/8, H], down_scales [E, G_I, H], down_qzeros [E, G_I, H/8]; G_H = H / group_size, G_I = I / group_size
    (one group per row for group_size = -1).  bf16 / fp16 compute in their own dtype; any other dtype computes in fp16 and is cast
    back (warned once per module).  The dense route (the referee, and the escape hatch) recover()s the two matrices of every expert
    that was hit and runs transformers' eager MLP on them."""

    # the fused route serves up to this many routed rows per expert on average (T * top_k <= MOE_MAX_ROWS * E); larger batches take the
    # dense route.  Measured (profiles/r8/moe_woq_time.log): Mixtral (E 8, k 2) fused 1.49 x faster than dense at T = 1024 (256 rows per
    # expert), dense 1.39 x faster at T = 4096 (1024 per expert); Qwen3-MoE (E 128, k 8) fused 16.9 x faster at T = 4096 (256 per expert)
    MOE_MAX_ROWS = 256

    def __init__(self, num_experts, hidden_dim, intermediate_dim, bits=4, group_size=32, act_fn=None, dtype="int", device="cuda"):
        if bits != 4 or dtype != "int":
            raise NotImplementedError(f"packed experts are INT4 (dtype='int', bits=4), got dtype={dtype!r} bits={bits}")
        dev = _hip_device(device)
        super().__init__(num_experts, hidden_dim, intermediate_dim, act_fn)
        E, H, I = num_experts, hidden_dim, intermediate_dim
        self.bits, self.dtype, self.group_size = bits, dtype, group_size
        for prefix, N, K in (("gate_up", 2 * I, H), ("down", H, I)):
            G = math.ceil(K / self._gs(K))
            self.register_buffer(f"{prefix}_qweight", torch.zeros((E, math.ceil(K / 8), N), dtype=torch.int32, device=dev))
            self.register_buffer(f"{prefix}_scales", torch.zeros((E, G, N), dtype=torch.float16, device=dev))
            self.register_buffer(f"{prefix}_qzeros", torch.zeros((E, G, math.ceil(N / 8)), dtype=torch.int32, device=dev))

    def _gs(self, K):
        return K if (self.group_size == -1 or self.group_size >= K) else self.group_size

    def _bufs(self, prefix):
        return tuple(self._buffers[f"{prefix}_{p}"] for p in _PARTS)

    def pack(self, gate_up_int, gate_up_scale, gate_up_zp, down_int, down_scale, down_zp):
        """Integer weights [E, N, K] (signed for sym: zp None; codes 0..15 with zp [E, N, G] for asym), scales [E, N, G] fp32 -> the
        stacked optimum layout, one `inc_woq_pack` per expert and matrix (the kernel MI355XWeightOnlyLinear.pack runs)."""
        self.__dict__["_call"] = None
        for prefix, iw, sc, zp in (("gate_up", gate_up_int, gate_up_scale, gate_up_zp), ("down", down_int, down_scale, down_zp)):
            qw, scales, qz = self._bufs(prefix)
            dev = qw.device
            iw, sc = iw.to(dev), sc.to(dev)
            zp = None if zp is None else zp.to(dev)
            shift = 2 ** (self.bits - 1) if zp is None else 0
            for e in range(self.num_experts):
                ops.woq_pack(iw[e].contiguous(), sc[e], None if zp is None else zp[e], self.bits, shift, qweight=qw[e], qzeros=qz[e],
                             scales_out=scales[e])

    def pack_codes(self, prefix, expert, codes, scales, zp):
        """GPTQ's entry (mirrors MI355XWeightOnlyLinear.pack_codes): the already-offset codes 0..15 (uint8 [N, K], what the column loop
        emits) of matrix `prefix` ("gate_up" / "down") of one expert, scales [N, G] fp32, zp [N, G] or None (sym) -> that expert's
        slices, bit-identical to `pack` on `codes - 8` (sym) / `codes` with zp (asym)."""
        self.__dict__["_call"] = None
        qw, sc, qz = self._bufs(prefix)
        ops.woq_pack(codes, scales, zp, self.bits, 0, qweight=qw[expert], qzeros=qz[expert], scales_out=sc[expert])

    def recover(self, dtype=None, expert=None):
        """Dense weights (gate_up [E, 2I, H], down [E, H, I]) of `dtype` (default fp16), or expert `expert`'s two matrices [2I, H], [H, I]:
        inc_woq_dequant on every slice, so each equals MI355XWeightOnlyLinear.recover() of that expert's matrix."""
        dtype = dtype or torch.float16
        experts = range(self.num_experts) if expert is None else [int(expert)]
        out = []
        for prefix, N, K in (("gate_up", 2 * self.intermediate_dim, self.hidden_dim), ("down", self.hidden_dim, self.intermediate_dim)):
            qw, sc, qz = self._bufs(prefix)
            mats = [ops.woq_dequant(qw[e], sc[e], qz[e], None, N, K, self._gs(K), self.bits, out_dtype=dtype) for e in experts]
            out.append(mats[0] if expert is not None else torch.stack(mats))
        return tuple(out)

    def _fusable(self):
        H, I, gs = self.hidden_dim, self.intermediate_dim, self.group_size
        groups_ok = gs == -1 or (gs >= 32 and gs & (gs - 1) == 0 and H % gs == 0 and I % gs == 0)
        return is_silu(self.act_fn) and H % 32 == 0 and I % 32 == 0 and self.num_experts <= MAX_EXPERTS and groups_ok

    def _compute_dtype(self, x):
        cdt = x.dtype if x.dtype in (torch.bfloat16, torch.float16) else torch.float16
        if cdt is not x.dtype and not self.__dict__.get("_warned_dtype"):
            self.__dict__["_warned_dtype"] = True
            logger.warning("MI355XWeightOnlyExperts: %s activations are computed in fp16 (the packed kernels take bf16 / fp16)", x.dtype)
        return cdt

    def _fused_forward(self, x2d, idx, w, cdt):
        call = self.__dict__.get("_call")
        gu, dn = self._bufs("gate_up"), self._bufs("down")
        if call is None or not call.current(gu, dn):
            call = self.__dict__["_call"] = ops.WoqMoeCall(gu, dn, self.num_experts, self.hidden_dim, self.intermediate_dim, self.group_size)
        xin = x2d if x2d.dtype is cdt else x2d.to(cdt)
        xin = xin.contiguous()
        if xin.data_ptr() % 16:
            xin = xin.clone()  # the kernels read x in 16-byte pieces; a fresh allocation is aligned
        return call(xin, idx, w)

    def _dense_forward(self, x2d, idx, w, cdt):
        return super()._dense_forward(x2d.to(cdt), idx, w, cdt)  # F.linear takes the weights' dtype: one cast, before the loop

    def _expert_mlp(self, rows, e, cdt):
        """transformers' MixtralExperts MLP on expert e's recovered weights."""
        gu, dn = self.recover(cdt, expert=e)
        gate, up = torch.nn.functional.linear(rows, gu).chunk(2, dim=-1)
        return torch.nn.functional.linear(self.act_fn(gate) * up, dn)

    def extra_repr(self):
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, intermediate_dim={self.intermediate_dim}, "
                f"bits={self.bits}, group_size={self.group_size}")


def unsupported_reason(module, cfg):
    """Why RTN leaves the fused-experts `module` in float under `cfg` (None = it packs it)."""
    E, N2, H = module.gate_up_proj.shape
    I = N2 // 2
    gs = cfg.get("group_size", 32)
    if cfg.get("dtype", "int") != "int" or cfg.get("bits", 4) != 4:
        return f"dtype={cfg.get('dtype')!r} bits={cfg.get('bits')}: packed experts are INT4"
    if cfg.get("use_mse_search", False):
        return "use_mse_search is not implemented for experts"
    if cfg.get("use_double_quant", False):
        return "double quantisation is not implemented for experts"
    if cfg.get("group_dim", 1) != 1:
        return "group_dim must be 1"
    if not is_silu(getattr(module, "act_fn", None)):
        return f"activation {type(getattr(module, 'act_fn', None)).__name__} is not SiLU"
    if gs not in (32, 64, 128, 256, -1) or (gs != -1 and (H % gs or I % gs)):
        return f"group_size={gs} must be one of 32 / 64 / 128 / 256 / -1 and divide H={H} and I={I}"
    if H % 32 or I % 32 or E > MAX_EXPERTS:
        return f"H={H} and I={I} must be multiples of 32 and E={E} at most {MAX_EXPERTS}"
    return None


def quantize_experts(module, cfg, device):
    """RTN of a fused-experts module -> MI355XWeightOnlyExperts.  quant_tensor runs on the [E*N, K] view of each parameter: RTN groups run
    along K inside a row, so this is each expert quantised on its own."""
    from .utility import quant_tensor

    E, N2, H = module.gate_up_proj.shape
    I = N2 // 2
    gs = cfg.get("group_size", 32)
    kw = dict(dtype="int", bits=4, group_size=gs, scheme=cfg.get("scheme", "sym"), quantile=cfg.get("quantile", 1.0), return_int=True,
              full_range=cfg.get("use_full_range", False))
    packed = []
    for p, N, K in ((module.gate_up_proj, 2 * I, H), (module.down_proj, H, I)):
        w = p.detach().to(device).reshape(E * N, K).contiguous()
        iw, sc, zp = quant_tensor(w, **kw)
        packed += [iw.reshape(E, N, K), sc.reshape(E, N, -1), None if zp is None else zp.reshape(E, N, -1)]
    new = MI355XWeightOnlyExperts(E, H, I, bits=4, group_size=gs, act_fn=module.act_fn, device=device)
    new.pack(*packed)
    logger.debug("RTN experts: E=%d H=%d I=%d group_size=%s scheme=%s", E, H, I, gs, kw["scheme"])
    return new
