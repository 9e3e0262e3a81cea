"""GPTQ for fused MoE experts: Hessians from routed rows, the per-expert solve, the packed module.

`GPTQConfig(quant_experts=True)` puts the `is_fused_experts` modules of a model into the GPTQ weight config; `RAWGPTQuantizer.
quantize_block` hands each block to `quantize_block_experts` below before its Linear flow runs:

  * calibration: one forward of the block over every calibration batch (float weights everywhere, the reference's non-sequential
    scheme: every layer of a block is calibrated on the float block) with the experts' forward replaced by `ExpertsCalibration.
    forward` -- ops.moe_route, per hit expert `g, u = x_e Wgu_e^T`, `h = act(g) * u`, `y = h Wd_e^T` as torch GEMMs on the float
    weights, and both Hessians of ALL experts folded by inc_gptq_hessian_accum_routed (gather mode on x, sorted mode on h);
  * solve: per expert and matrix the Linear path unchanged -- inc_gptq_hessian_finalize, HessianAccumulator.inverse_factor,
    GPTQ.fasterquant on gate_up_proj[e] [2I, H] (gate and up stacked on N) and down_proj[e] [H, I] -- and
    MI355XWeightOnlyExperts.pack_codes on the emitted codes;
  * an expert that received no routed row has H = 0 (the reference would zero its whole weight): it is quantised with RTN
    (quantize_experts' arithmetic on that slice) and named in one warning per module.

The Linears of the block do not depend on its experts (attention and the router sit in front of them), so their solve is the same
with the experts float or packed; the block's second (propagating) forward runs the packed experts like every packed Linear.
"""

import torch

from .... import ops
from ....common.utils import logger
from ...utils.utility import is_fused_experts, set_module
from ..fused_experts import is_silu
from .experts import MI355XWeightOnlyExperts

# False: fold the Hessians with one inc_gptq_hessian_accum per hit expert on host-sliced ranges (the only way before K5e; what the
# calibration forward also does when the library declines a shape).  A module attribute for A/B runs and tests.
ROUTED_LAUNCH = True
# The routed launch serves forwards whose mean rows per hit expert x K^2 stay at or below this; larger per-expert problems take the loop.
# Measured (profiles/r9/moe_gptq_time.log): the routed kernel's 128 x 128 tile runs at 0.09-0.20 of the bf16 MFMA peak at every shape,
# the dense kernel's 256 x 256 LDS-DMA tile at 0.33-0.83 once one expert fills the chip -- Mixtral-8x7B (E 8): loop 2.6-4.5 x faster at
# 4096 / 16384 rows per expert (rows x K^2 >= 2^36); Qwen3-30B-A3B (E 128): routed 1.3-14.6 x faster at 1024 / 4096 rows per expert
# (rows x K^2 <= 2^34), where the loop is 128 launches that each leave most CUs idle.  2^35 sits between the two regimes.
ROUTED_MAX_WORK = 1 << 35


def gptq_unsupported_reason(module, cfg):
    """Why GPTQ leaves the fused-experts `module` in float under the per-layer dict `cfg` (None = it packs it).  The packed module is
    INT4 in contiguous groups with no g_idx, so everything that reorders columns or changes the code format is out."""
    E, N2, H = module.gate_up_proj.shape
    I = N2 // 2
    gs = cfg.get("group_size", 32)
    if cfg.get("dtype", "int") != "int" or cfg.get("bits", 4) != 4:
        return f"dtype={cfg.get('dtype')!r} bits={cfg.get('bits')}: packed experts are INT4"
    for key, what in (("act_order", "act_order"), ("static_groups", "static_groups"), ("hybrid_order", "hybrid_order"),
                      ("mse", "use_mse_search"), ("use_double_quant", "double quantisation"), ("fp8_aware", "fp8_aware")):
        if cfg.get(key, False):
            return f"{what} is not implemented for experts"
    if not is_silu(getattr(module, "act_fn", None)):
        return f"activation {type(getattr(module, 'act_fn', None)).__name__} is not SiLU"
    if gs not in (32, 64, 128, 256, -1) or (gs != -1 and (H % gs or I % gs)):
        return f"group_size={gs} must be one of 32 / 64 / 128 / 256 / -1 and divide H={H} and I={I}"
    if H % 32 or I % 32 or E > 512:
        return f"H={H} and I={I} must be multiples of 32 and E={E} at most 512"
    return None


def _distributed_reason(quantizer):
    if (getattr(quantizer, "dist_ctx", None) is not None or getattr(quantizer, "hessian_allreduce", None)
            or getattr(quantizer, "independent_blocks", None) or getattr(quantizer, "layer_ctx", None) is not None):
        return "multi-GPU calibration of experts is not implemented"
    return None


class ExpertsCalibration:
    """The Hessians of one fused-experts module: H_gate_up [E, H, H], H_down [E, I, I] fp32 and the rows folded per expert.
    `forward` stands in for the module's forward during the capture pass; `solve` returns the packed module."""

    def __init__(self, module, cfg, device):
        self.module, self.cfg, self.device = module, dict(cfg), torch.device(device)
        E, N2, H = module.gate_up_proj.shape
        self.E, self.H, self.I = E, H, N2 // 2
        self.H_gate_up = torch.zeros((E, H, H), dtype=torch.float32, device=self.device)
        self.H_down = torch.zeros((E, self.I, self.I), dtype=torch.float32, device=self.device)
        self.rows_gate_up = torch.zeros(E, dtype=torch.int64, device=self.device)
        self.rows_down = torch.zeros(E, dtype=torch.int64, device=self.device)
        self.rowless = []  # experts quantised with RTN by solve()

    # -- capture ---------------------------------------------------------------------------------------------------------
    def _fold(self, Hs, rows, a, route, T, k, sorted_rows, offs, sorted_a):
        """Both forms compute H_e <- H_e c/(c+c_new) + 2/(c+c_new) X_e^T X_e; `sorted_a()` gives the rows in sorted order."""
        hit = sum(1 for e in range(self.E) if offs[e + 1] > offs[e])
        small = hit > 0 and (offs[self.E] / hit) * a.shape[1] * a.shape[1] <= ROUTED_MAX_WORK
        if ROUTED_LAUNCH and small and a.dtype in (torch.float32, torch.float16, torch.bfloat16):
            if a.data_ptr() % 16:
                a = a.clone()
            if ops.gptq_hessian_accum_routed(Hs, rows, a, route, T, k, sorted_rows=sorted_rows):
                return
        xs = sorted_a()
        done = rows.cpu().tolist()
        add = [0] * self.E
        for e in range(self.E):
            c_new = offs[e + 1] - offs[e]
            if c_new <= 0:
                continue
            tot = done[e] + c_new
            ops.gptq_hessian_accum(Hs[e], xs[offs[e]:offs[e + 1]], done[e] / tot, 2.0 / tot)
            add[e] = c_new
        rows += torch.tensor(add, dtype=torch.int64, device=rows.device)

    @torch.no_grad()
    def forward(self, hidden_states, top_k_index, top_k_weights):
        """transformers' experts forward on the float weights (same routing weights; the per-token sum runs in fp32 in sorted-slot
        order) that also folds this forward's rows into both Hessians."""
        m, E = self.module, self.E
        x2d = hidden_states.reshape(-1, self.H).contiguous()
        T = x2d.shape[0]
        idx = top_k_index.reshape(T, -1)
        k = idx.shape[1]
        if T == 0 or k == 0:
            return torch.zeros_like(hidden_states)
        if idx.dtype not in (torch.int64, torch.int32):
            idx = idx.long()
        S = T * k
        route = ops.moe_route(idx.contiguous(), E)
        offs = route[1:E + 2].cpu().tolist()  # the torch GEMMs below are per expert: their ranges are needed on the host anyway
        n = offs[E]
        order = route[E + 2:E + 2 + n].long()
        tok = torch.div(order, k, rounding_mode="floor")
        xs = x2d[tok]  # [n, H] in sorted order
        self._fold(self.H_gate_up, self.rows_gate_up, x2d, route, T, k, False, offs, lambda: xs)
        h = torch.zeros((S, self.I), dtype=x2d.dtype, device=x2d.device)  # rows past offsets[E] belong to no expert
        y = torch.zeros((n, self.H), dtype=torch.float32, device=x2d.device)
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi <= lo:
                continue
            g, u = torch.nn.functional.linear(xs[lo:hi], m.gate_up_proj[e].to(x2d.dtype)).chunk(2, dim=-1)
            h[lo:hi] = m.act_fn(g) * u
            y[lo:hi] = torch.nn.functional.linear(h[lo:hi], m.down_proj[e].to(x2d.dtype)).float()
        self._fold(self.H_down, self.rows_down, h, route, T, k, True, offs, lambda: h)
        w = top_k_weights.reshape(-1)[order].float()
        out = torch.zeros((T, self.H), dtype=torch.float32, device=x2d.device)
        out.index_add_(0, tok, y * w[:, None])
        return out.to(hidden_states.dtype).reshape(hidden_states.shape)

    # -- solve -----------------------------------------------------------------------------------------------------------
    def _rtn_slice(self, w, new, prefix, e):
        """quantize_experts' arithmetic for one expert's matrix (RTN is row-wise: the slice alone gives the same codes)."""
        from .utility import quant_tensor

        iw, sc, zp = quant_tensor(w.detach().to(self.device).contiguous(), dtype="int", bits=4, group_size=self.cfg.get("group_size", 32),
                                  scheme="sym" if self.cfg.get("sym", False) else "asym", quantile=1.0, return_int=True, full_range=False)
        qw, scales, qz = new._bufs(prefix)
        ops.woq_pack(iw.contiguous(), sc, zp, new.bits, 2 ** (new.bits - 1) if zp is None else 0, qweight=qw[e], qzeros=qz[e],
                     scales_out=scales[e])

    @torch.no_grad()
    def solve(self, name="experts", timings=None):
        """Per expert and matrix: finalize -> inverse factor -> column loop (GPTQ.fasterquant) -> pack_codes.  Consumes the Hessians."""
        from .gptq import GPTQ, HessianAccumulator

        cfg, m, dev = self.cfg, self.module, self.device
        gs = cfg.get("group_size", 32)
        new = MI355XWeightOnlyExperts(self.E, self.H, self.I, bits=4, group_size=gs, act_fn=m.act_fn, device=dev)
        sym = bool(cfg.get("sym", False))
        accs = []
        self.rowless = []
        for prefix, W3, Hs, rows in (("gate_up", m.gate_up_proj, self.H_gate_up, self.rows_gate_up),
                                     ("down", m.down_proj, self.H_down, self.rows_down)):
            done = rows.cpu().tolist()
            for e in range(self.E):
                W = W3[e].detach().to(dev)
                if done[e] == 0:
                    if e not in self.rowless:
                        self.rowless.append(e)
                    self._rtn_slice(W, new, prefix, e)
                    continue
                acc = HessianAccumulator(W.shape[1], dev)
                acc.H, acc._n = Hs[e], 1  # the running mean is complete; GPTQ does not depend on a positive factor of H
                sv = GPTQ(None, W=W, device=dev, accumulator=acc)
                sv.defer_check = True
                sv.configure(cfg)
                scale, _, zp, _ = sv.fasterquant(W, blocksize=cfg.get("block_size", 128), percdamp=cfg.get("percdamp", 0.01), groupsize=gs)
                new.pack_codes(prefix, e, sv.codes, scale, None if sym else zp)
                accs.append(acc)
                sv.free()
        for acc in accs:
            acc.check()  # the deferred "not positive definite" checks
        self.H_gate_up = self.H_down = None
        if self.rowless:
            logger.warning("GPTQ: experts %s of %s received no calibration row; they are quantised with RTN", sorted(self.rowless), name)
        return new


def quantize_block_experts(quantizer, block, block_idx):
    """The fused-experts modules of `block` that have a GPTQ config entry: calibrate on the float block, solve, pack, replace.
    Unsupported settings and multi-GPU runs leave a module float with one warning; modules without an entry (the default,
    `quant_experts=False`) are not looked at."""
    todo = []
    for name, module in block.named_modules():
        if not is_fused_experts(module):
            continue
        full = quantizer.get_full_layer_name(name, block_idx)
        cfg = quantizer.weight_config.get(full)
        if cfg is None:
            continue
        reason = gptq_unsupported_reason(module, cfg) or _distributed_reason(quantizer)
        if reason is not None:
            logger.warning("GPTQ: %s stays in floating point (%s)", full, reason)
            continue
        todo.append((name, full, module, ExpertsCalibration(module, cfg, quantizer.device)))
    if not todo:
        return
    # the grouping of the calibration batches (and its probe forwards of the block) is settled before the Hessians listen
    batch_num = quantizer.cache_key_arguments.pop("batch_num")
    try:
        quantizer._forward_groups(batch_num, "hidden_states" in quantizer.cache_key_arguments, block)
    finally:
        quantizer.cache_key_arguments["batch_num"] = batch_num
    for _, _, module, cal in todo:
        module.forward = cal.forward
    try:
        quantizer._run_block(block, capture=True)
    finally:
        for _, _, module, _ in todo:
            del module.forward  # back to the class's forward
    for name, full, module, cal in todo:
        set_module(block, name, cal.solve(full))
