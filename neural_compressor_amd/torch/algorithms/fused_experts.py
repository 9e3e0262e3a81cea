"""The frame of the fused MoE experts modules (MI355XWeightOnlyExperts, FP8Experts, MXExperts, MXGptOssExperts).

transformers (5.x) calls an experts module as `forward(hidden_states, top_k_index, top_k_weights)`.  `FusedExperts` holds the one copy
of that contract -- shapes, the empty batch, the choice between the fused and the dense route, the types the kernels take for the ids
and the routing weights, the cast back -- and the one copy of the dense route's loop over the experts that were hit.  A format is a
subclass with its buffers, its conversion and four hooks:

  _compute_dtype(x)                    bf16 / fp16 the products run in for activations of x.dtype
  _fusable()                           whether the module's shapes and activation fit the fused kernels
  _fused_forward(x2d, idx, w, cdt)     the HIP launches, no host wait; idx [T, k] int64 / int32, w [T, k] fp32 / bf16 / fp16, contiguous
  _expert_mlp(rows, e, cdt)            one expert's MLP on the gathered rows [n, H] -> [n, H]: the dense route's two products

The frame never asks which subclass it serves.
"""

import torch

MAX_EXPERTS = 512  # of inc_moe_route and the routed GEMMs (inc_woq_moe_gemm, inc_mx_moe_gemm, inc_fp8_moe_gemm)


def is_silu(act_fn):
    return isinstance(act_fn, torch.nn.SiLU) or type(act_fn).__name__ in ("SiLU", "SiLUActivation")


class FusedExperts(torch.nn.Module):
    # True: the fused route (_fused_forward).  False: the dense route -- per expert that was hit (host waits), gather its rows and run
    # _expert_mlp on them: the referee, and the escape hatch.  Every concrete class sets MOE_MAX_ROWS beside its measurement: the fused
    # route serves up to that many routed rows per expert on average (T * top_k <= MOE_MAX_ROWS * E), larger batches take the dense route
    MOE_FUSED = True

    def __init__(self, num_experts, hidden_dim, intermediate_dim, act_fn=None):
        super().__init__()
        self.num_experts, self.hidden_dim, self.intermediate_dim = num_experts, hidden_dim, intermediate_dim
        self.act_fn = act_fn if act_fn is not None else torch.nn.SiLU()

    def forward(self, hidden_states, top_k_index, top_k_weights):
        """transformers' experts signature: hidden_states [T, H], top_k_index / top_k_weights [T, k] -> [T, H] of hidden_states' dtype
        (computed in _compute_dtype and cast back).  Expert ids outside 0..E-1 (a "no expert" sentinel such as -1) contribute nothing,
        on both routes.  An empty batch or k = 0 is zeros."""
        x = hidden_states
        x2d = x.reshape(-1, self.hidden_dim)
        T = x2d.shape[0]
        if T == 0 or top_k_index.numel() == 0:
            return torch.zeros_like(x)
        cdt = self._compute_dtype(x)
        idx = top_k_index.reshape(T, -1)
        k = idx.shape[1]
        w = top_k_weights.reshape(T, k)
        if self.MOE_FUSED and T * k <= self.MOE_MAX_ROWS * self.num_experts and self._fusable():
            if idx.dtype not in (torch.int64, torch.int32):
                idx = idx.long()
            if w.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                w = w.float()
            y = self._fused_forward(x2d, idx.contiguous(), w.contiguous(), cdt)
        else:
            y = self._dense_forward(x2d, idx, w, cdt)
        return y.to(x.dtype).reshape(x.shape)

    def _dense_forward(self, x2d, idx, w, cdt):
        """transformers' MixtralExperts.forward with _expert_mlp on every expert that was hit (host waits: nonzero / where)."""
        out = torch.zeros((x2d.shape[0], self.hidden_dim), dtype=cdt, device=x2d.device)
        E = self.num_experts
        with torch.no_grad():
            # ids outside 0..E-1 go to an extra class E that is never visited: they contribute nothing, as on the fused route
            ids = torch.where((idx >= 0) & (idx < E), idx, torch.full_like(idx, E)).long()
            mask = torch.nn.functional.one_hot(ids, num_classes=E + 1)[..., :E].permute(2, 1, 0)
            hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
        for e in hit:
            e = int(e[0])
            top_k_pos, token_idx = torch.where(mask[e])
            y = self._expert_mlp(x2d[token_idx], e, cdt)
            y = y * w[token_idx, top_k_pos, None]
            out.index_add_(0, token_idx, y.to(cdt))
        return out

    def _compute_dtype(self, x):
        raise NotImplementedError

    def _fusable(self):
        raise NotImplementedError

    def _fused_forward(self, x2d, idx, w, cdt):
        raise NotImplementedError

    def _expert_mlp(self, rows, e, cdt):
        raise NotImplementedError
