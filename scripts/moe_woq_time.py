"""Time one MoE experts layer forward on the MI355X (device events, median of repeated calls), INT4 g128 asym RTN experts.

Routes, same inputs and routing (softmax top-k of random logits):
  bf16    transformers' own experts module with bf16 weights (eager forward: host loop over the experts that were hit)
  loop    the same loop over per-expert MI355XWeightOnlyLinear gate_up / down modules (the packed Linear kernels)
  dense   MI355XWeightOnlyExperts with MOE_FUSED = False (per-expert recover() + the eager loop)
  fused   MI355XWeightOnlyExperts' fused route (route -> gate_up -> down -> combine)
`bytes` is what the fused route must stream at least: the packed weights, scales and zero points of the experts that were hit, plus x,
the intermediate and the output; `hbm` is that over the fused time as a fraction of 8 TB/s.

    python scripts/moe_woq_time.py [--shapes mixtral,qwen3] [--ts 1,4,16,64,256,1024,4096]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"mixtral": (4096, 14336, 8, 2), "qwen3": (2048, 768, 128, 8)}  # H, I, E, k
PEAK = 8.0e12


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def _float_experts(H, I, E, k, dev):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)
    try:
        cfg._experts_implementation = "eager"
    except Exception:  # pragma: no cover
        pass
    with torch.device(dev):
        m = MixtralExperts(cfg).to(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        m.gate_up_proj.normal_(0.0, 0.02, generator=g)
        m.down_proj.normal_(0.0, 0.02, generator=g)
    return m


def _loop(lin_gu, lin_dn, x, idx, w, E):
    out = torch.zeros_like(x)
    mask = F.one_hot(idx, num_classes=E).permute(2, 1, 0)
    for e in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero():
        e = int(e[0])
        pos, tok = torch.where(mask[e])
        gate, up = lin_gu[e](x[tok]).chunk(2, dim=-1)
        h = lin_dn[e](F.silu(gate) * up) * w[tok, pos, None]
        out.index_add_(0, tok, h.to(out.dtype))
    return out


def main():
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts, quantize_experts
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--ts", default="1,4,16,64,256,1024,4096")
    ap.add_argument("--gs", type=int, default=128)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ts = [int(t) for t in args.ts.split(",")]
    for shape in args.shapes.split(","):
        H, I, E, k = SHAPES[shape]
        fm = _float_experts(H, I, E, k, dev)
        qm = quantize_experts(fm, dict(group_size=args.gs, scheme="asym"), dev)
        qm.MOE_MAX_ROWS = 1 << 30  # this script times the fused route at every T
        lin_gu, lin_dn = [], []
        for e in range(E):
            for prefix, N, K, dst in (("gate_up", 2 * I, H, lin_gu), ("down", H, I, lin_dn)):
                lin = MI355XWeightOnlyLinear(K, N, bits=4, group_size=args.gs, zp=True, device=dev)
                qw, sc, qz = qm._bufs(prefix)
                lin.qweight, lin.scales, lin.qzeros = qw[e], sc[e], qz[e]
                lin.bias = None
                dst.append(lin)
        per_expert = sum(t[0].numel() * t.element_size() for t in qm._bufs("gate_up") + qm._bufs("down"))
        print(f"== {shape}: H {H} I {I} E {E} k {k}, INT4 g{args.gs} asym, {per_expert / 1e6:.1f} MB packed per expert "
              f"(bf16 {2 * 3 * H * I / 1e6:.1f} MB)", flush=True)
        print(f"{'T':>5} {'active':>6} {'bytes MB':>9} {'bf16 us':>9} {'loop us':>9} {'dense us':>9} {'fused us':>9} {'hbm':>6}"
              f" {'vs bf16':>7} {'vs loop':>7} {'vs dense':>8}", flush=True)
        crossover = None
        for T in ts:
            g = torch.Generator(device=dev).manual_seed(T)
            x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
            wts, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=g, device=dev), -1), k, dim=-1)
            wts = (wts / wts.sum(-1, keepdim=True)).to(torch.bfloat16)
            active = int(torch.unique(idx).numel())
            nbytes = active * per_expert + T * H * 2 + T * k * (I * 2 + H * 4) + T * H * 2
            reps = 20 if T <= 256 else 5
            with torch.no_grad():
                t_bf16 = _time(lambda: fm(x, idx, wts), reps)
                t_loop = _time(lambda: _loop(lin_gu, lin_dn, x, idx, wts, E), reps)
                qm.MOE_FUSED = False
                t_dense = _time(lambda: qm(x, idx, wts), max(3, reps // 4))
                qm.MOE_FUSED = True
                t_fused = _time(lambda: qm(x, idx, wts), reps)
            if crossover is None and t_dense <= t_fused:
                crossover = T
            print(f"{T:>5} {active:>6} {nbytes / 1e6:>9.1f} {t_bf16:>9.1f} {t_loop:>9.1f} {t_dense:>9.1f} {t_fused:>9.1f} "
                  f"{nbytes / (t_fused * 1e-6) / PEAK:>6.3f} {t_bf16 / t_fused:>6.2f}x {t_loop / t_fused:>6.2f}x {t_dense / t_fused:>7.2f}x",
                  flush=True)
        print(f"{shape}: dense route first as fast as fused at T = {crossover} (T*k = {None if crossover is None else crossover * k}, "
              f"{None if crossover is None else crossover * k // E} rows per expert; MOE_MAX_ROWS = "
              f"{MI355XWeightOnlyExperts.MOE_MAX_ROWS} rows per expert)", flush=True)
        del fm, qm, lin_gu, lin_dn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
