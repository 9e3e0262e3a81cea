"""SHA-256 of the outputs of every decode form, one line per case: run it in two trees and diff the listings to see whether a change
of the kernels moved a bit.  The cases and their seeded inputs are the tests' own tables, run through the public `ops` calls in bf16 and
fp16:

  route       the STREAM_W4 / STREAM_W8 / GEMV16 / STRIP rows of tests/gemm_route_cases.py (ops.woq_gemm)
  group       tests/decode_group_cases.py: the plain batch, the gathered batch (ops.WoqGemmGroupCall) and the gated pair (ops.WoqGatedCall)
  act_order   tests/act_order_cases.py, random order (ops.WoqGemmCall with k_order)
  anyw        tests/anyw_decode_cases.py (ops.woq_gemv_anyw)
  anyw_perm   tests/anyw_group_cases.py: the gathered single launch (ops.WoqGemvAnywCall with k_order) ...
  anyw_group  ... and the batches without orders, with orders and mixed (ops.WoqGemvAnywGroupCall)
  lut, moe    one split-K case each of the NF4 forward (inc_woq_gemm_lut) and of the fused experts forward (inc_woq_moe_gemm)

Every case is called twice on the shared workspace; the two outputs must agree before the digest is printed.
usage: python scripts/decode_outputs_digest.py > listing.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_compressor_amd import _lib, ops  # noqa: E402
from tests import act_order_cases as P  # noqa: E402
from tests import anyw_decode_cases as A  # noqa: E402
from tests import anyw_group_cases as G  # noqa: E402
from tests import decode_group_cases as D  # noqa: E402
from tests import gemm_route_cases as R  # noqa: E402

dev = torch.device("cuda:0")
DTYPES = ((torch.bfloat16, "bf16"), (torch.float16, "fp16"))


def tensors(L):
    return tuple(torch.from_numpy(L[k]).to(dev) for k in ("qweight", "scales", "qzeros"))


def order(p):
    return None if p is None else torch.from_numpy(p).to(dev)


def emit(name, fn):
    """fn() -> a tensor or a list of tensors."""
    outs = [fn(), fn()]
    torch.cuda.synchronize()
    for o in outs:
        assert o is not None, f"{name}: the library declined the case"
    a, b = ([o] if torch.is_tensor(o) else list(o) for o in outs)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), f"{name}: a second call is not bit-identical"
    h = hashlib.sha256()
    for t in a:
        h.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
    print(f"{name} {h.hexdigest()}", flush=True)


def main():
    for dtype, dn in DTYPES:
        for c in R.CASES:
            if c.route in ("STREAM_W4", "STREAM_W8", "GEMV16", "STRIP"):
                qw, sc, qz = tensors(R.make_layer(c.N, c.K, c.group_size, c.bits))
                x, bias = R.make_x(c.M, c.K, dtype).to(dev), R.make_bias(c.N, dtype).to(dev)
                emit(f"route {c.name} {dn}", lambda: ops.woq_gemm(x, qw, sc, qz, bias, c.N, c.K, c.group_size, c.bits))
        for c, M in D.PARAMS:
            x = R.make_x(M, c.K, dtype).to(dev)
            parts = [(*tensors(L), R.make_bias(L["N"], dtype).to(dev), L["N"]) for L in D.layers(c)]
            call = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype)
            emit(f"group plain {c.name}_m{M} {dn}", lambda call=call: call(x))
            for mixed in (False, True):
                ps = [order(p) for p in D.orders(c, mixed)]
                call = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=ps)
                emit(f"group gathered{' mixed' if mixed else ''} {c.name}_m{M} {dn}", lambda call=call: call(x))
        for c, M in D.GATED_PARAMS:
            x = R.make_x(M, c.K, dtype).to(dev)
            gp, up = [(*tensors(L), None, L["N"]) for L in D.layers(c, D.gated_ns(c))]
            for what, ps in (("", None), (" gathered", [order(p) for p in D.orders(c, n=2)])):
                call = ops.WoqGatedCall(gp, up, c.K, c.group_size, 4, dtype, k_orders=ps)
                emit(f"group gated{what} {c.name}_m{M} {dn}", lambda call=call: call(x))
        for c, M in P.PARAMS:
            qw, sc, qz = tensors(P.layer(c))
            x, bias = R.make_x(M, c.K, dtype).to(dev), R.make_bias(c.N, dtype).to(dev)
            call = ops.WoqGemmCall(qw, sc, qz, bias, c.N, c.K, c.group_size, c.bits, dtype, k_order=order(P.perm(c.K, "random")))
            emit(f"act_order {c.name}_m{M} {dn}", lambda call=call: call(x))
        for c in A.CASES:
            qw, sc, qz = tensors(A.layer_of(c))
            x, bias = R.make_x(c.M, c.K, dtype).to(dev), R.make_bias(c.N, dtype).to(dev)
            emit(f"anyw {c.name} {dn}", lambda: ops.woq_gemv_anyw(x, qw, sc, qz, bias, c.N, c.K, c.group_size, c.bits))
        for c in G.PERM_CASES:
            L = A.layer_of(c)
            x, bias = R.make_x(c.M, c.K, dtype).to(dev), R.make_bias(c.N, dtype).to(dev)
            call = ops.WoqGemvAnywCall(*tensors(L), bias, c.N, c.K, L["group_size"], c.bits, dtype, k_order=order(P.perm(c.K, "random")))
            assert call.gathers(c.M)
            emit(f"anyw_perm {c.name} {dn}", lambda call=call: call(x, checked=False))
        for c in G.GROUP_CASES:
            x = R.make_x(c.M, c.K, dtype).to(dev)
            biases = [None if b is None else b.to(dev) for b in G.group_biases(c, dtype)]
            parts = [(*tensors(L), b, L["N"]) for L, b in zip(G.group_layers(c), biases)]
            for mode in G.ORDER_MODES:
                od = None if mode == "plain" else [order(p) for p in G.group_orders(c, mode)]
                call = ops.WoqGemvAnywGroupCall(parts, c.K, c.group_size, c.bits, dtype, k_orders=od)
                emit(f"anyw_group {mode} {c.name} {dn}", lambda call=call: call(x))
        lut_and_moe(dtype, dn)


def lut_and_moe(dtype, dn):
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    lib = _lib.lib
    gen = torch.Generator(device=dev).manual_seed(11)
    M, N, K = 5, 200, 2048
    m = MI355XWeightOnlyLinear(K, N, dtype="nf4", bits=4, group_size=32, scale_dtype=torch.float32, use_optimum_format=False, device=dev)
    m.pack(torch.randint(-8, 8, (N, K), generator=gen, device=dev, dtype=torch.int32),
           torch.rand(N, K // 32, generator=gen, device=dev) * 0.02 + 1e-3, None, None)
    x = R.make_x(M, K, dtype).to(dev)
    assert m._forward_plan() == "fused_lut" and lib.inc_woq_gemm_lut_workspace_bytes(M, N, K) > 0, "the LUT case does not split K"
    emit(f"lut nf4_g32_{N}x{K}_m{M} {dn}", lambda: m(x))

    E, H, I, T, k = 4, 256, 512, 5, 2
    q = MI355XWeightOnlyExperts(E, H, I, bits=4, group_size=128, device=dev)
    packs = []
    for n_out, k_in in ((2 * I, H), (H, I)):
        packs += [torch.randint(0, 16, (E, n_out, k_in), generator=gen, device=dev, dtype=torch.int32),
                  torch.rand(E, n_out, k_in // 128, generator=gen, device=dev) * 0.002 + 0.0005,
                  torch.randint(0, 16, (E, n_out, k_in // 128), generator=gen, device=dev, dtype=torch.int32)]
    q.pack(*packs)
    w, idx = torch.topk(torch.softmax(torch.randn(T, E, generator=gen, device=dev), dim=-1), k, dim=-1)
    w = (w / w.sum(-1, keepdim=True)).to(dtype)
    xm = R.make_x(T, H, dtype).to(dev)
    assert lib.inc_woq_moe_gemm_workspace_bytes(0, T, k, E, 2 * I, H) > 0 and lib.inc_woq_moe_gemm_workspace_bytes(1, T, k, E, H, I) > 0, \
        "the MoE case does not split K"
    emit(f"moe e{E}_h{H}_i{I}_t{T} {dn}", lambda: q(xm, idx, w))


if __name__ == "__main__":
    with torch.no_grad():
        main()
