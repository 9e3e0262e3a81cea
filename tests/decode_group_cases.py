"""Shared by tests/test_decode_groups_cpu.py and tests/test_gpu_decode_groups.py (a helper module, not a conftest).

Two one-launch decode forms on the streaming GEMV (neural_compressor_amd/csrc/gemm_stream.hip):
  A  inc_woq_gemm_multi_perm   y_i = x[:, k_order_i] . W_i^T + b_i for the members of a group, every member through its own order;
  B  inc_woq_gemm_gated        h = silu(x . Wg^T) * (x . Wu^T), one rounding (form (i) of the issue: the strips of gate and up share a
                               ticket, the last arriver forms the product from the two fixed-order fp32 sums).

CASES are the smallest shapes at which each rung of the launch ladder can go wrong; `plan` is what the batched launch must use there
(K-slices, row blocks, steps per wave).  The batched plan is inc_woq_gemm's streaming plan for the members' strips together, so a case
is pinned through inc_woq_gemm_route on the N-concatenated layer (at 5 rows where M <= 4: a single call of so few rows may take the
no-split kernel, the batched launch never does, and up to 16 rows the plan does not depend on M) and through the workspace size.  A
retune that moves a case off its rung has to move the shape: never drop the case.

Layers follow gemm_route_cases.make_layer's pattern (asymmetric; scale / zero point walk through 41 / 2^bits values along n and g) with
a member-dependent shift and seed, so that members of equal shape differ clearly: exchanging gate and up, or two members, is visible.

Bounds: part A gemm_route_cases.tolerance; part B moe_stage_cases.mode0_tolerance with dg, du = accum_bound(K, |x| . |W|).  Neither
is taken from a kernel's output.
"""

import collections

import numpy as np
import torch

from tests import gemm_route_cases as R
from tests import moe_stage_cases as MS

O = R.O

Plan = collections.namedtuple("Plan", "route splitk steps")
Case = collections.namedtuple("Case", "name Ns K group_size bits Ms plan pins")

CASES = [
    Case("ragged", (200, 264), 416, 32, 4, (1, 5, 16, 17, 33, 64), Plan("STREAM_W4", 1, 4),
         "13 K-steps (clamped steps read k_order), ragged last strip, per-step groups, 1 / 2 / 4 row blocks"),
    Case("slices", (264, 64, 328), 1024, 128, 4, (1, 16, 33), Plan("STREAM_W4", 2, 4), "splitk 2, one group per 4 steps, three members"),
    Case("one_group", (200, 200), 2048, 2048, 4, (5,), Plan("STREAM_W4", 4, 4), "g_shift = -1, 4 slices"),
    Case("eight_steps", (64, 64), 33280, 128, 4, (5,), Plan("STREAM_W4", 33, 8), "the 8-step rung, whose gather keeps eight index pairs in flight"),
    Case("int8", (200, 264), 512, 128, 8, (1, 16), Plan("STREAM_W8", 1, 4), "the 8-bit form (part A only)"),
]
PARAMS = [(c, M) for c in CASES for M in c.Ms]
PARAM_IDS = [f"{c.name}_m{M}" for c, M in PARAMS]

GATED_MAX_M = 16   # rows inc_woq_gemm_gated serves (include/inc_mi355x.h)
GATED_CASES = [c for c in CASES if c.bits == 4]
GATED_PARAMS = [(c, M) for c in GATED_CASES for M in c.Ms if M <= GATED_MAX_M]
GATED_PARAM_IDS = [f"{c.name}_m{M}" for c, M in GATED_PARAMS]
GATED_OVER_M = 17  # one M above the limit: declined, nothing launched

DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "fp16"]
COUNTER_BYTES = 16384
STREAM_SLICE_K = 512  # k of one K-slice at 4 steps per wave


def case(name):
    return next(c for c in CASES if c.name == name)


def row_blocks(M):
    return 4 if M > 32 else 2 if M > 16 else 1


def gated_ns(c):
    """Part B: two equal members with the first member's N."""
    return (c.Ns[0], c.Ns[0])


def assert_on_rung(c, M, dtype, Ns=None):
    """The batched launch of case c at M rows still sits on the rung the case was written for (host only: inc_woq_gemm_route on the
    N-concatenated layer, the multi workspace size for the K-slices at 4 steps per wave)."""
    import ctypes

    from neural_compressor_amd import _lib, ops

    Ns = c.Ns if Ns is None else Ns
    got = ops.woq_gemm_route(max(M, 5), sum(Ns), c.K, c.group_size, c.bits, dtype)
    want = dict(route=c.plan.route, splitk=c.plan.splitk, row_blocks=row_blocks(M), steps=c.plan.steps)
    assert {k: got[k] for k in want} == want, f"{c.name} M = {M}: the case no longer reaches the rung it was written for: {got}"
    narr = (ctypes.c_int64 * len(Ns))(*Ns)
    ws = _lib.lib.inc_woq_gemm_multi_workspace_bytes(len(Ns), M, narr, c.K)
    assert ws == COUNTER_BYTES + -(-c.K // STREAM_SLICE_K) * M * sum(Ns) * 4
    assert c.plan.splitk == -(-c.K // (STREAM_SLICE_K * c.plan.steps // 4))
    return ws


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
_layers = {}


def make_layer(N, K, group_size, bits, member):
    """gemm_route_cases.make_layer's pattern for member `member` of a group (numpy, optimum layout): scale and zero point of (column n,
    group g) shifted by 11 / 7 per member, codes from a member-dependent seed.  Cached: the tests share it and must not write to it."""
    key = (N, K, group_size, bits, member)
    if key in _layers:
        return _layers[key]
    rng = np.random.default_rng(1000003 * N + 1009 * K + 17 * group_size + bits + 7919 * (member + 1))
    G = 1 if group_size >= K else -(-K // group_size)
    n, g = np.arange(N)[:, None], np.arange(G)[None, :]
    scales = (0.004 * (1.0 + 0.05 * ((7 * n + 3 * g + 11 * member) % 41))).astype(np.float32)
    levels = 1 << bits
    if bits == 8:  # keep q - zp inside int8
        zp = 96 + (5 * n + 3 * g + 7 * member) % 64
        kgroup = np.minimum(np.arange(K) // group_size, G - 1)
        iw = np.clip(zp[:, kgroup] + rng.integers(-100, 101, size=(N, K)), 0, 255)
    else:
        zp = (5 * n + 3 * g + 7 * member) % levels
        iw = rng.integers(0, levels, size=(N, K))
    qweight, qzeros, scales_gn = O.woq_pack_optimum(iw, scales, zp, bits)
    layer = dict(N=N, K=K, G=G, group_size=group_size, bits=bits, qweight=qweight, qzeros=qzeros, scales=scales_gn, g_idx=None, member=member)
    _layers[key] = layer
    return layer


def layers(c, Ns=None):
    return [make_layer(N, c.K, c.group_size, c.bits, i) for i, N in enumerate(c.Ns if Ns is None else Ns)]


_dense = {}


def dense64(layer, dtype):
    """The oracle's dense weight of a member (compute dtype = x dtype) in float64, cached."""
    key = (layer["N"], layer["K"], layer["group_size"], layer["bits"], layer["member"], dtype)
    if key not in _dense:
        _dense[key] = O.woq_dense_weight(layer["qweight"], layer["scales"], layer["qzeros"], layer["N"], layer["K"], layer["bits"],
                                         layer["group_size"], compute_dtype=dtype).double()
    return _dense[key]


def order(K, member):
    """A random order of member `member`, int32 [K] numpy; the members' orders differ."""
    return np.random.default_rng(4241 + K + 101 * member).permutation(K).astype(np.int32)


def orders(c, mixed=False, n=None):
    """One order per member; `mixed`: the LAST member has none (a plain member in an act_order group)."""
    n = len(c.Ns) if n is None else n
    out = [order(c.K, i) for i in range(n)]
    if mixed:
        out[-1] = None
    return out


def gathered(x, p):
    return x if p is None else x[:, torch.from_numpy(p).long()]


# ---------------------------------------------------------------------------------------------------------------------------------------
# references (computed once per key, shared, never written to)
# ---------------------------------------------------------------------------------------------------------------------------------------
_refs = {}


def group_reference(c, M, dtype, mixed=False, with_bias=True):
    """Part A: x [M, K], the members' biases, and per member (ref, S) in float64 of x[:, p_i] @ W_i^T + b_i."""
    key = ("A", c.name, M, dtype, mixed, with_bias)
    if key not in _refs:
        x = R.make_x(M, c.K, dtype)
        ps = orders(c, mixed)
        biases = [R.make_bias(N, dtype) if with_bias else torch.zeros(N, dtype=dtype) for N in c.Ns]
        outs = [R.reference(gathered(x, p), dense64(L, dtype), b) for L, p, b in zip(layers(c), ps, biases)]
        _refs[key] = (x, biases, outs)
    return _refs[key]


def gated_reference(c, M, dtype, ps=(None, None)):
    """Part B: (x, ref, tol) with ref = silu(g) u in float64, g = x[:, ps[0]] . Wg, u = x[:, ps[1]] . Wu, and mode0_tolerance's bound."""
    key = ("B", c.name, M, dtype, tuple(None if p is None else p.tobytes() for p in ps))
    if key not in _refs:
        x = R.make_x(M, c.K, dtype)
        ref, tol = gated_oracle(c, x, dtype, ps)
        _refs[key] = (x, ref, tol)
    return _refs[key]


def gated_oracle(c, x, dtype, ps=(None, None), swap=False, act=True):
    """(ref, tol) of the gated pair of case c on x.  `swap`: gate and up exchanged; `act` False: the SiLU dropped (the mutants of the
    comparator's self-test)."""
    Lg, Lu = layers(c, gated_ns(c))
    if swap:
        Lg, Lu = Lu, Lg
    xg, xu = gathered(x, ps[0]).double(), gathered(x, ps[1]).double()
    wg, wu = dense64(Lg, dtype), dense64(Lu, dtype)
    g, u = xg @ wg.t(), xu @ wu.t()
    dg, du = MS.accum_bound(c.K, xg.abs() @ wg.abs().t()), MS.accum_bound(c.K, xu.abs() @ wu.abs().t())
    ref, tol = MS.mode0_tolerance(g, u, dg, du, dtype)
    if not act:
        ref = g * u
    return ref, tol
