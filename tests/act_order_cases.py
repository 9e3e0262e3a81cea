"""Shared by tests/test_act_order_decode_cpu.py and tests/test_gpu_act_order_decode.py (a helper module, not a conftest).

inc_woq_gemm_perm computes y = x[:, k_order] . W_sorted^T + bias on the three streaming decode routes.  The cases are the shapes
of tests/gemm_route_cases.py at which those kernels branch; a case's layer (gemm_route_cases.make_layer, contiguous groups) plays
the K-sorted weight, so the reference of a case is gemm_route_cases.reference(x[:, perm], ...) and the bound is that module's.
"""

import collections

import numpy as np
import torch

from tests import gemm_route_cases as R

PermCase = collections.namedtuple("PermCase", "name Ms N K group_size bits")

LADDER = (5, 16, 17, 32, 33, 64)
CASES = [
    PermCase("gemv16_g32", (1, 4), 1000, 416, 32, 4),
    PermCase("gemv16_one_group", (1, 4), 200, 2048, 2048, 4),
    PermCase("one_group_m5", (5,), 200, 2048, 2048, 4),             # STREAM_W4, 4 K-slices
    PermCase("stream4_g32", LADDER, 200, 416, 32, 4),               # 13 K-steps: the clamped steps past the end read k_order; ragged N
    PermCase("stream4_g128", LADDER, 264, 1024, 128, 4),            # 2 K-slices
    PermCase("stream4_8step", (5,), 64, 33280, 128, 4),             # the 8-step body
    PermCase("stream8_g128", LADDER, 200, 512, 128, 8),
    PermCase("stream8_g32", (5, 33), 200, 512, 32, 8),
]
PARAMS = [(c, M) for c in CASES for M in c.Ms]
PARAM_IDS = [f"{c.name}_m{M}" for c, M in PARAMS]
PERM_KINDS = ("random", "reversal", "identity")
PERM_ROUTES = ("GEMV16", "STREAM_W4", "STREAM_W8")


def route_case(c, M):
    """The row of gemm_route_cases.CASES for this shape: the kernel and variant the case must reach."""
    rows = [r for r in R.CASES if (r.M, r.N, r.K, r.group_size, r.bits) == (M, c.N, c.K, c.group_size, c.bits)
            and not r.g_idx and r.x_align == 16 and r.y_align == 16]
    assert len(rows) == 1, f"{c.name} M = {M}: no unique row in the route table"
    assert rows[0].route in PERM_ROUTES
    return rows[0]


def layer(c):
    return R.make_layer(c.N, c.K, c.group_size, c.bits)


def perm(K, kind):
    """int32 [K] numpy."""
    if kind == "identity":
        return np.arange(K, dtype=np.int32)
    if kind == "reversal":
        return np.arange(K - 1, -1, -1, dtype=np.int32)
    assert kind == "random"
    return np.random.default_rng(4241 + K).permutation(K).astype(np.int32)


def swapped(p, x_row):
    """p with two entries exchanged: the one that selects the largest |x| of x_row and its right neighbour."""
    q = p.copy()
    j = int(np.nonzero(p == int(torch.argmax(x_row.float().abs())))[0][0])
    k = (j + 1) % len(p)
    q[j], q[k] = p[k], p[j]
    return q


_refs = {}


def reference(c, M, dtype, kind):
    """(x, bias, ref, S): x [M, K] and bias as the kernel gets them (CPU, `dtype`); ref, S in float64 for x[:, perm(kind)].
    Cached: the tests share it and must not write to it."""
    key = (c.name, M, dtype, kind)
    if key not in _refs:
        x, bias = R.make_x(M, c.K, dtype), R.make_bias(c.N, dtype)
        ref, S = R.reference(x[:, torch.from_numpy(perm(c.K, kind)).long()], R.dense_weight64(layer(c), dtype), bias)
        _refs[key] = (x, bias, ref, S)
    return _refs[key]


def exact_result(c, x, p, bias, dtype):
    """What a kernel that gathers x through p returns, up to its rounding: float64, rounded once to `dtype`."""
    return R.reference(x[:, torch.from_numpy(p).long()], R.dense_weight64(layer(c), dtype), bias)[0].to(dtype)
