"""Shared by tests/test_anyw_groups_cpu.py and tests/test_gpu_anyw_groups.py (a helper module, not a conftest): the cases of the gathered
and the batched decode GEMV of the 1 / 2 / 3 / 5 / 6 / 7-bit modules (inc_woq_gemv_anyw_perm, inc_woq_gemv_anyw_multi).

inc_woq_gemv_anyw_perm computes y = x[:, k_order] . W_sorted^T + bias: a case's layer (gemm_route_cases.make_layer, contiguous groups)
plays the K-sorted weight, so the reference is gemm_route_cases.reference(x[:, perm], ...) on the oracle's dense weight and the bound
is that module's, unchanged:

    |y - ref| <= u_out * |ref| + 2 * (K + 4) * 2^-24 * S + tiny

The perm cases are rows of tests/anyw_decode_cases.py (the layout edges they hold are named there); the orders are those of
tests/act_order_cases.py.  A group case is (bits, K, group size, the members' N, M); member i's layer is make_layer(N[i], ...), its
order a permutation seeded by (K, i).
"""

import collections

import numpy as np
import torch

from tests import act_order_cases as P
from tests import anyw_decode_cases as A
from tests import gemm_route_cases as R

COUNTER_BYTES = 16384
DTYPES = A.DTYPES
DTYPE_IDS = ["bf16", "fp16"]
PERM_KINDS = P.PERM_KINDS

PERM_CASE_NAMES = ("b3_g32_straddle", "b3_long_m16", "b2_long", "b5_long", "b6_tail4", "b7_long", "b1_long")
PERM_CASES = [next(c for c in A.CASES if c.name == n) for n in PERM_CASE_NAMES]

GroupCase = collections.namedtuple("GroupCase", "name bits K group_size Ns M")
GROUP_CASES = [
    GroupCase("b3_one_slice", 3, 96, 32, (64, 68, 204), 5),        # the ragged strip of member 1 sits in the middle of the grid
    GroupCase("b3_four_slices", 3, 2080, 128, (264, 64), 16),
    GroupCase("b2_long", 2, 2080, 128, (200, 64, 68), 1),
    GroupCase("b5_long", 5, 1056, 64, (204, 64), 4),
]
GROUP_IDS = [c.name for c in GROUP_CASES]
ORDER_MODES = ("plain", "orders", "mixed")  # no orders; one random order per member; member 0 the identity, the others random


def slices(K, bits):
    return -(-K // A.SLICE_K[bits])


def multi_workspace_bytes(M, Ns, K, bits):
    s = slices(K, bits)
    return 0 if s <= 1 else COUNTER_BYTES + s * M * sum(Ns) * 4


# ---------------------------------------------------------------------------------------------------------------------------------------
# the gathered single launch
# ---------------------------------------------------------------------------------------------------------------------------------------
_perm_refs = {}


def perm_reference(c, dtype, kind):
    """(x, bias, p, ref, S): x [M, K] and bias as the kernel gets them, p = perm(K, kind) int32 numpy, ref and S in float64 for x[:, p].
    Cached: the tests share it and must not write to it."""
    key = (c.name, dtype, kind)
    if key not in _perm_refs:
        x, bias, p = R.make_x(c.M, c.K, dtype), R.make_bias(c.N, dtype), P.perm(c.K, kind)
        ref, S = R.reference(x[:, torch.from_numpy(p).long()], R.dense_weight64(A.layer_of(c), dtype), bias)
        _perm_refs[key] = (x, bias, p, ref, S)
    return _perm_refs[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------------------------------------------------
def group_layers(c):
    return [R.make_layer(N, c.K, c.group_size, c.bits) for N in c.Ns]


def member_order(K, i):
    return np.random.default_rng(977 + 31 * i + K).permutation(K).astype(np.int32)


def group_orders(c, mode):
    """One int32 [K] numpy order or None per member."""
    if mode == "plain":
        return [None] * len(c.Ns)
    if mode == "orders":
        return [member_order(c.K, i) for i in range(len(c.Ns))]
    assert mode == "mixed"
    return [None] + [member_order(c.K, i) for i in range(1, len(c.Ns))]


def group_biases(c, dtype):
    """A bias on the even members, none on the odd ones."""
    return [R.make_bias(N, dtype) + 0.25 * i if i % 2 == 0 else None for i, N in enumerate(c.Ns)]


_group_refs = {}


def group_reference(c, dtype, mode):
    """(x, biases, orders, [(ref, S) per member]).  Cached: shared, not to be written to."""
    key = (c.name, dtype, mode)
    if key not in _group_refs:
        x, biases, orders = R.make_x(c.M, c.K, dtype), group_biases(c, dtype), group_orders(c, mode)
        outs = []
        for L, b, p, N in zip(group_layers(c), biases, orders, c.Ns):
            xg = x if p is None else x[:, torch.from_numpy(p).long()]
            outs.append(R.reference(xg, R.dense_weight64(L, dtype), torch.zeros(N, dtype=dtype) if b is None else b))
        _group_refs[key] = (x, biases, orders, outs)
    return _group_refs[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# sort_packed_k
# ---------------------------------------------------------------------------------------------------------------------------------------
def fields_of(qweight, bits):
    """[rows * n_pack, N] uint32 numpy: every field of the packed words, padding included, in k order."""
    npk, mask = 32 // bits, (1 << bits) - 1
    q = np.asarray(qweight).astype(np.uint32)
    sh = (np.arange(npk, dtype=np.uint32) * bits)[None, :, None]
    return ((q[:, None, :] >> sh) & np.uint32(mask)).reshape(q.shape[0] * npk, q.shape[1])
