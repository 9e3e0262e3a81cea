"""Shared by tests/test_anyw_decode_cpu.py and tests/test_gpu_anyw_decode.py (a helper module, not a conftest): the cases of the decode
GEMV of the 1 / 2 / 3 / 5 / 6 / 7-bit modules (inc_woq_gemv_anyw, csrc/gemm_anyw.hip).

The layers, activations, biases, the float64 reference and the element-wise bound are those of tests/gemm_route_cases.py, unchanged:

    |y - ref| <= u_out * |ref| + 2 * (K + 4) * 2^-24 * S + tiny

A case names the edges of the layout it holds (`Pins`): padding fields in the last word, words that straddle a group boundary, column
quads (the four adjacent columns one lane owns) that straddle a qzeros word, a partly filled last qzeros word, the columns of the last
64-column strip, a ragged last group, and whether the launch splits K.  `pins_of` recomputes them from the layer, so a changed table
cannot silently lose an edge.  A retune of the split plan (SLICE_K) moves a `*_long` shape; it never drops the case.
"""

import collections

import numpy as np
import torch

from tests.gemm_route_cases import assert_elementwise, dense_weight64, make_bias, make_layer, make_x, reference  # noqa: F401

BITS = (1, 2, 3, 5, 6, 7)
MAX_M = 16
# k of one K-slice (one workgroup) per width: AnywShape<BITS>::SLICE_K of csrc/gemm_anyw.hip
SLICE_K = {1: 1024, 2: 1024, 3: 640, 5: 768, 6: 640, 7: 512}

Case = collections.namedtuple("Case", "name bits M N K group_size pins")
Pins = collections.namedtuple("Pins", "padding straddle_words straddle_quads partial_zword strip_tail ragged_group splits")


def _c(name, bits, M, N, K, gs, padding=0, straddle_words=0, straddle_quads=0, partial_zword=False, strip_tail=0, ragged_group=False,
       splits=False):
    return Case(name, bits, M, N, K, gs, Pins(padding, straddle_words, straddle_quads, partial_zword, strip_tail, ragged_group, splits))


CASES = [
    _c("b3_min", 3, 1, 64, 32, -1, padding=8, straddle_quads=3, partial_zword=True),
    _c("b3_g32_straddle", 3, 5, 68, 96, 32, padding=4, straddle_words=2, straddle_quads=3, partial_zword=True, strip_tail=4),
    _c("b3_g64_ragged_group", 3, 16, 204, 160, 64, straddle_words=2, straddle_quads=10, partial_zword=True, strip_tail=12, ragged_group=True),
    _c("b3_long", 3, 4, 64, 2080, 128, straddle_words=13, straddle_quads=3, partial_zword=True, ragged_group=True, splits=True),
    _c("b3_long_m16", 3, 16, 264, 2080, 128, straddle_words=13, straddle_quads=13, partial_zword=True, strip_tail=8, ragged_group=True,
       splits=True),
    _c("b2_g32", 2, 5, 68, 96, 32, partial_zword=True, strip_tail=4),
    _c("b2_long", 2, 16, 200, 2080, 128, partial_zword=True, strip_tail=8, ragged_group=True, splits=True),
    _c("b5_tail4", 5, 4, 68, 64, 32, padding=2, straddle_words=1, straddle_quads=6, partial_zword=True, strip_tail=4),
    _c("b5_long", 5, 16, 204, 1056, 64, straddle_words=11, straddle_quads=17, strip_tail=12, ragged_group=True, splits=True),
    _c("b6_tail4", 6, 1, 64, 64, 32, padding=1, straddle_words=1, straddle_quads=9, partial_zword=True),
    _c("b6_long", 6, 5, 204, 1056, 128, padding=4, straddle_words=7, straddle_quads=30, partial_zword=True, strip_tail=12, ragged_group=True,
       splits=True),
    _c("b7_exact", 7, 16, 68, 64, 32, strip_tail=4),
    _c("b7_long", 7, 4, 68, 1056, 64, strip_tail=4, ragged_group=True, splits=True),
    _c("b1_word", 1, 5, 64, 64, 32),
    _c("b1_long", 1, 16, 132, 1056, 128, partial_zword=True, strip_tail=4, ragged_group=True, splits=True),
]
CASE_IDS = [c.name for c in CASES]
DTYPES = (torch.bfloat16, torch.float16)


def layer_of(c):
    return make_layer(c.N, c.K, c.group_size if c.group_size > 0 else c.K, c.bits)


def group_size_eff(c):
    return c.K if (c.group_size == -1 or c.group_size >= c.K) else c.group_size


def slices_of(c):
    return -(-c.K // SLICE_K[c.bits])


def pins_of(c):
    """The edges of case c, recomputed from its layer's arrays."""
    L = layer_of(c)
    npk, gs = 32 // c.bits, group_size_eff(c)
    words = L["qweight"].shape[0]
    first = np.arange(words) * npk
    last = np.minimum(first + npk - 1, c.K - 1)
    quads = np.arange(c.N // 4) * 4
    return Pins(
        padding=words * npk - c.K,
        straddle_words=int(((first // gs) != (last // gs)).sum()),
        straddle_quads=int(((quads // npk) != ((quads + 3) // npk)).sum()),
        partial_zword=L["qzeros"].shape[1] * npk != c.N,
        strip_tail=c.N % 64,
        ragged_group=c.K % gs != 0,
        splits=slices_of(c) >= 2,
    )


def has_zero_zp(c):
    """The layer holds zp = 0 entries: stored as the all-ones field, which decodes by wrapping."""
    L = layer_of(c)
    npk, mask = 32 // c.bits, (1 << c.bits) - 1
    n = np.arange(c.N)
    fields = (L["qzeros"].astype(np.uint32)[:, n // npk] >> (c.bits * (n % npk)).astype(np.uint32)) & np.uint32(mask)
    return bool((L["zp"] == 0).any()) and bool((fields[(L["zp"] == 0).T] == mask).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the contract in fp32 torch, from the packed words alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def emulated_weight(c, dtype):
    """[N, K] of `dtype`: rn(int8(q - z) * scale), fields and zero points decoded from the packed arrays by the layout rules."""
    L = layer_of(c)
    bits, npk, mask, gs = c.bits, 32 // c.bits, (1 << c.bits) - 1, group_size_eff(c)
    k, n = np.arange(c.K), np.arange(c.N)
    q = (L["qweight"].astype(np.uint32)[k // npk, :] >> (bits * (k % npk)).astype(np.uint32)[:, None]) & np.uint32(mask)      # [K, N]
    z = ((L["qzeros"].astype(np.uint32)[:, n // npk] >> (bits * (n % npk)).astype(np.uint32)[None, :]) & np.uint32(mask)) + 1  # [G, N]
    z = np.where(z > mask, 0, z)
    g = k // gs
    diff = (q.astype(np.int32) - z.astype(np.int32)[g, :]).astype(np.int8)
    s = torch.from_numpy(L["scales"].astype(np.float16)).float()[torch.from_numpy(g)]                                          # [K, N]
    w = torch.from_numpy(diff.astype(np.float32)) * s   # exact in fp32: 8-bit integer x 11-bit significand
    return w.t().contiguous().to(dtype)


def emulate(c, x, bias, dtype):
    """fp32 accumulation of exact products, K-slices summed in slice order, + bias, one rounding."""
    w = emulated_weight(c, dtype).float()
    acc = torch.zeros(x.shape[0], c.N, dtype=torch.float32)
    sk = SLICE_K[c.bits]
    for k0 in range(0, c.K, sk):
        acc = acc + x[:, k0:k0 + sk].float() @ w[:, k0:k0 + sk].t()
    if bias is not None:
        acc = acc + bias.float()
    return acc.to(dtype)


def one_hot_ks(c):
    """Columns of x worth a one-hot row: the ends, the two sides of a group boundary and of a word boundary, the first k of the last word."""
    npk, gs = 32 // c.bits, group_size_eff(c)
    ks = [0, c.K - 1, npk - 1, npk, npk * ((c.K - 1) // npk)]
    if gs < c.K:
        ks += [gs - 1, gs]
    return sorted(set(ks))


def one_hot(c, dtype):
    ks = one_hot_ks(c)
    x = torch.zeros(len(ks), c.K, dtype=dtype)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    return x, ks
