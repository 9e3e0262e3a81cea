"""Shared by tests/test_gemm_routes_cpu.py and tests/test_gpu_gemm_routes.py (a helper module, not a conftest).

  * CASES: the route table of the fused weight-only GEMM.  (shape, dtype-independent, alignment) -> the kernel family
    `inc_woq_gemm_route` must report and its variant (K-slices, row blocks, steps, store / load form).  A retuned threshold in
    neural_compressor_amd/csrc/gemm.hip (woq_gemm_plan; the kernels it chooses among are csrc/gemm_*.hip) moves a case off the kernel it was written for: the table is where that
    has to be acknowledged -- move the shape so that the route keeps a case, never drop the route.
  * the inputs of a case (asymmetric weights whose scales and zero points differ clearly between neighbouring columns and
    groups, a bias that is distinct per column, activations with a few large entries) and its float64 reference;
  * the element-wise comparator and its bound.

Bound, per output element (issue "Pin every route of the fused weight-only GEMM to an element-wise oracle"):

    |y - ref| <= u_out * |ref| + 2 * (K + 4) * 2^-24 * S + tiny,   S = sum_k |x_k| |w_k| + |bias|   (float64)

u_out = 2^-8 (bf16) / 2^-11 (fp16): one rounding to the output type.  Products of two 16-bit values are exact in fp32 and any
order of K fp32 additions errs by at most K * 2^-24 * S; the factor 2 and the + 4 cover the slab re-sum, the bias add and the
double rounding.  tiny = the smallest fp16 subnormal (0 for bf16).  The bound follows from the arithmetic, not from a measurement.
"""

import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import woq_oracle as O  # noqa: E402

# INC_WOQ_ROUTE_* of include/inc_mi355x.h
ROUTES = {
    "TILE_ANYW": 1, "STRIP8": 2, "STRIP": 3, "3A2B_W8": 4, "D2R": 5, "3A2B_W4": 6, "BIG": 7, "TILE": 8, "GEMV16": 9,
    "STREAM_W4": 10, "STREAM_W8": 11, "SMALL": 12,
}
INC_ERR_WORKSPACE = -4
# without a workspace these fall back to one pass; STREAM_* and SMALL return INC_ERR_WORKSPACE
ONE_PASS_FALLBACK = ("STRIP", "D2R", "3A2B_W4", "3A2B_W8")

# y_align / x_align: the largest power of two (bytes) the address is a multiple of, as the case requires (16, 8 or 2 / 16 or 2).
# splitk: with a workspace of inc_woq_gemm_workspace_bytes.  y_vec_ok / x_vec_ok: -1 where the route has no such form.
Case = collections.namedtuple(
    "Case", "name M N K group_size bits y_align x_align g_idx route splitk row_blocks steps y_vec_ok x_vec_ok")


def _c(name, M, N, K, gs, route, splitk=1, row_blocks=0, steps=0, y_vec_ok=-1, x_vec_ok=-1, bits=4, y_align=16, x_align=16, g_idx=False):
    return Case(name, M, N, K, gs, bits, y_align, x_align, g_idx, route, splitk, row_blocks, steps, y_vec_ok, x_vec_ok)


def _ladder(prefix, N, K, gs, route, splitk, bits=4):
    """M = 5 .. 64 on one layer: 1 / 2 / 4 row blocks of the streaming kernel, 4 steps per wave."""
    return [_c(f"{prefix}_m{M}", M, N, K, gs, route, splitk=splitk, row_blocks=mb, steps=4, bits=bits)
            for M, mb in ((5, 1), (16, 1), (17, 2), (32, 2), (33, 4), (64, 4))]


CASES = [
    # ---- direct-to-register kernel, one pass: ragged last N tile (2 columns) / last M tile (1 row), the three store forms
    _c("d2r_yvec0_ragged_n", 300, 258, 256, 64, "D2R", steps=4, y_vec_ok=0),
    _c("d2r_yvec1_ragged_m", 1025, 68, 256, 64, "D2R", steps=4, y_vec_ok=1),
    _c("d2r_yvec3", 1025, 72, 256, 128, "D2R", steps=4, y_vec_ok=3),
    _c("d2r_yvec1_y8", 1025, 72, 256, 128, "D2R", steps=4, y_vec_ok=1, y_align=8),
    _c("d2r_yvec0_y2", 1025, 72, 256, 128, "D2R", steps=4, y_vec_ok=0, y_align=2),
    # ---- ... with fp32 slabs and the slab reduce, at a ragged M
    _c("d2r_slab", 1025, 64, 1024, 128, "D2R", splitk=4, steps=4, y_vec_ok=3),
    _c("d2r_slab_one_group", 1025, 72, 2048, 2048, "D2R", splitk=8, steps=4, y_vec_ok=3),
    _c("d2r_slab_y2_one_pass", 1025, 64, 1024, 128, "D2R", splitk=1, steps=16, y_vec_ok=0, y_align=2),  # no 8-byte stores: no slabs
    # ---- 3A2B kernel, 4-bit: what the direct-to-register kernel does not take (groups of 32, odd N)
    _c("3a2b4_g32", 1025, 72, 256, 32, "3A2B_W4", steps=4, y_vec_ok=1),
    _c("3a2b4_g32_slab", 1025, 64, 1024, 32, "3A2B_W4", splitk=4, steps=4, y_vec_ok=1),
    _c("3a2b4_odd_n", 40, 67, 256, 128, "3A2B_W4", steps=4, y_vec_ok=0),
    # ---- the older 256x256 kernel: K % 128 == 64
    _c("big_k192", 1025, 68, 192, 64, "BIG", y_vec_ok=1),
    _c("big_k320_g32", 40, 66, 320, 32, "BIG", y_vec_ok=0),
    # ---- 3A2B kernel, 8-bit
    _c("3a2b8_ragged_n", 300, 258, 256, 64, "3A2B_W8", steps=4, y_vec_ok=0, bits=8),
    _c("3a2b8_slab", 1025, 64, 1024, 128, "3A2B_W8", splitk=4, steps=4, y_vec_ok=1, bits=8),
    # ---- strip kernels
    _c("strip8_m129", 129, 64, 128, 128, "STRIP8"),
    _c("strip8_ragged", 200, 388, 512, 64, "STRIP8"),
    _c("strip_k96", 65, 200, 96, 32, "STRIP"),
    _c("strip_m257", 257, 640, 1024, 64, "STRIP"),          # too few K-steps for K-slices (>= 4 per wave): one pass
    _c("strip_m257_split", 257, 200, 2048, 64, "STRIP", splitk=2),
    # ---- streaming kernel, 4-bit: the M ladder on a group-32 and a group-128 layer; M = 65 is the strip kernel's (boundary)
    *_ladder("stream4_g32", 200, 416, 32, "STREAM_W4", 1),
    _c("stream4_g32_m65_is_strip", 65, 200, 416, 32, "STRIP"),
    *_ladder("stream4_g128", 264, 1024, 128, "STREAM_W4", 2),
    _c("stream4_g128_m65_is_strip", 65, 264, 1024, 128, "STRIP"),
    _c("stream4_8step", 5, 64, 33280, 128, "STREAM_W4", splitk=33, row_blocks=1, steps=8),
    _c("stream4_kslice_limit", 17, 64, 32768, 128, "STREAM_W4", splitk=64, row_blocks=2, steps=4),
    _c("stream4_kslice_over_is_d2r", 17, 64, 32896, 128, "D2R", splitk=16, steps=34, y_vec_ok=3),
    # ---- streaming kernel, 8-bit
    *_ladder("stream8_g128", 200, 512, 128, "STREAM_W8", 1, bits=8),
    _c("stream8_g128_m65_is_3a2b8", 65, 200, 512, 128, "3A2B_W8", splitk=2, steps=4, y_vec_ok=1, bits=8),
    _c("stream8_g32_m5", 5, 200, 512, 32, "STREAM_W8", row_blocks=1, steps=4, bits=8),
    _c("stream8_g32_m33", 33, 200, 512, 32, "STREAM_W8", row_blocks=4, steps=4, bits=8),
    # ---- decode kernel without split-K: M <= 4; M = 5 on the same layer streams
    _c("gemv16_g32_m1", 1, 1000, 416, 32, "GEMV16"),
    _c("gemv16_g32_m4", 4, 1000, 416, 32, "GEMV16"),
    _c("gemv16_g32_m5_is_stream", 5, 1000, 416, 32, "STREAM_W4", row_blocks=1, steps=4),
    _c("gemv16_one_group_m1", 1, 200, 2048, 2048, "GEMV16"),
    _c("gemv16_one_group_m4", 4, 200, 2048, 2048, "GEMV16"),
    _c("gemv16_one_group_m5_is_stream", 5, 200, 2048, 2048, "STREAM_W4", splitk=4, row_blocks=1, steps=4),
    # ---- general 128x128 tile kernel, M > 16
    _c("tile4_group40", 100, 70, 200, 40, "TILE", x_vec_ok=1),
    _c("tile8_group40", 100, 70, 200, 40, "TILE", x_vec_ok=1, bits=8),
    _c("tile4_x2", 40, 128, 256, 128, "TILE", x_vec_ok=0, x_align=2),
    _c("tile8_x2", 40, 128, 256, 128, "TILE", x_vec_ok=0, x_align=2, bits=8),
    _c("tile4_g_idx", 100, 72, 256, 64, "TILE", x_vec_ok=1, g_idx=True),
    _c("tile8_g_idx", 100, 72, 256, 64, "TILE", x_vec_ok=1, g_idx=True, bits=8),
    # ---- generic split-K kernel + reduce, M <= 16
    _c("small_n60", 16, 60, 256, 128, "SMALL", splitk=2),
    _c("small_n70_group40", 5, 70, 200, 40, "SMALL", splitk=2),
    _c("small_x2", 5, 128, 256, 128, "SMALL", splitk=2, x_align=2),
    _c("small_g_idx", 7, 128, 256, 64, "SMALL", splitk=2, g_idx=True),
    _c("small8_k200", 5, 64, 200, 40, "SMALL", splitk=2, bits=8),
    _c("small8_n60", 16, 60, 256, 128, "SMALL", splitk=2, bits=8),
    # ---- odd widths: the tile kernel's per-element form
    _c("anyw_3bit", 40, 70, 192, 64, "TILE_ANYW", x_vec_ok=1, bits=3),
    _c("anyw_6bit", 40, 70, 192, 64, "TILE_ANYW", x_vec_ok=1, bits=6),
]
CASE_IDS = [c.name for c in CASES]


def dtype_code(dtype):
    from neural_compressor_amd import _lib

    return _lib.INC_BF16 if dtype is torch.bfloat16 else _lib.INC_F16


def query_route(c, dtype, x_ptr, y_ptr, bias_ptr, ws_ptr, ws_bytes):
    """ops.woq_gemm_route (inc_woq_gemm_route) for case c at these addresses -> dict(route, splitk, row_blocks, steps, y_vec_ok,
    x_vec_ok, need)."""
    from neural_compressor_amd import ops

    return ops.woq_gemm_route(c.M, c.N, c.K, c.group_size, c.bits, dtype, c.g_idx, x_ptr, y_ptr, bias_ptr, ws_ptr, ws_bytes)


def expected(c):
    return dict(route=c.route, splitk=c.splitk, row_blocks=c.row_blocks, steps=c.steps, y_vec_ok=c.y_vec_ok, x_vec_ok=c.x_vec_ok)


def misalign(align):
    """Byte offset from a 16-byte boundary that leaves an address `align`-byte aligned and no better."""
    return {16: 0, 8: 8, 2: 2}[align]


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
_layers = {}


def make_layer(N, K, group_size, bits, g_idx=False):
    """A packed layer in the optimum layout (numpy): asymmetric, scale and zero point of (column n, group g) walk through 41 / 2^bits
    values with strides 7 / 5 along n and 3 along g, so neighbouring columns differ by >= 11 % in scale and neighbouring groups by >= 5 %.
    Cached: the tests share it and must not write to it."""
    key = (N, K, group_size, bits, g_idx)
    if key in _layers:
        return _layers[key]
    rng = np.random.default_rng(1000003 * N + 1009 * K + 17 * group_size + bits)
    G = 1 if group_size >= K else -(-K // group_size)
    n, g = np.arange(N)[:, None], np.arange(G)[None, :]
    scales = (0.004 * (1.0 + 0.05 * ((7 * n + 3 * g) % 41))).astype(np.float32)
    levels = 1 << bits
    if bits == 8:  # keep q - zp inside int8 (recover() casts the difference to int8, modules.py:436)
        zp = 96 + (5 * n + 3 * g) % 64
    else:
        zp = (5 * n + 3 * g) % levels
    gi = rng.integers(0, G, size=K).astype(np.int32) if g_idx else None
    kgroup = gi if g_idx else np.minimum(np.arange(K) // group_size, G - 1)
    if bits == 8:
        iw = np.clip(zp[:, kgroup] + rng.integers(-100, 101, size=(N, K)), 0, 255)
    else:
        iw = rng.integers(0, levels, size=(N, K))
    qweight, qzeros, scales_gn = O.woq_pack_optimum(iw, scales, zp, bits)
    layer = dict(N=N, K=K, G=G, group_size=group_size, bits=bits, qweight=qweight, qzeros=qzeros, scales=scales_gn, g_idx=gi,
                 int_weight=iw, zp=zp)
    _layers[key] = layer
    return layer


def make_x(M, K, dtype):
    """Random activations with a few large entries, already rounded to `dtype`."""
    g = torch.Generator().manual_seed(7919 * M + K)
    x = torch.randn(M, K, generator=g)
    flat = x.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[: max(4, flat.numel() // 512)]] *= 12.0
    return x.to(dtype)


def make_bias(N, dtype):
    """Distinct per column (a permuted ramp), rounded to `dtype`."""
    n = torch.arange(N, dtype=torch.float32)
    return (((n * 37) % 101) * 0.03125 - 1.5 + n * 0.001).to(dtype)


_dense = {}


def dense_weight64(layer, dtype):
    """The oracle's dense weight (compute dtype = x dtype) in float64, cached per (layer, dtype)."""
    key = (layer["N"], layer["K"], layer["group_size"], layer["bits"], layer["g_idx"] is not None, dtype)
    if key not in _dense:
        _dense[key] = O.woq_dense_weight(layer["qweight"], layer["scales"], layer["qzeros"], layer["N"], layer["K"], layer["bits"],
                                         layer["group_size"], compute_dtype=dtype, g_idx=layer["g_idx"]).double()
    return _dense[key]


def reference(x, w64, bias):
    """(ref, S) in float64: ref = x @ w.T + bias, S = |x| @ |w|.T + |bias|."""
    x64, b64 = x.double(), bias.double()
    return x64 @ w64.t() + b64, x64.abs() @ w64.abs().t() + b64.abs()


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparator
# ---------------------------------------------------------------------------------------------------------------------------------------
def tolerance(ref, S, K, dtype):
    u_out = 2.0 ** -8 if dtype is torch.bfloat16 else 2.0 ** -11
    tiny = 0.0 if dtype is torch.bfloat16 else 2.0 ** -24
    return u_out * ref.abs() + 2.0 * (K + 4) * 2.0 ** -24 * S + tiny


def worst_ratio(y, ref, S, K, dtype):
    """max over the elements of |y - ref| / tol, and where; a non-finite output counts as infinitely wrong."""
    assert y.dtype is dtype and y.shape == ref.shape
    err = (y.double().cpu() - ref).abs()
    ratio = err / tolerance(ref, S, K, dtype)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    idx = int(torch.argmax(ratio))
    return float(ratio.view(-1)[idx]), divmod(idx, ref.shape[1])


def assert_elementwise(y, ref, S, K, dtype, what=""):
    r, (i, j) = worst_ratio(y, ref, S, K, dtype)
    assert r <= 1.0, (f"{what}: element ({i}, {j}) is off by {r:.3g} x its bound: got {float(y[i, j])!r}, reference {float(ref[i, j])!r}, "
                      f"S = {float(S[i, j])!r}")
    return r
