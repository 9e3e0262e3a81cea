"""Shared by tests/test_w8a8_routes_cpu.py and tests/test_gpu_w8a8_routes.py (a helper module, not a conftest).

  * a pure-Python mirror of the host plan of the SmoothQuant W8A8 GEMM (neural_compressor_amd/csrc/gemm_i8.hip: i8_tail_plan, the
    per-split K-step arithmetic of w8a8_gemm_kernel, the GEMV's M buckets).  The library exports only inc_w8a8_gemm_workspace_bytes
    about its plan; the CPU test ties the mirror to it, so a retuned threshold shows up there first;
  * CASES: the route table.  Each case names the kernel, the tile counts, the K-split and its steps, and the store form it was
    written for.  When a threshold moves a case off its route: move the shape so that the route keeps a case, never drop the route;
  * the inputs of a case (int8 codes over the full range, a per-column alpha that differs clearly between neighbours, int32
    corr, a per-column bias; a seeded generator per case) and the exact reference;
  * the two comparators.

Reference.  acc = xq.double() @ wq.double().T is exact: |sum| <= 2^14 * K << 2^53, whatever the order of the additions.
  without corr / bias   the epilogue is one fp32 multiply and one rounding: y == (alpha * acc.float()).to(dtype), bit for bit;
  with corr and bias    the multiply-add may or may not be fused: |y - exact| <= ulp * |exact| + 1e-6 per element with
                        ulp = 2^-7 (bf16) / 2^-10 (fp16) and exact in float64 -- the bound of tests/test_gpu_sq.py, nothing new.
"""

import collections

import torch

# constants of gemm_i8.hip
IM, IN, IK = 256, 256, 128     # tile: rows of x, rows of w, K bytes per step
I_CUS = 256                    # workgroups per round
MAX_SPLIT = 8
MIN_STEPS_FEW, MIN_STEPS = 4, 24   # K-steps per split at least: fewer than I_CUS / 4 tiles / otherwise
SLAB_BYTES = IM * IN * 4
GV_MAXM, GV_KC, GV_ROWS = 16, 4096, 4
BAND = 8                       # banded_tile_decode (common.hpp)
XCDS = 8


def ceil_div(a, b):
    return -(-a // b)


def tail_plan(tiles, nk):
    """i8_tail_plan -> (split, full_tiles)."""
    tail = tiles % I_CUS
    if tail == 0:
        return 1, tiles
    split = min(I_CUS // tail, MAX_SPLIT)
    min_steps = MIN_STEPS_FEW if tiles < I_CUS // 4 else MIN_STEPS
    while split > 1 and nk // split < min_steps:
        split -= 1
    if split <= 1:
        return 1, tiles
    return split, tiles - tail


def split_steps(nk_all, split):
    """The kernel's per-split arithmetic -> (steps, [(kbase, nk) of split 0 .. split - 1]); nk <= 0 is an empty split."""
    steps = ceil_div(nk_all, split)
    return steps, [(ks * steps, min(steps, nk_all - ks * steps)) for ks in range(split)]


def gemv_bucket(M):
    return 1 if M == 1 else 4 if M <= 4 else 8 if M <= 8 else 16


def workspace_bytes(M, N, K):
    """inc_w8a8_gemm_workspace_bytes."""
    if M <= GV_MAXM or N <= 0 or K <= 0 or K % IK:
        return 0
    tiles = ceil_div(M, IM) * ceil_div(N, IN)
    split, full = tail_plan(tiles, K // IK)
    return (tiles - full) * split * SLAB_BYTES if split > 1 else 0


def plan(M, N, K, y_align=16, workspace=True):
    """What inc_w8a8_gemm launches for this call, as the fields of Case.  GEMV: `steps` counts the K chunks of GV_KC bytes staged in
    LDS and `nk_last` the 128-byte pieces of the last one; it has one store form (y_vec_ok = -1)."""
    assert K % IK == 0
    if M <= GV_MAXM:
        chunks = ceil_div(K, GV_KC)
        return dict(kernel="GEMV", tiles=0, full_tiles=0, split=1, steps=chunks, nk_last=(K - (chunks - 1) * GV_KC) // IK, y_vec_ok=-1,
                    mt=gemv_bucket(M))
    tiles = ceil_div(M, IM) * ceil_div(N, IN)
    nk_all = K // IK
    split, full = tail_plan(tiles, nk_all)
    if split > 1 and not workspace:
        split, full = 1, tiles
    steps, per_split = split_steps(nk_all, split)
    return dict(kernel="MFMA", tiles=tiles, full_tiles=full, split=split, steps=steps, nk_last=per_split[-1][1],
                y_vec_ok=int(N % 4 == 0 and y_align >= 8), mt=0)


def xcd_remap(wg, full_tiles):
    """Block wg < full_tiles -> the tile it computes (block b runs on XCD b % 8; an XCD gets a contiguous run of tiles)."""
    q, r = divmod(full_tiles, XCDS)
    xcd, idx = wg % XCDS, wg // XCDS
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def banded_tile_decode(idx, tiles_m, tiles_n):
    per_band = BAND * tiles_n
    band = idx // per_band
    first = band * BAND
    rows = min(tiles_m - first, BAND)
    r = idx - band * per_band
    return first + r % rows, r // rows


# y_align: the largest power of two (bytes) the address of y is a multiple of (16 or 2).  fill: "uniform" or "saturated".
Case = collections.namedtuple("Case", "name M N K kernel tiles full_tiles split steps nk_last y_vec_ok y_align fill mt")


def _c(name, M, N, K, tiles, full_tiles, split, steps, nk_last, y_vec_ok, y_align=16, fill="uniform"):
    return Case(name, M, N, K, "MFMA", tiles, full_tiles, split, steps, nk_last, y_vec_ok, y_align, fill, 0)


def _gemv(name, M, N, K, mt, chunks, nk_last):
    return Case(name, M, N, K, "GEMV", 0, 0, 1, chunks, nk_last, -1, 16, "uniform", mt)


CASES = [
    # ---- K-split tail tiles: every tile is split, the finish kernel sums the slabs
    # M = 33: of the upper wave row only row blocks 0 and 1 are parked; the ragged N tile is 8 columns wide
    _c("split2_pair", 33, 264, 1024, tiles=2, full_tiles=0, split=2, steps=4, nk_last=4, y_vec_ok=1),
    # 33 K-steps over 8 splits of 5: split 6 has 3, split 7 starts at 35 and has none (nk = -2): a zero slab
    _c("split8_empty_last", 32, 256, 4224, tiles=1, full_tiles=0, split=8, steps=5, nk_last=-2, y_vec_ok=1),
    # 5 + 4 steps, odd N (scalar stores in the finish kernel), the second M tile has 44 rows
    _c("split2_uneven_scalar_store", 300, 1001, 1152, tiles=8, full_tiles=0, split=2, steps=5, nk_last=4, y_vec_ok=0),
    # one row and one column in the ragged tiles
    _c("split2_four_tiles", 257, 257, 1024, tiles=4, full_tiles=0, split=2, steps=4, nk_last=4, y_vec_ok=0),
    _c("split_y_misaligned", 64, 256, 1024, tiles=1, full_tiles=0, split=2, steps=4, nk_last=4, y_vec_ok=0, y_align=2),
    # all codes -128, alpha = 1: every sum is 16384 * K = 2^25
    _c("saturated", 40, 272, 2048, tiles=2, full_tiles=0, split=4, steps=4, nk_last=4, y_vec_ok=1, fill="saturated"),
    # the first row count of the MFMA kernel; its first 16 rows must equal the GEMV's (gemv_m16 has the same N and K)
    _c("handover_m17", 17, 50, 4224, tiles=1, full_tiles=0, split=8, steps=5, nk_last=-2, y_vec_ok=0),
    # ---- one pass: the XCD remap and the banded decode
    _c("unsplit_y_misaligned", 64, 256, 384, tiles=1, full_tiles=1, split=1, steps=3, nk_last=3, y_vec_ok=0, y_align=2),
    _c("unsplit_odd_n", 40, 67, 256, tiles=1, full_tiles=1, split=1, steps=2, nk_last=2, y_vec_ok=0),
    _c("remap_r_nonzero", 257, 1300, 384, tiles=12, full_tiles=12, split=1, steps=3, nk_last=3, y_vec_ok=1),   # q = 1, r = 4
    _c("band_partial", 2049, 264, 384, tiles=18, full_tiles=18, split=1, steps=3, nk_last=3, y_vec_ok=1),     # tiles_m = 9; q = 2, r = 2
    # ---- 256 remapped full tiles, then 16 tail tiles x 2 splits of 24 steps; tiles_m = 17.  The one large case.
    _c("full_round_plus_split_tail", 4097, 4096, 6144, tiles=272, full_tiles=256, split=2, steps=24, nk_last=24, y_vec_ok=1),
    # ---- GEMV: every M (M < MT in each bucket), N no multiple of the 16 rows of a workgroup, a second K chunk of 128 bytes
    *[_gemv(f"gemv_m{M}", M, 50, 4224, mt, 2, 1)
      for M, mt in ((1, 1), (2, 4), (3, 4), (4, 4), (5, 8), (6, 8), (7, 8), (8, 8), (9, 16), (10, 16), (11, 16), (12, 16), (13, 16),
                    (14, 16), (15, 16), (16, 16))],
    _gemv("gemv_k128", 5, 64, 128, 8, 1, 1),        # lanes 0 .. 7 of a wave load, the others nothing
    _gemv("gemv_k8192", 9, 48, 8192, 16, 2, 32),    # two exact chunks
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}


def expected(c):
    return dict(kernel=c.kernel, tiles=c.tiles, full_tiles=c.full_tiles, split=c.split, steps=c.steps, nk_last=c.nk_last,
                y_vec_ok=c.y_vec_ok, mt=c.mt)


def tiles_m(c):
    return ceil_div(c.M, IM)


def misalign(align):
    """Byte offset from a 16-byte boundary that leaves an address `align`-byte aligned and no better."""
    return {16: 0, 2: 2}[align]


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs and reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(c):
    """CPU tensors of a case: xq int8 [M, K], wq int8 [N, K], alpha fp32 [N], corr int32 [N], bias fp32 [N] (round it to the output
    type before use).  alpha walks through 13 levels with stride 7: neighbouring columns differ by a factor >= 1.5 either way."""
    M, N, K = c.M, c.N, c.K
    if c.fill == "saturated":
        return dict(xq=torch.full((M, K), -128, dtype=torch.int8), wq=torch.full((N, K), -128, dtype=torch.int8),
                    alpha=torch.ones(N), corr=None, bias=None)
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    xq = torch.randint(-128, 128, (M, K), generator=g, dtype=torch.int32).to(torch.int8)
    wq = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8)
    n = torch.arange(N)
    alpha = (1e-5 * (1 + (7 * n) % 13)).to(torch.float32)
    corr = torch.randint(-100000, 100000, (N,), generator=g, dtype=torch.int32)
    bias = torch.randn(N, generator=g) * 0.5
    return dict(xq=xq, wq=wq, alpha=alpha, corr=corr, bias=bias)


def accumulate(xq, wq):
    """xq @ wq^T, exact, in float64 (on whatever device the operands are: torch's matmul, independent of the kernel under test)."""
    return xq.double() @ wq.double().T


def expect_no_bias(alpha, acc, dtype):
    """One fp32 multiply, one rounding."""
    return (alpha.view(1, -1) * acc.float()).to(dtype)


def exact_with_bias(alpha, acc, corr, bias):
    """float64; `bias` already rounded to the output type."""
    return alpha.double().view(1, -1) * (acc + corr.double().view(1, -1)) + bias.double().view(1, -1)


def ulp(dtype):
    return 2.0 ** -7 if dtype is torch.bfloat16 else 2.0 ** -10


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------------------------
def assert_bit_equal(y, want, what=""):
    assert y.dtype is want.dtype and y.shape == want.shape, (what, y.dtype, want.dtype, tuple(y.shape), tuple(want.shape))
    bad = y.view(torch.int16) != want.view(torch.int16)
    n = int(bad.sum())
    if n:
        i, j = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {n} of {y.numel()} elements differ in bits, first at ({i}, {j}): got {float(y[i, j])!r}, "
                             f"want {float(want[i, j])!r}")


def assert_within_ulp(y, exact, dtype, what=""):
    assert y.dtype is dtype and y.shape == exact.shape
    err = (y.double() - exact).abs()
    ok = err <= ulp(dtype) * exact.abs() + 1e-6   # (a NaN compares false)
    n = int((~ok).sum())
    if n:
        i, j = (int(v) for v in (~ok).nonzero()[0])
        raise AssertionError(f"{what}: {n} of {y.numel()} elements are out of bound, first at ({i}, {j}): got {float(y[i, j])!r}, "
                             f"exact {float(exact[i, j])!r}")
