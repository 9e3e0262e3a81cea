"""The CPU oracle of the block-scaled FP8 cell and the cases of tests/test_fp8_block_cpu.py and tests/test_gpu_fp8_block.py.  No GPU code.

The specification is the comment of inc_fp8_quant_groups / inc_fp8_quant_blocks / inc_fp8_block_gemm / inc_fp8_block_gemv in
include/inc_mi355x.h.  The quantisers are that text in fp32 torch ops on the CPU (true division, max; the element rounding is
mx_cases.round_to_format); the product is float64: sum_kt f[m, n, kt] * (x_kt @ w_kt.T), with mass = sum_kt f * (|x_kt| @ |w_kt|.T).
"""

import torch

from tests.fp8_cases import DTYPE_IDS, DTYPES, OUT_DTYPES, SAT, SCALE_FLOOR, random_codes  # noqa: F401
from tests.mx_cases import FP8, code_table, encode_values, padded_k, round_to_format, ulp_of  # noqa: F401
from tests.mx_moe_cases import route_of

B = 128


def quant_blocked(t, rb, Kp=None):
    """One scale per rb x 128 block of t [R, K] (rb = 1: inc_fp8_quant_groups, rb = 128: inc_fp8_quant_blocks) -> (codes uint8 [R, Kp],
    scales fp32 [ceil(R/rb), Kp/128])."""
    R, K = t.shape
    Kp = padded_k(K) if Kp is None else Kp
    RB = -(-R // rb)
    p = torch.zeros((RB * rb, Kp), dtype=torch.float32)
    p[:R, :K] = t.to(torch.float32)
    blk = p.view(RB, rb, Kp // B, B)
    s = torch.maximum(blk.abs().amax(dim=(1, 3)) / torch.tensor(SAT, dtype=torch.float32), torch.tensor(SCALE_FLOOR, dtype=torch.float32))
    v = blk / s[:, None, :, None]                                       # fp32, true division
    code = round_to_format(v.to(torch.float64), FP8)[1] | (torch.signbit(blk).to(torch.int32) * 0x80)
    return code.to(torch.uint8).view(RB * rb, Kp)[:R].contiguous(), s


def product(xd, xs, wd, ws):
    """float64 values xd [M, Kp], wd [N, Kp], scales xs [M, KB], ws [ceil(N/128), KB] -> (y, mass)"""
    wse = ws.double().repeat_interleave(B, 0)[: wd.shape[0]]
    y = torch.zeros((xd.shape[0], wd.shape[0]), dtype=torch.float64)
    mass = torch.zeros_like(y)
    for kt in range(xd.shape[1] // B):
        f = xs[:, kt].double()[:, None] * wse[:, kt][None, :]
        xk, wk = xd[:, B * kt: B * kt + B], wd[:, B * kt: B * kt + B]
        y += f * (xk @ wk.T)
        mass += f * (xk.abs() @ wk.abs().T)
    return y, mass


# (rb, rows, K): groups at M in {1, 3} x every K tail, blocks at every N / K tail
QUANT_CASES = [(1, M, K) for K in (1, 127, 128, 129, 600) for M in (1, 3)] + [(128, N, K) for N, K in ((1, 1), (127, 129), (128, 128), (130, 600), (260, 384))]


def quant_input(R, K, dtype, rb):
    """Gaussian values with a magnitude 2^-6 .. 2^6 per rb x 128 block (neighbouring scales differ), one negative zero, exact in `dtype`."""
    g = torch.Generator().manual_seed(6000 + 7 * K + R + rb)
    e = torch.randint(-6, 7, (-(-R // rb), -(-K // B)), generator=g)
    x = torch.randn(R, K, generator=g) * torch.ldexp(torch.ones(()), e).repeat_interleave(rb, 0)[:R].repeat_interleave(B, 1)[:, :K]
    x[R - 1, K // 2] = -0.0
    return x.to(dtype)


GEMM_SHAPES, GEMM_KPS = [(1, 4), (17, 130), (257, 260)], [128, 384, 640]
GEMV_MS, GEMV_NS = [1, 15, 16], [7, 16, 130, 260]
GEMV_TILES = [1, 7, 8, 9, 26, 33]     # 8 waves, 4 tiles per round: no full round, one, and `left` = 1, 2, 3 on some wave (as inc_fp8_gemv)
CROSS_GEMM, CROSS_GEMV = (257, 260, 640), (16, 260, 3328)
_exact = {}


def exact_case(M, N, Kp):
    """Integer codes in -3 .. 3, xs[m, kt] = 2^((3m + kt) % 5 - 3), ws[nb, kt] = 2^((2nb + 3kt) % 4 - 2): they differ along every index,
    so the wrong tile's, row's or block's scale changes the result.  The smallest factor is 2^-5 and max(mass) * 2^5 < 2^24: every
    partial sum, in any order, is a multiple of 2^-5 with at most 24 bits -- exact in fp32.  bias: a multiple of 2^-4 up to 8."""
    if (M, N, Kp) not in _exact:
        g = torch.Generator().manual_seed(1900 + 131 * M + 17 * N + Kp)
        x, w = torch.randint(-3, 4, (M, Kp), generator=g), torch.randint(-3, 4, (N, Kp), generator=g)
        kt = torch.arange(Kp // B)[None, :]
        xs = torch.ldexp(torch.ones(()), (3 * torch.arange(M)[:, None] + kt) % 5 - 3)
        ws = torch.ldexp(torch.ones(()), (2 * torch.arange(-(-N // B))[:, None] + 3 * kt) % 4 - 2)
        bias = torch.randint(-128, 129, (N,), generator=g).double() / 16
        y, mass = product(x.double(), xs, w.double(), ws)
        assert float(xs.min() * ws.min()) >= 2.0 ** -5 and float(mass.max()) * 2.0 ** 5 < 2.0 ** 24
        assert float(y.abs().max()) + 8 < 60000.0                                               # finite in fp16
        _exact[(M, N, Kp)] = dict(xq=encode_values(x, FP8), wq=encode_values(w, FP8), xs=xs, ws=ws, bias=bias, y=y, yb=y + bias[None, :])
    return _exact[(M, N, Kp)]


def random_scales(M, N, Kp, seed):
    """Positive non-power-of-two scales |N(0, 1)| * 2^-9 + 2^-12 (fp16 outputs of random codes stay finite) and a bias exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    xs = (torch.randn(M, Kp // B, generator=g).abs() * 2.0 ** -9 + 2.0 ** -12).float()
    ws = (torch.randn(-(-N // B), Kp // B, generator=g).abs() * 2.0 ** -9 + 2.0 ** -12).float()
    return xs, ws, (torch.randn(N, generator=g) * 4).to(torch.bfloat16).double()


# ---- the routed experts GEMM (tests/test_gpu_fp8_block_moe.py, scripts/strip_outputs_digest.py) -----------------------------------------
MOE_EXACT = [("edges3", 4, 128), ("edges3", 260, 1024), ("edges3", 264, 1152), ("edges", 264, 3328), ("one_slot", 20, 256),
             ("all_invalid", 20, 256)]          # (routing, Nout, Kp) of modes 2 and 1
MOE_EXACT_MODE0 = [(136, 1024), (7, 256)]      # (I, Kp) on "edges3"


def moe_reference(ro, mode, ad, as_, wd, ws):
    """float64 over the valid positions: (val, mass) [nvalid, N], the named source rows.  Mode 0: each half of ws is blocked from its row 0."""
    nv, order, k, (E, N), KB = ro["nvalid"], ro["order"].long(), ro["k"], wd.shape[:2], as_.shape[1]
    wse = ws.double().reshape(E, 2 if mode == 0 else 1, -1, KB).repeat_interleave(B, 2)[:, :, :N // 2 if mode == 0 else N].reshape(E, N, KB)
    val, mass, named = torch.zeros(nv, N, dtype=torch.float64), torch.zeros(nv, N, dtype=torch.float64), torch.zeros(ad.shape[0], dtype=torch.bool)
    for e in range(E):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        src = torch.arange(lo, hi) if mode == 1 else order[lo:hi] // k
        named[src] = True
        for kt in range(KB if lo < hi else 0):
            f = as_[src, kt].double()[:, None] * wse[e, :, kt][None, :]
            xk, wk = ad[src, B * kt:B * kt + B], wd[e][:, B * kt:B * kt + B]
            val[lo:hi] += f * (xk @ wk.T)
            mass[lo:hi] += f * (xk.abs() @ wk.abs().T)
    return val, mass, named


def moe_exact(routing, mode, Nout, Kp):
    """Integers in -3..3 (per expert from its own seed; mode 0: gate rows from {-1, 0, 1}, two zeros in three), as[r, kt] =
    2^((3r + kt) % 5 - 3), ws[e, nb, kt] = 2^((2(nb + 7e) + kt + 1) % 5 - 3) (mode 0: both exponents 3 lower); unnamed rows poisoned."""
    ro = route_of(routing)
    E, N, shift = ro["E"], (2 if mode == 0 else 1) * Nout, 6 if mode == 0 else 3
    rows, kt, nblk = (ro["S"] if mode == 1 else ro["T"]), torch.arange(Kp // B), (2 if mode == 0 else 1) * -(-Nout // B)
    a = torch.randint(-3, 4, (rows, Kp), generator=torch.Generator().manual_seed(5151 + 7 * Nout + Kp + mode))
    as_ = torch.ldexp(torch.ones(()), (3 * torch.arange(rows)[:, None] + kt) % 5 - shift)
    w = torch.empty((E, N, Kp), dtype=torch.int64)
    for e in range(E):
        ge = torch.Generator().manual_seed(800001 + 7919 * e + Nout + Kp + mode)
        w[e] = torch.randint(-3, 4, (N, Kp), generator=ge)
        if mode == 0:
            w[e, :Nout] = torch.randint(-1, 2, (Nout, Kp), generator=ge) * torch.randint(0, 2, (Nout, Kp), generator=ge)
    ws = torch.ldexp(torch.ones(()), (2 * (torch.arange(nblk)[None, :, None] + 7 * torch.arange(E)[:, None, None]) + kt + 1) % 5 - shift)
    val, mass, named = moe_reference(ro, mode, a.double(), as_, w.double(), ws)
    assert bool((val.float().double() == val).all()) and bool((mass < 2.0 ** 17 * float(as_.max() * ws.max())).all())
    aq, wq = encode_values(a, FP8), encode_values(w.view(E * N, Kp), FP8).view(E, N, Kp)
    aq[~named], as_[~named] = 0xFF, float("nan")
    return ro, aq, as_, wq, ws, val
