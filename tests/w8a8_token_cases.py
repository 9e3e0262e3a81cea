"""Shared by tests/test_w8a8_token_cpu.py and tests/test_gpu_w8a8_token.py (a helper module, not a conftest): the oracle of the dynamic
per-token symmetric int8 activation cell of SmoothQuant W8A8, its inputs and its comparators.  Nothing here comes from a kernel.

The cell has no reference text; its specification, all fp32 with true division and round-half-even:

  t[k]   = float(x[m,k]) * in_scale[k]                      (the multiply only when in_scale is given)
  s[m]   = max(max_k |t[k]| / 127, FLT_EPSILON)
  q[k]   = clamp(rint(t[k] / s[m]), -127, 127) as int8,  0 for K <= k < Kp
  y[m,n] = rd16((s[m] * w_scale[n]) * float(acc[m,n]) + bias[n]),   acc = sum_k q[m,k] * wq[n,k]  (int32)

torch on the CPU does each of these steps as one correctly rounded fp32 operation (the divisors are tensors, never host scalars), and
max is order-free, so q and s have one right answer bit for bit; without bias so has y.  acc comes from tests/w8a8_route_cases.accumulate
(float64, exact).  With bias the multiply-add may or may not be fused: the bound of tests/w8a8_route_cases.assert_within_ulp.
"""

import collections

import torch

from tests import w8a8_route_cases as R

EPS = float(torch.finfo(torch.float32).eps)
HELD_KP = 16384       # sq.hip: QT_HELD * 256 * 16, the longest padded row quant_act_token_kernel keeps in registers
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]

TIES = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, -126.5]
TIES_Q = [127, 0, 2, 2, 0, -2, -2, 126, -126]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
def quant_token(x, in_scale=None, Kp=None):
    """x [M, K] (any float type, CPU) -> (q int8 [M, Kp], s fp32 [M])."""
    assert x.device.type == "cpu" and x.dim() == 2
    M, K = x.shape
    Kp = K if Kp is None else Kp
    t = x.float()
    if in_scale is not None:
        t = t * in_scale.float().view(1, -1)
    amax = t.abs().amax(dim=1)
    s = torch.maximum(amax / torch.full_like(amax, 127.0), torch.full_like(amax, EPS))
    q = torch.zeros((M, Kp), dtype=torch.int8)
    q[:, :K] = torch.round(t / s.view(-1, 1)).clamp_(-127.0, 127.0).to(torch.int8)
    return q, s


def dequant(q, s, K):
    return q[:, :K].float() * s.view(-1, 1)


def expect_no_bias(row_scale, w_scale, acc, dtype):
    """Two fp32 multiplies in the written order, one int32 -> fp32 conversion, one rounding."""
    return ((row_scale.view(-1, 1) * w_scale.view(1, -1)) * acc.float()).to(dtype)


def exact_with_bias(row_scale, w_scale, acc, bias):
    """float64 of the fp32 factor; `bias` already rounded to the output type."""
    return (row_scale.view(-1, 1) * w_scale.view(1, -1)).double() * acc + bias.double().view(1, -1)


def gemm_row_scale(M):
    """row_scale[m] = (1 + (37 m % 101) / 128) * 2^(m % 5 - 8): neighbouring rows differ in mantissa and exponent."""
    m = torch.arange(M)
    return ((1.0 + ((37 * m) % 101).double() / 128.0) * torch.pow(2.0, (m % 5 - 8).double())).float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# quantiser cases
# ---------------------------------------------------------------------------------------------------------------------------------------
# specials: the rows 1, 2, ... of the case, in this order ("zero", "last_neg", "first", "ties"); row 0 and the rest stay random
QCase = collections.namedtuple("QCase", "name M K Kp specials unaligned")
ALL = ("zero", "last_neg", "first", "ties")
QCASES = [
    QCase("m1_k128", 1, 128, 128, (), False),                                  # 8 chunks: lanes 8 .. 255 hold nothing
    QCase("m3_k100_ragged", 3, 100, 128, ("zero", "last_neg"), False),         # K % 8 != 0: element-wise loads, 28 padding bytes
    QCase("m16_k4224", 16, 4224, 4224, ALL, False),                            # 264 chunks: lanes 0 .. 7 hold two
    QCase("m17_k768", 17, 768, 768, ALL, False),
    QCase("m17_k768_unaligned", 17, 768, 768, ALL, True),                      # x starts one element past a 16-byte boundary
    QCase("m300_k1000_pad", 300, 1000, 1024, ALL, False),                      # K % 8 == 0, the last chunk is half padding
    QCase("m3_k16384_held_max", 3, HELD_KP, HELD_KP, ("ties", "last_neg"), False),       # every lane holds four chunks
    QCase("m3_k16512_two_reads", 3, HELD_KP + 128, HELD_KP + 128, ("first", "ties"), False),  # the first length of the two-read kernel
    QCase("m3_k16500_two_reads_ragged", 3, HELD_KP + 116, HELD_KP + 128, ("zero", "last_neg"), False),
]
QCASE_IDS = [c.name for c in QCASES]


def quant_inputs(c, dtype, with_in_scale):
    """-> (x [M, K] of `dtype`, in_scale fp32 [K] or None), CPU.  Row m is N(0, 1) * 2^(m % 7 - 3); the special rows: all zero / the
    amax is the LAST valid element and negative / the amax is element 0 / half-integer ties with amax exactly 127 (s == 1; only without
    in_scale are they still ties after the multiply)."""
    g = torch.Generator().manual_seed(7919 * c.M + c.K + (1 if with_in_scale else 0))
    x = torch.randn(c.M, c.K, generator=g) * torch.pow(2.0, (torch.arange(c.M) % 7 - 3).float()).view(-1, 1)
    for i, kind in enumerate(c.specials):
        r = 1 + i
        assert r < c.M
        if kind == "zero":
            x[r] = 0
        elif kind == "last_neg":
            x[r, -1] = -64.0 * float(x[r].abs().max())
        elif kind == "first":
            x[r, 0] = 64.0 * float(x[r].abs().max())
        else:
            k = torch.arange(c.K)
            x[r] = (k % 253 - 126).float() + 0.5        # -125.5 .. 126.5: exact in bf16
            x[r, :len(TIES)] = torch.tensor(TIES)
    in_scale = (0.5 + 1.5 * torch.rand(c.K, generator=g)) if with_in_scale else None
    return x.to(dtype), in_scale


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------------------------
def assert_quant_equal(q, s, want_q, want_s, what=""):
    """Every byte of q [M, Kp] (the padding included) and every bit of s [M]."""
    assert q.dtype is torch.int8 and q.shape == want_q.shape, (what, q.dtype, tuple(q.shape), tuple(want_q.shape))
    assert s.dtype is torch.float32 and s.shape == want_s.shape, (what, s.dtype, tuple(s.shape), tuple(want_s.shape))
    bad = s.view(torch.int32) != want_s.view(torch.int32)
    if bool(bad.any()):
        m = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {s.numel()} row scales differ in bits, first at row {m}: got {float(s[m])!r}, "
                             f"want {float(want_s[m])!r}")
    bad = q != want_q
    if bool(bad.any()):
        m, k = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {q.numel()} codes differ, first at ({m}, {k}): got {int(q[m, k])}, "
                             f"want {int(want_q[m, k])}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the accuracy condition: T = 64 tokens of N(0, 1), K = 256, token OUTLIER_ROW times 64
# ---------------------------------------------------------------------------------------------------------------------------------------
OUT_T, OUT_K, OUTLIER_ROW, OUTLIER_GAIN = 64, 256, 17, 64.0
ACC_SEEDS = [0, 1, 2, 3, 4]
ACC_RATIO = 0.1


def outlier_input(seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(OUT_T, OUT_K, generator=g)
    x[OUTLIER_ROW] *= OUTLIER_GAIN
    return x.to(dtype)


def ordinary(t):
    """The 63 rows other than the outlier token."""
    keep = torch.ones(t.shape[0], dtype=torch.bool)
    keep[OUTLIER_ROW] = False
    return t[keep.to(t.device)]


def rel_err(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def static_qdq(x):
    """The static cell's fake quantisation with the range calibrated on x itself: per-tensor asymmetric uint8 (the arithmetic of
    quant_dequant_x_v1 / SQLinearWrapper._calculate_qparams, restated here so that the CPU figures need nothing from the package)."""
    t = x.float()
    mn, mx = torch.clamp(t.min(), max=0.0), torch.clamp(t.max(), min=0.0)
    scale = torch.clamp((mx - mn) / torch.tensor(255.0), min=EPS)
    zp = torch.clamp(-torch.round(mn / scale), 0, 255)
    return (torch.clamp(torch.round(t / scale + zp), 0, 255) - zp) * scale


def token_qdq(x):
    q, s = quant_token(x)
    return dequant(q, s, x.shape[1])

