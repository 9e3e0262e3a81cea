"""The CPU oracle of the per-token / per-channel FP8 cell and the cases of tests/test_fp8_cpu.py and tests/test_gpu_fp8.py.  No GPU code.

The specification is the comment of inc_fp8_quant_rows / inc_fp8_gemm / inc_fp8_gemv in include/inc_mi355x.h.  The quantiser oracle is
that text in fp32 torch ops on the CPU (true division, max); the element rounding is mx_cases.round_to_format (float64, frexp, round
half to even -- nothing of the kernel's bit arithmetic).

  quant_rows(x, in_scale, Kp)  -> (codes uint8 [M,Kp], row_scale fp32 [M])
  dequant(codes, scale)        -> float64 [M,Kp]: code table * scale
  exact_case(M, N, Kp)         -> integer operands, power-of-two factors and the exact float64 result
  random_codes(M, N, Kp, seed) -> uniform e4m3 bytes with the two NaN codes remapped, and their float64 values
"""

import torch

from tests.mx_cases import FP8, FP8_TIES, FP8_TIES_TO, code_table, encode_values, padded_k, round_to_format, ulp_of  # noqa: F401

SAT = 448.0
SCALE_FLOOR = 2.0 ** -60
HELD_MAX = 16384            # padded row length up to which the kernel keeps the row in registers
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]
OUT_DTYPES = [torch.bfloat16, torch.float16]


def quant_rows(x, in_scale=None, Kp=None):
    """The row quantiser of the specification, fp32 on the CPU."""
    M, K = x.shape
    Kp = padded_k(K) if Kp is None else Kp
    assert Kp % 128 == 0 and Kp >= K
    t = x.to(torch.float32)
    if in_scale is not None:
        t = t * in_scale.to(torch.float32)[None, :]
    amax = t.abs().amax(dim=1)
    s = torch.maximum(amax / torch.tensor(SAT, dtype=torch.float32), torch.tensor(SCALE_FLOOR, dtype=torch.float32))
    v = t / s[:, None]                                        # fp32, true division
    _, code = round_to_format(v.to(torch.float64), FP8)
    code = code | (torch.signbit(t).to(torch.int32) * 0x80)
    out = torch.zeros((M, Kp), dtype=torch.uint8)
    out[:, :K] = code.to(torch.uint8)
    return out, s


def dequant(codes, scale):
    """float64: the value of every code times its row's scale."""
    return code_table(FP8)[codes.long()] * scale.to(torch.float64)[:, None]


class FakeQuantLinear(torch.nn.Module):
    """The float emulation of the cell: both operands through quant / dequant (on the CPU), the product in `dtype`."""

    def __init__(self, linear, dtype=torch.float32):
        super().__init__()
        w = linear.weight.detach().cpu()
        q, s = quant_rows(w)
        self.register_buffer("weight", dequant(q, s)[:, : w.shape[1]].to(dtype).to(linear.weight.device))
        self.register_buffer("bias", None if linear.bias is None else linear.bias.detach().to(dtype))

    def forward(self, x):
        x2 = x.reshape(-1, x.shape[-1])
        q, s = quant_rows(x2.detach().cpu())
        xd = dequant(q, s)[:, : x2.shape[1]].to(self.weight.dtype).to(x.device)
        y = torch.nn.functional.linear(xd, self.weight, self.bias)
        return y.reshape(*x.shape[:-1], -1).to(x.dtype)


# ---- quantiser cases ------------------------------------------------------------------------------------------------------------------
QUANT_KS = [1, 15, 16, 17, 128, 129, 600, 4112]
QUANT_MS = [1, 3]
REREAD_K = 16400            # padded to 16512 > HELD_MAX: the row is read twice

_qin = {}


def quant_input(M, K, dtype, seed=0):
    """Gaussian rows with per-row magnitudes 2^-6 .. 2^6, one negative zero, exact in `dtype`; built once."""
    key = (M, K, dtype, seed)
    if key not in _qin:
        g = torch.Generator().manual_seed(4000 + 7 * K + M + seed)
        x = torch.randn(M, K, generator=g) * torch.ldexp(torch.ones(M, 1), torch.randint(-6, 7, (M, 1), generator=g))
        x[M - 1, K // 2] = -0.0
        _qin[key] = x.to(dtype)
    return _qin[key]


def in_scale_for(K):
    g = torch.Generator().manual_seed(5000 + K)
    return (torch.rand(K, generator=g) * 1.5 + 0.25).to(torch.float32)


def ties_row(j, K=128):
    """A row whose largest magnitude is 448 * 2^j, so its scale is exactly 2^j, holding every e4m3 tie of mx_cases scaled by 2^j with
    both signs -> (row fp32 [K], the grid values the codes must carry, without the scale, [K]).  The two entries of FP8_TIES above 448
    (the MX cell's saturation band) are left out: a value above 448 * 2^j would itself be the row's maximum and move the scale off 2^j
    -- in this cell |t| / s never exceeds 448 by more than one rounding."""
    pairs = [(t, to) for t, to in zip(FP8_TIES, FP8_TIES_TO) if t <= SAT]
    assert len(pairs) == len(FP8_TIES) - 2
    vals = [SAT, -SAT, 0.0, -0.0] + [t for t, _ in pairs] + [-t for t, _ in pairs]
    want = [SAT, -SAT, 0.0, -0.0] + [to for _, to in pairs] + [-to for _, to in pairs]
    row = torch.zeros(K, dtype=torch.float64)
    to = torch.zeros(K, dtype=torch.float64)
    row[: len(vals)] = torch.tensor(vals, dtype=torch.float64) * 2.0 ** j
    to[: len(want)] = torch.tensor(want, dtype=torch.float64)
    assert bool((row.float().double() == row).all())          # every value is exact in fp32
    return row.float(), to


# ---- product cases --------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 4), (17, 7), (255, 260), (256, 256), (257, 264)]
GEMM_KPS = [128, 256, 384, 640]
GEMV_MS = [1, 15, 16]
GEMV_NS = [4, 7, 16, 17, 260]
GEMV_TILES = [1, 7, 8, 9, 26, 33]     # W = 8 waves, UNROLL = 4: full rounds and every `left` branch
CROSS_GEMM = (257, 260, 640)
CROSS_GEMV = (16, 260, 3328)

_exact = {}


def exact_case(M, N, Kp):
    """Integer operands in -3 .. 3 (as mx_cases.exact_operands draws them), row_scale[m] = 2^((3m) % 5 - 3), alpha[n] = 2^((2n + 1) % 5
    - 3), bias a multiple of 2^-4 up to 8.  acc is an integer below 2^17, the factor product a power of two in 2^-6 .. 2^2, so
    (s a) acc + bias is a multiple of 2^-6 below 2^19 + 8: exact in fp32 with or without the contraction, in any summation order."""
    key = (M, N, Kp)
    if key not in _exact:
        g = torch.Generator().manual_seed(900 + 131 * M + 17 * N + Kp)
        x = torch.randint(-3, 4, (M, Kp), generator=g)
        w = torch.randint(-3, 4, (N, Kp), generator=g)
        rs = torch.ldexp(torch.ones(M, dtype=torch.float64), (3 * torch.arange(M)) % 5 - 3)
        al = torch.ldexp(torch.ones(N, dtype=torch.float64), (2 * torch.arange(N) + 1) % 5 - 3)
        bias = torch.randint(-128, 129, (N,), generator=g).double() / 16
        acc = x.double() @ w.double().T
        y = (rs[:, None] * al[None, :]) * acc
        yb = y + bias[None, :]
        assert float((x.abs().double() @ w.abs().double().T).max()) < 2.0 ** 17
        for t in (y, yb):
            assert bool((t.float().double() == t).all()) and float(t.abs().max()) < 60000.0   # exact in fp32, finite in fp16
        _exact[key] = dict(xq=encode_values(x, FP8), wq=encode_values(w, FP8), rs=rs.float(), al=al.float(), bias=bias, y=y, yb=yb)
    return _exact[key]


_random = {}


def random_codes(M, N, Kp, seed):
    """Uniform bytes with the NaN codes 0x7f / 0xff moved to 0x7e / 0xfe -> codes and their float64 values, acc64 and the absolute mass."""
    key = (M, N, Kp, seed)
    if key not in _random:
        g = torch.Generator().manual_seed(seed)
        def draw(rows):
            q = torch.randint(0, 256, (rows, Kp), generator=g).to(torch.uint8)
            return torch.where((q & 0x7F) == 0x7F, q - 1, q)
        xq, wq = draw(M), draw(N)
        xd, wd = code_table(FP8)[xq.long()], code_table(FP8)[wq.long()]
        assert bool(torch.isfinite(xd).all()) and bool(torch.isfinite(wd).all())
        _random[key] = dict(xq=xq, wq=wq, acc=xd @ wd.T, mass=xd.abs() @ wd.abs().T)
    return _random[key]


def gaussian_factors(M, N, seed):
    """Non-power-of-two positive factors: |N(0, 1)| * 2^-9 + 2^-12 (the random codes' sums reach 10^6; this keeps fp16 outputs finite)."""
    g = torch.Generator().manual_seed(seed)
    rs = (torch.randn(M, generator=g).abs() * 2.0 ** -9 + 2.0 ** -12).float()
    al = (torch.randn(N, generator=g).abs() * 2.0 ** -9 + 2.0 ** -12).float()
    bias = (torch.randn(N, generator=g) * 4).to(torch.bfloat16).double()      # exact in bf16; rounded to fp16 by the test where needed
    return rs, al, bias
