"""The CPU oracle of the MX (OCP microscaling) cell and the cases of tests/test_mx_cpu.py and tests/test_gpu_mx.py.  No GPU code.

The specification is the comment of inc_mx_quant / inc_mx_gemm in include/inc_mi355x.h.  The oracle works in float64 with frexp and
torch.round (half to even) -- nothing of the kernel's bit arithmetic -- and runs on whatever device its inputs live on.

  quant_mx(x, fmt, Kp)        -> (codes uint8 [M,Kp], one code per element, NOT packed; scale bytes uint8 [M,Kp/32])
  pack_fp4(codes)             -> [M,Kp/2], element 2i in the low nibble
  stored(codes, fmt)          -> the codes as inc_mx_quant stores them (fp8: as they are, fp4: packed)
  dequant_mx(codes, scales, fmt) -> float64 [M,Kp] (codes unpacked)
  FakeQuantLinear             -> y = dequant(quant(x)) @ dequant(quant(W))^T + bias in the dtype it is given, for the model test
"""

from collections import namedtuple

import torch

FP8, FP4 = 0, 4                      # the instruction's format codes (INC_MX_FP8_E4M3, INC_MX_FP4_E2M1)
FMT_IDS = {FP8: "fp8", FP4: "fp4"}
FMT_NAMES = {FP8: "fp8_e4m3", FP4: "fp4"}
PAIRS = [(FP8, FP8), (FP8, FP4), (FP4, FP4)]          # (activation, weight)
PAIR_IDS = ["a8w8", "a8w4", "a4w4"]
KTILE = 128
TILE = 256                           # the GEMM's tile edge along M and along N
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]

# emax of the scale rule, mantissa bits, exponent of the smallest normal, exponent bias, largest magnitude
_F = {FP8: dict(emax=8, mb=3, emin=-6, bias=7, sat=448.0, sign=0x80), FP4: dict(emax=2, mb=1, emin=0, bias=1, sat=6.0, sign=0x8)}
FP4_GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
FP4_TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0]
FP4_TIES_TO = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0]
# e4m3 midpoints (and the saturation band) with the grid value each goes to: ties to the even code
FP8_TIES = [2.0 ** -10, 3 * 2.0 ** -10, 1.0625, 1.1875, 17.0, 19.0, 232.0, 248.0, 432.0, 464.0, 500.0]
FP8_TIES_TO = [0.0, 2.0 ** -8, 1.0, 1.25, 16.0, 20.0, 224.0, 256.0, 448.0, 448.0, 448.0]


def padded_k(K):
    return (K + KTILE - 1) // KTILE * KTILE


def _floor_log2(a):
    """floor(log2(a)) of a positive float64 tensor, exactly (frexp: a = m * 2^e with m in [0.5, 1))."""
    return torch.frexp(a)[1] - 1


def scale_bytes(x, fmt, Kp):
    """[M, Kp/32] uint8: clamp(expfield(max |x| of the block as fp32) - emax, 0, 254)."""
    M, K = x.shape
    xp = torch.zeros((M, Kp), dtype=torch.float32, device=x.device)
    xp[:, :K] = x.to(torch.float32)
    amax = xp.view(M, Kp // 32, 32).abs().amax(dim=2)
    expfield = (amax.view(torch.int32) >> 23) & 0xFF
    return (expfield - _F[fmt]["emax"]).clamp(0, 254).to(torch.uint8)


def round_to_format(v, fmt):
    """float64 v -> (the nearest grid value of the element format, ties to even, saturating; its code without the sign)."""
    f = _F[fmt]
    a = v.abs().clamp(max=f["sat"])
    e = torch.where(a > 0, _floor_log2(torch.where(a > 0, a, torch.ones_like(a))), torch.full_like(a, f["emin"], dtype=torch.int32))
    e = e.clamp(min=f["emin"])
    step = torch.ldexp(torch.ones_like(a), e - f["mb"])
    q = torch.round(a / step) * step                                   # exact: a / step is a float64 with few bits
    normal = q >= 2.0 ** f["emin"]
    e2 = _floor_log2(torch.where(normal, q, torch.ones_like(q)))
    mant = torch.round((q / torch.ldexp(torch.ones_like(q), e2) - 1.0) * (1 << f["mb"])).to(torch.int32)
    code_n = ((e2 + f["bias"]) << f["mb"]) | mant
    code_s = torch.round(q * 2.0 ** (f["mb"] - f["emin"])).to(torch.int32)   # subnormals: multiples of 2^(emin - mb)
    return q, torch.where(normal, code_n, code_s)


def quant_mx(x, fmt, Kp=None):
    """The row quantiser of the specification.  x [M,K] of any float type."""
    M, K = x.shape
    Kp = padded_k(K) if Kp is None else Kp
    assert Kp % KTILE == 0 and Kp >= K
    sb = scale_bytes(x, fmt, Kp)
    xp = torch.zeros((M, Kp), dtype=torch.float64, device=x.device)
    xp[:, :K] = x.to(torch.float64)
    neg = torch.zeros((M, Kp), dtype=torch.bool, device=x.device)
    neg[:, :K] = torch.signbit(x)
    mult = torch.ldexp(torch.ones((M, Kp // 32), dtype=torch.float64, device=x.device), 127 - sb.to(torch.int32))
    v = (xp.view(M, Kp // 32, 32) * mult[:, :, None]).view(M, Kp)      # exact in float64
    _, code = round_to_format(v, fmt)
    code = code | (neg.to(torch.int32) * _F[fmt]["sign"])
    return code.to(torch.uint8), sb


def pack_fp4(codes):
    assert codes.shape[1] % 2 == 0 and int(codes.max()) < 16
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack_fp4(packed):
    out = torch.empty((packed.shape[0], packed.shape[1] * 2), dtype=torch.uint8, device=packed.device)
    out[:, 0::2] = packed & 0xF
    out[:, 1::2] = packed >> 4
    return out


def stored(codes, fmt):
    return codes.contiguous() if fmt == FP8 else pack_fp4(codes)


def code_table(fmt):
    """The value of every code, from the format's definition: (-1)^s * 2^(e - bias) * (1 + m / 2^mb), subnormals m * 2^(emin - mb)."""
    f = _F[fmt]
    n = 2 * f["sign"]
    t = []
    for c in range(n):
        mag = c & (f["sign"] - 1)
        e, m = mag >> f["mb"], mag & ((1 << f["mb"]) - 1)
        val = m * 2.0 ** (f["emin"] - f["mb"]) if e == 0 else 2.0 ** (e - f["bias"]) * (1 + m / (1 << f["mb"]))
        t.append(-val if c & f["sign"] else val)
    return torch.tensor(t, dtype=torch.float64)


def dequant_mx(codes, scales, fmt):
    """float64 [M,Kp]: table value * 2^(byte - 127).  (e4m3 code 0x7f / 0xff is NaN in the format; the quantiser never emits it.)"""
    M, Kp = codes.shape
    vals = code_table(fmt).to(codes.device)[codes.long()]
    s = torch.ldexp(torch.ones(scales.shape, dtype=torch.float64, device=codes.device), scales.to(torch.int32) - 127)
    return (vals.view(M, Kp // 32, 32) * s[:, :, None]).view(M, Kp)


def fake_quant(x, fmt):
    """dequant(quant(x)) cut back to x's columns, float64."""
    q, s = quant_mx(x, fmt)
    return dequant_mx(q, s, fmt)[:, :x.shape[1]]


class FakeQuantLinear(torch.nn.Module):
    """The float emulation of an MX linear (what the reference's MXLinear computes): both operands fake-quantised, the product in
    the module's float type.  Shares the quantisation error with the native module and differs in summation order and roundings."""

    def __init__(self, linear, w_fmt, act_fmt, dtype=torch.float32):
        super().__init__()
        self.act_fmt = act_fmt
        self.register_buffer("weight", fake_quant(linear.weight.detach(), w_fmt).to(dtype))
        self.register_buffer("bias", None if linear.bias is None else linear.bias.detach().to(dtype))

    def forward(self, x):
        x2 = fake_quant(x.reshape(-1, x.shape[-1]), self.act_fmt).to(self.weight.dtype)
        y = torch.nn.functional.linear(x2, self.weight, self.bias)
        return y.reshape(*x.shape[:-1], -1).to(x.dtype)


# ---- quantiser cases ------------------------------------------------------------------------------------------------------------------
# The kernel gives one lane one block, so it has no rows-held-in-registers limit; its paths are the 16-byte loads (K a multiple of 8,
# or of 4 for fp32, and an aligned x) against the element loads (any other K, or an unaligned x), and whole / partly padded / fully
# padded blocks.  Every row kind below is built per input type and format, so that it is finite and hits the intended boundary.
QCase = namedtuple("QCase", "name M K rows unaligned")
QCASES = [
    QCase("k32_plain", 1, 32, ["rand"], False),
    QCase("k32_specials", 5, 32, ["zero", "ties", "tiny", "max", "pow2"], False),
    QCase("k200_ragged", 5, 200, ["zero", "pow2", "below", "sat", "ties"], False),
    QCase("k200_unaligned", 3, 200, ["rand", "sat", "max"], True),
    QCase("k203_element_loads", 2, 203, ["rand", "below"], False),
    QCase("k204_fp32_vector_only", 2, 204, ["pow2", "rand"], False),
    QCase("k1024", 4, 1024, ["rand", "pow2", "below", "sat"], False),
    QCase("k1024_unaligned", 2, 1024, ["tiny", "ties"], True),
]
QCASE_IDS = [c.name for c in QCASES]


def ties_of(fmt):
    return (FP8_TIES, FP8_TIES_TO, 256.0) if fmt == FP8 else (FP4_TIES, FP4_TIES_TO, 7.0)


def _row(kind, K, dtype, fmt, g):
    """One row in fp32 whose values are exact in `dtype`."""
    fi = torch.finfo(dtype)
    nb = (K + 31) // 32
    u = torch.randint(-10, 11, (1,), generator=g).item()
    base = (torch.randn(nb * 32, generator=g) * 2.0 ** u).to(dtype).float()
    r = base.view(nb, 32).clone()
    if kind == "rand":
        r[nb // 2, 3] = -0.0
    elif kind == "zero":            # an all-zero block with one negative zero, among ordinary blocks
        r[0] = 0.0
        r[0, 5] = -0.0
    elif kind in ("pow2", "below", "sat"):
        for b in range(nb):
            j = (3 * b) % 21 - 10
            top = {"pow2": 1.0, "below": 1.0 - fi.eps / 2, "sat": 1.99}[kind] * 2.0 ** j
            blk = (torch.rand(32, generator=g) * 1.8 - 0.9) * 2.0 ** j
            blk[b % 32] = top if b % 2 == 0 else -top
            r[b] = blk.to(dtype).float()
    elif kind == "ties":            # the block's largest value puts its scale at 2^0, so the codes are those of the values
        ties, _, anchor = ties_of(fmt)
        vals = [anchor, -0.0, 0.0] + ties + [-t for t in ties]
        for b in range(nb):
            r[b] = 0.0
            r[b, :len(vals)] = torch.tensor(vals)
    elif kind == "tiny":            # subnormals of the input type (fp32 / bf16: scale byte 0)
        r[0] = (torch.arange(-16, 16).double() * (fi.tiny * fi.eps)).float()
        r[0, 0] = -0.0
    elif kind == "max":
        r[0, 7] = fi.max
        r[-1, 0] = -fi.max
    else:
        raise KeyError(kind)
    out = r.reshape(-1)[:K].to(dtype)
    assert bool(torch.isfinite(out.float()).all())
    return out


_inputs = {}


def quant_inputs(c, dtype, fmt):
    key = (c.name, dtype, fmt)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 + QCASES.index(c) * 10 + fmt)
        _inputs[key] = torch.stack([_row(kind, c.K, dtype, fmt, g) for kind in c.rows])
    return _inputs[key]


# ---- GEMM cases -----------------------------------------------------------------------------------------------------------------------
# Per tile edge of the kernel as built (256 x 256 x 128): M and N at 1, tile - 1, tile, tile + 1; N no multiple of 4; a y that is not
# 8-byte aligned; one, two and an odd number of K-tiles; the largest about 2 x tile rows.
GCase = namedtuple("GCase", "name M N Kp y_misaligned")
GCASES = [
    GCase("m1_n1_k1tile", 1, 1, 128, False),
    GCase("tile_exact", TILE, TILE, 128, False),
    GCase("m255_n257_k2tiles", TILE - 1, TILE + 1, 256, False),
    GCase("m257_n255_k3tiles", TILE + 1, TILE - 1, 384, False),
    GCase("m33_n260_k5tiles_y_unaligned", 33, 260, 640, True),
    GCase("m16_n512_k8tiles", 16, 2 * TILE, 1024, False),
    GCase("m300_n516_k8tiles", 300, 516, 1024, False),
    GCase("m513_n300_k2tiles", 2 * TILE + 1, 300, 256, False),
]
GCASE_IDS = [c.name for c in GCASES]
# scale rules: the first is the one the cell was specified with ((3 row + 5 block) % 5 -- which does not move with the block, 5 block
# being 0 mod 5); the second moves with the block too and differs between the operands, so a scale taken from the wrong block shows.
SCALE_RULES = {
    "issue": (lambda r, b: 125 + (3 * r + 5 * b) % 5, lambda r, b: 125 + (3 * r + 5 * b) % 5),
    "block": (lambda r, b: 125 + (3 * r + 7 * b) % 5, lambda r, b: 125 + (2 * r + 3 * b + 1) % 5),
}
_VALUE_CODE = {FP8: {0: 0x00, 1: 0x38, 2: 0x40, 3: 0x44}, FP4: {0: 0, 1: 2, 2: 4, 3: 5}}


def encode_values(v, fmt):
    """integer values in {0, +-1, +-2, +-3} -> codes (unpacked)."""
    lut = torch.tensor([_VALUE_CODE[fmt][i] for i in range(4)], dtype=torch.uint8)
    return lut[v.abs().long()] | ((v < 0).to(torch.uint8) * _F[fmt]["sign"])


_exact = {}


def exact_operands(c, rule):
    """values x [M,Kp], w [N,Kp] (int), scale bytes xs [M,Kp/32], ws [N,Kp/32], bias [N] (multiples of 2^-4 up to 8) and the exact
    float64 result without / with bias.  Built once per (case, rule)."""
    key = (c.name, rule)
    if key not in _exact:
        g = torch.Generator().manual_seed(77 + GCASES.index(c))
        x = torch.randint(-3, 4, (c.M, c.Kp), generator=g)
        w = torch.randint(-3, 4, (c.N, c.Kp), generator=g)
        fx, fw = SCALE_RULES[rule]
        nb = c.Kp // 32
        b = torch.arange(nb)[None, :]
        xs = fx(torch.arange(c.M)[:, None], b).to(torch.uint8)
        ws = fw(torch.arange(c.N)[:, None], b).to(torch.uint8)
        bias = torch.randint(-128, 129, (c.N,), generator=g).double() / 16
        xd = (x.double().view(c.M, nb, 32) * torch.ldexp(torch.ones(c.M, nb, dtype=torch.float64), xs.int() - 127)[:, :, None]).view(c.M, c.Kp)
        wd = (w.double().view(c.N, nb, 32) * torch.ldexp(torch.ones(c.N, nb, dtype=torch.float64), ws.int() - 127)[:, :, None]).view(c.N, c.Kp)
        y = xd @ wd.T
        mass = xd.abs() @ wd.abs().T                   # bounds every partial sum of every output, in any order
        _exact[key] = dict(x=x, w=w, xs=xs, ws=ws, bias=bias, y=y, yb=y + bias[None, :], mass=mass, xd=xd, wd=wd)
    return _exact[key]


def assert_exact_condition(d):
    """Every product is an integer times 2^(sx + sw - 254) >= 2^-4 and every partial sum stays below 2^18: a multiple of 2^-4 with at
    most 22 bits, exact in fp32 in any order; adding the bias (a multiple of 2^-4, |b| <= 8) keeps it below 2^19."""
    assert int(d["xs"].min()) >= 125 and int(d["ws"].min()) >= 125 and int(d["xs"].max()) <= 129 and int(d["ws"].max()) <= 129
    assert float(d["mass"].max()) + 8 < 2.0 ** 18
    assert bool((d["y"] * 16 == torch.round(d["y"] * 16)).all()) and bool((d["bias"] * 16 == torch.round(d["bias"] * 16)).all())
    assert bool((d["y"].float().double() == d["y"]).all()) and bool((d["yb"].float().double() == d["yb"]).all())


def ulp_of(y64, dtype):
    """Spacing of `dtype` at |y64| (float64 tensor)."""
    mb, emin = (7, -126) if dtype is torch.bfloat16 else (10, -14)
    a = y64.abs()
    e = torch.where(a > 0, _floor_log2(torch.where(a > 0, a, torch.ones_like(a))), torch.full_like(a, emin, dtype=torch.int32)).clamp(min=emin)
    return torch.ldexp(torch.ones_like(a), e - mb)


def chain_bound(xd, wd, y64, dtype, bias=None):
    """|y - y64| <= Kp * 2^-23 * sum_k |a_k b_k| + ulp(y64): an fp32 accumulation chain of Kp terms in any order (each of the Kp - 1
    additions and the scaling of a product err by at most 2^-24 relative to a partial sum bounded by the absolute mass) plus one
    rounding to the output type.  The fp32 bias add is one more term of the chain; y64 then includes the bias."""
    terms, mass = xd.shape[1], xd.abs() @ wd.abs().T
    if bias is not None:
        terms, mass = terms + 1, mass + bias.abs()[None, :]
    return terms * 2.0 ** -23 * mass + ulp_of(y64, dtype)


def random_operands(M, N, K, afmt, wfmt, seed):
    """Gaussian rows with per-row magnitudes 2^-10 .. 2^10 through the oracle quantiser -> codes, scales and dequantised operands."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.ldexp(torch.ones(M, 1), torch.randint(-10, 11, (M, 1), generator=g))
    w = torch.randn(N, K, generator=g) * torch.ldexp(torch.ones(N, 1), torch.randint(-10, 11, (N, 1), generator=g))
    xq, xs = quant_mx(x, afmt)
    wq, ws = quant_mx(w, wfmt)
    return dict(xq=xq, xs=xs, wq=wq, ws=ws, xd=dequant_mx(xq, xs, afmt), wd=dequant_mx(wq, ws, wfmt))


# the exact-operand condition, asserted for every case this file defines (the expected results are shared with the tests)
for _c in GCASES:
    for _rule in SCALE_RULES:
        assert_exact_condition(exact_operands(_c, _rule))
