"""Shared by tests/test_fp8_group_cpu.py and tests/test_gpu_fp8_group.py (a helper module, not a conftest): the cases and the float64
oracle of the FP8 decode group launches (inc_fp8_gemv_multi, inc_fp8_gemv_gated, neural_compressor_amd/csrc/gemm_fp8_group.hip).  No
GPU code.

The code table, the random codes and the Gaussian factors of the multi launch are those of tests/fp8_cases.py; the small codes, the
silu and the mode-0 bound of the gated launch are those of tests/fp8_moe_cases.py and tests/moe_stage_cases.py.

Exact operands of the gated launch (gated_exact_case): x and the up weight are integers in -3..3, the GATE weight is from {-1, 0, 1}
with two zeros in three (fp8_moe_cases.exact_case's mode-0 draw), and every factor is a power of two that differs from row to row,
from column to column and between the two members:
  row_scale[m] = 2^((3 m) % 5 - 6),  alpha_gate[n] = 2^((2 n + 1) % 5 - 6),  alpha_up[n] = 2^((2 n + 3) % 5 - 6)
  bias_gate, bias_up: independent multiples of 2^-4 in -4 .. 4 (exact in bf16 and fp16)
so f = row_scale alpha is a power of two in 2^-12 .. 2^-4, f acc a multiple of 2^-12 and g = f acc + bias, u likewise, are exact in
fp32 with or without the contraction (asserted on the values), and g stays above MODE0_MIN_G = -80.  The bound is the mode-0 bound of
fp8_moe_cases.check_output, moe_stage_cases.mode0_tolerance(g, u, 0, 0, dtype) -- the output rounding plus the expf allowance -- on the
elements with 1.01 |ref| < finfo(dtype).max / 2.
"""

import torch

from tests import fp8_cases as F
from tests import fp8_moe_cases as M
from tests import moe_stage_cases as S
from tests.fp8_moe_cases import MIN_SHARE, MODE0_MIN_G  # noqa: F401

MAX_MEMBERS = 8
MULTI_NS = [4, 17, 260]          # below one strip; a last strip with one valid column and no vector store; several strips, ragged tail
MULTI_NS8 = [MULTI_NS[i % 3] for i in range(MAX_MEMBERS)]
MS = [1, 15, 16]
# Kp / 128: one tile (7 idle waves), a second round of one wave, 2 and 3 tiles for every wave (the `left == 2` and `left == 3` tails, no
# full round), full rounds of 4 plus one left over
TILES = [1, 9, 16, 24, 33]
GATED_MS = [1, 5, 16]
GATED_NS = [20, 7, 260]          # the experts case table's accepted widths (mx_moe_cases.CASES); 7 is no multiple of 16 (or of 4)
OUT_DTYPES = F.OUT_DTYPES
MUTATIONS = ("gate_up_swapped", "silu_on_up", "bias_of_the_other_member", "alpha_of_the_other_member", "row_scale_of_next_row")

assert set(GATED_NS) <= {c.Nout for c in M.CASES if 0 in c.modes}


# ---- multi: random codes, one x for every member ------------------------------------------------------------------------------------
_multi = {}


def multi_case(M_, Ns, Kp, seed=0):
    """xq [M, Kp] and, per member, wq [N_i, Kp] from fp8_cases.random_codes, row_scale / alpha_i / bias_i from fp8_cases.gaussian_factors;
    members with an odd index have no bias."""
    key = (M_, tuple(Ns), Kp, seed)
    if key not in _multi:
        base = 9100 + 1000 * seed + 31 * M_ + Kp
        xq = F.random_codes(M_, 4, Kp, base)["xq"]
        rs = F.gaussian_factors(M_, 4, base + 1)[0]
        wqs, als, biases = [], [], []
        for i, N in enumerate(Ns):
            wqs.append(F.random_codes(M_, N, Kp, base + 10 + i)["wq"])
            _, al, bias = F.gaussian_factors(M_, N, base + 50 + i)
            als.append(al)
            biases.append(bias if i % 2 == 0 else None)
        _multi[key] = dict(xq=xq, rs=rs, wqs=wqs, als=als, biases=biases)
    return _multi[key]


# ---- gated: the float64 oracle --------------------------------------------------------------------------------------------------------
def gated_reference(d, mutate=None):
    """float64 (g, u, h = silu(g) u) [M, N] of the operands d (x, wg, wu as values; rs, ag, au, bg, bu; a bias may be None).  `mutate`
    names the wrong read of a kernel with that mistake."""
    x, wg, wu = d["x"].double(), d["wg"].double(), d["wu"].double()
    rs, ag, au = d["rs"].double(), d["ag"].double(), d["au"].double()
    zero = torch.zeros(wg.shape[0], dtype=torch.float64)
    bg = zero if d["bg"] is None else d["bg"].double()
    bu = zero if d["bu"] is None else d["bu"].double()
    if mutate == "bias_of_the_other_member":
        bg, bu = bu, bg
    if mutate == "alpha_of_the_other_member":
        ag, au = au, ag
    if mutate == "row_scale_of_next_row":
        rs = rs[(torch.arange(rs.shape[0]) + 1) % rs.shape[0]]
    g = (rs[:, None] * ag[None, :]) * (x @ wg.T) + bg[None, :]
    u = (rs[:, None] * au[None, :]) * (x @ wu.T) + bu[None, :]
    if mutate == "gate_up_swapped":
        g, u = u, g
    if mutate == "silu_on_up":
        return g, u, g * S.silu64(u)
    assert mutate is None or mutate in MUTATIONS
    return g, u, S.silu64(g) * u


_gated = {}


def gated_exact_case(M_, N, Kp, bias="both"):
    """The exact operands of the module docstring, built once.  bias: "both", "gate" (up has none) or "none"."""
    key = (M_, N, Kp, bias)
    if key in _gated:
        return _gated[key]
    gen = torch.Generator().manual_seed(5300 + 131 * M_ + 17 * N + Kp)
    x = torch.randint(-3, 4, (M_, Kp), generator=gen, dtype=torch.int8)
    wu = torch.randint(-3, 4, (N, Kp), generator=gen, dtype=torch.int8)
    wg = (torch.randint(-1, 2, (N, Kp), generator=gen, dtype=torch.int8) * torch.randint(0, 2, (N, Kp), generator=gen, dtype=torch.int8))
    one_m, one_n = torch.ones(M_, dtype=torch.float64), torch.ones(N, dtype=torch.float64)
    rs = torch.ldexp(one_m, (3 * torch.arange(M_)) % 5 - 6)
    ag = torch.ldexp(one_n, (2 * torch.arange(N) + 1) % 5 - 6)
    au = torch.ldexp(one_n, (2 * torch.arange(N) + 3) % 5 - 6)
    bg = torch.randint(-64, 65, (N,), generator=gen).double() / 16
    bu = torch.randint(-64, 65, (N,), generator=gen).double() / 16
    d = dict(M=M_, N=N, Kp=Kp, x=x, wg=wg, wu=wu, rs=rs.float(), ag=ag.float(), au=au.float(),
             bg=bg if bias in ("both", "gate") else None, bu=bu if bias == "both" else None)
    _gated[key] = d
    return d


def assert_gated_exact_condition(d):
    """The conditions of the module docstring on the values -> (min g, share of comparable outputs per 16-bit type)."""
    g, u, _ = gated_reference(d)
    for t in (d["rs"], d["ag"], d["au"]):
        assert bool((torch.frexp(t.double())[0] == 0.5).all())                       # powers of two
    assert bool((d["ag"] != d["au"]).all())
    x, wg, wu = d["x"].double(), d["wg"].double(), d["wu"].double()
    assert float(max((x.abs() @ wg.abs().T).max(), (x.abs() @ wu.abs().T).max())) < 2.0 ** 17   # the sums are exact in any order
    for t in (g, u):
        assert bool((t.float().double() == t).all())                                 # f acc + bias is exact in fp32
    for b in (d["bg"], d["bu"]):
        assert b is None or all(bool((b.to(dt).double() == b).all()) for dt in OUT_DTYPES)
    assert float(g.min()) >= MODE0_MIN_G, float(g.min())
    shares = {}
    for dtype in OUT_DTYPES:
        ref, _ = S.mode0_tolerance(g, u, torch.zeros(()), torch.zeros(()), dtype)
        shares[dtype] = float((1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2).double().mean())
        assert shares[dtype] >= MIN_SHARE, (dtype, shares[dtype])
    return float(g.min()), shares


def gated_check(d, h, dtype, mutate=None):
    """None if h [M, N] (CPU) is within the mode-0 bound of the reference (of the mutated read when asked), else a message."""
    g, u, _ = gated_reference(d, mutate)
    if mutate == "silu_on_up":
        g, u = u, g                                       # the bound's formula is symmetric in which factor passes through silu
    zero = torch.zeros(())
    ref, tol = S.mode0_tolerance(g, u, zero, zero, dtype)
    ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
    bad = ok & ~((h.double() - ref).abs() <= tol)
    if bool(bad.any()):
        i, j = bad.nonzero()[0].tolist()
        return (f"{int(bad.sum())} of {int(ok.sum())} outputs past the bound, first at [{i}, {j}]: got {float(h[i, j])!r}, "
                f"reference {float(ref[i, j])!r}, bound {float(tol[i, j])!r}")
    return None


def gated_oracle_output(d, dtype, mutate=None):
    """What a kernel with that read returns: its float64 result rounded once."""
    return gated_reference(d, mutate)[2].to(dtype)


def gated_stored(d):
    """(xq, wq_gate, wq_up) uint8: the e4m3 codes of the exact case's values."""
    return F.encode_values(d["x"], F.FP8), F.encode_values(d["wg"], F.FP8), F.encode_values(d["wu"], F.FP8)


# ---- gated: random small codes against the experts kernel ----------------------------------------------------------------------------
_gated_random = {}


def gated_random_case(M_, N, Kp):
    """Random e4m3 codes of magnitude below 1.0 (fp8_moe_cases._draw, small) and Gaussian factors |N(0, 1)| / 2 + 1 / 4 -- no powers of
    two; sums of such products stay in the tens, so silu(g) u stays inside fp16 and above its subnormals (test_fp8_group_cpu.py
    asserts both on the float64 result) -> operands and the float64 (g, u)."""
    key = (M_, N, Kp)
    if key not in _gated_random:
        gen = torch.Generator().manual_seed(6400 + 131 * M_ + 17 * N + Kp)
        xq, wg, wu = M._draw(gen, (M_, Kp), True), M._draw(gen, (N, Kp), True), M._draw(gen, (N, Kp), True)
        f = lambda n: (torch.randn(n, generator=gen).abs() * 0.5 + 0.25).float()  # noqa: E731
        rs, ag, au = f(M_), f(N), f(N)
        tab = F.code_table(F.FP8)
        xd = tab[xq.long()]
        g = (rs.double()[:, None] * ag.double()[None, :]) * (xd @ tab[wg.long()].T)
        u = (rs.double()[:, None] * au.double()[None, :]) * (xd @ tab[wu.long()].T)
        _gated_random[key] = dict(xq=xq, wg=wg, wu=wu, rs=rs, ag=ag, au=au, g=g, u=u)
    return _gated_random[key]
