"""Shared by tests/test_fp8_moe_cpu.py and tests/test_gpu_fp8_moe.py (a helper module, not a conftest): the cases and the float64 oracle
of the routed FP8 GEMM of the fused MoE experts (inc_fp8_moe_gemm, neural_compressor_amd/csrc/gemm_strip_moe.hip).  No GPU code.

The case table and the routings are those of tests/mx_moe_cases.py (CASES, route_of) and tests/moe_stage_cases.py, the quantiser oracle,
the code table and the random codes those of tests/fp8_cases.py.

Exact operands: values are integers in -3..3 drawn with per-expert seeds as mx_moe_cases.exact_case draws them (the weight values of
expert e come from their own seed, so reading expert e +- 1 shows), and the two factors are powers of two that differ from row to row,
from column to column and from expert to expert:
  modes 2 and 1   a_scale[r] = 2^((3 r) % 5 - 3), alpha[e, n] = 2^((2 (n + 7 e) + 1) % 5 - 3).  acc is an integer below 2^17 (Kp <= 3328,
                  |a b| <= 9), f = a_scale alpha a power of two in 2^-6 .. 2^2 and the routing weight a power of two in 0.25 .. 2 (by
                  (37 slot % 101) % 4, so w[order[p]] and w[p] differ): every multiply is exact, the output is BIT-EQUAL to the float64
                  result.
  mode 0          both exponents shifted to ... - 6 (f in 2^-12 .. 2^-4), the GATE rows from {-1, 0, 1} with two zeros in three: g and
                  u are exact in fp32 and small enough that silu(g) u stays inside fp16, and g stays above MODE0_MIN_G = -80, the range
                  of the fp32 expression g / (1.f + expf(-g)) * u (mx_moe_cases' docstring has the reason):
                  |h - ref| <= mode0_tolerance(g, u, 0, 0, dtype) on the elements with 1.01 |ref| < finfo(dtype).max / 2, whose share must
                  be >= 0.99.  assert_exact_condition checks all of this on the CPU for every case.
"""

import torch

from tests import fp8_cases as F
from tests import moe_stage_cases as S
from tests import mx_moe_cases as M
from tests.mx_moe_cases import CASE_MODE_IDS, CASE_MODES, CASES, MIN_SHARE, MODE0_MIN_G, STRIP, WAVES, case, route_of, routing_weights  # noqa: F401

MODE0_SHIFT = 3                 # the factor exponents are ... - 6 in mode 0
PIPE = 2.0 ** -8                # per-term allowance for the instruction's internal sum ("MX experts numerics")
MUTATIONS = ("expert_plus_1", "halves_swapped", "weight_by_position", "row_scale_by_position", "alpha_of_next_expert",
             "alpha_of_previous_expert")

_cases = {}


def exact_case(c, mode):
    """Operands of case c in `mode`, built once: a [T or S, Kp] int8 values, rs fp32 [T or S], w [E, N, Kp] int8, al fp32 [E, N],
    rw [T, k] float64, the route oracle ro, and named [rows of a]: which source rows a valid position names."""
    key = (c.name, mode)
    if key in _cases:
        return _cases[key]
    ro = route_of(c.routing)
    T, k, E, Sn = ro["T"], ro["k"], ro["E"], ro["S"]
    N = 2 * c.Nout if mode == 0 else c.Nout
    shift = 3 + (MODE0_SHIFT if mode == 0 else 0)
    rows = Sn if mode == 1 else T
    g = torch.Generator().manual_seed(4242 + 31 * CASES.index(c) + mode)
    a = torch.randint(-3, 4, (rows, c.Kp), generator=g, dtype=torch.int8)
    rs = torch.ldexp(torch.ones(rows, dtype=torch.float64), (3 * torch.arange(rows)) % 5 - shift)
    w = torch.empty((E, N, c.Kp), dtype=torch.int8)
    al = torch.empty((E, N), dtype=torch.float64)
    for e in range(E):
        ge = torch.Generator().manual_seed(900001 + 7919 * e + 31 * CASES.index(c) + mode)   # expert-dependent: e +- 1 shows
        w[e] = torch.randint(-3, 4, (N, c.Kp), generator=ge, dtype=torch.int8)
        if mode == 0:                                                        # gate rows: {-1, 0, 1}, two zeros in three
            w[e, :N // 2] = (torch.randint(-1, 2, (N // 2, c.Kp), generator=ge, dtype=torch.int8)
                             * torch.randint(0, 2, (N // 2, c.Kp), generator=ge, dtype=torch.int8))
        al[e] = torch.ldexp(torch.ones(N, dtype=torch.float64), (2 * (torch.arange(N) + 7 * e) + 1) % 5 - shift)
    order = ro["order"].long()[:ro["nvalid"]]
    named = torch.zeros(rows, dtype=torch.bool)
    named[torch.arange(ro["nvalid"]) if mode == 1 else order // k] = True
    d = dict(case=c, mode=mode, ro=ro, N=N, a=a, rs=rs.float(), w=w, al=al.float(), rw=routing_weights(T, k, torch.float64), named=named)
    _cases[key] = d
    return d


def reference(d, mutate=None):
    """float64 over the valid positions: (val [nvalid, N] = f acc, mass [nvalid, N] = f sum |a b|, out [nvalid, Nout]).  out is val
    (mode 2), w[order[p]] val (mode 1) or silu(g) u (mode 0).  `mutate` names the wrong read of a kernel with that mistake."""
    key = ("ref", mutate)
    if key in d:
        return d[key]
    ro, mode, N = d["ro"], d["mode"], d["N"]
    nvalid, order, k, E = ro["nvalid"], ro["order"].long(), ro["k"], ro["E"]
    val = torch.zeros(nvalid, N, dtype=torch.float64)
    mass = torch.zeros(nvalid, N, dtype=torch.float64)
    a, rs = d["a"].double(), d["rs"].double()
    for e in range(E):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo == hi:
            continue
        src = torch.arange(lo, hi) if mode == 1 else order[lo:hi] // k
        srs = torch.arange(lo, hi) % rs.shape[0] if mutate == "row_scale_by_position" else src
        ew = (e + 1) % E if mutate == "expert_plus_1" else e
        ea = (e + 1) % E if mutate == "alpha_of_next_expert" else (e - 1) % E if mutate == "alpha_of_previous_expert" else e
        w, al = d["w"][ew].double(), d["al"][ea].double()
        if mutate == "halves_swapped":
            w, al = torch.cat([w[N // 2:], w[:N // 2]]), torch.cat([al[N // 2:], al[:N // 2]])
        f = rs[srs][:, None] * al[None, :]
        val[lo:hi], mass[lo:hi] = f * (a[src] @ w.T), f * (a[src].abs() @ w.abs().T)
    if mode == 0:
        out = S.silu64(val[:, :N // 2]) * val[:, N // 2:]
    elif mode == 1:
        by = torch.arange(nvalid) if mutate == "weight_by_position" else order[:nvalid]
        out = d["rw"].reshape(-1)[by][:, None] * val
    else:
        out = val
    d[key] = (val, mass, out)
    return d[key]


def assert_exact_condition(d):
    """The conditions of the module docstring, on the CPU.  -> the figures (min g, max |ref|, share per 16-bit type) in mode 0."""
    val, mass, out = reference(d)
    mode = d["mode"]
    lo, hi = (-12, -4) if mode == 0 else (-6, 2)
    for t in (d["rs"], d["al"]):
        assert bool((torch.frexp(t.double())[0] == 0.5).all())                       # powers of two
    if val.numel() == 0:
        return None
    fmin, fmax = float(d["rs"].min() * d["al"].min()), float(d["rs"].max() * d["al"].max())
    assert 2.0 ** lo <= fmin and fmax <= 2.0 ** hi, (fmin, fmax)
    assert float(mass.max()) < 2.0 ** 17 * fmax
    assert bool((val.float().double() == val).all())                                 # f acc is exact in fp32
    if mode == 1:
        assert float(d["rw"].max()) <= 2.0 and bool((torch.frexp(d["rw"])[0] == 0.5).all())
    if mode != 0:
        assert bool((out.float().double() == out).all())
        return None
    I = d["N"] // 2
    assert float(val[:, :I].min()) >= MODE0_MIN_G, float(val[:, :I].min())
    shares = {}
    for dtype in (torch.bfloat16, torch.float16):
        _, _, ok, share = mode0_gate(d, dtype)
        assert share >= MIN_SHARE, (d["case"].name, dtype, share)
        shares[dtype] = share
    return dict(min_g=float(val[:, :I].min()), max_ref=float(out.abs().max()), shares=shares)


def mode0_gate(d, dtype):
    """(ref, tol, comparable, share) of mode 0 on exact operands."""
    val, _, _ = reference(d)
    I = d["N"] // 2
    zero = torch.zeros(())
    ref, tol = S.mode0_tolerance(val[:, :I], val[:, I:], zero, zero, dtype)
    ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
    return ref, tol, ok, (float(ok.double().mean()) if ok.numel() else 1.0)


def check_output(d, y, dtype=None, mutate=None):
    """None if y [nvalid, Nout] (CPU) passes the case's gate against the reference (of the mutated read when asked), else a message."""
    val, _, out = reference(d, mutate)
    if d["mode"] == 0:
        I = d["N"] // 2
        zero = torch.zeros(())
        ref, tol = S.mode0_tolerance(val[:, :I], val[:, I:], zero, zero, dtype)
        ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
        bad = ok & ~((y.double() - ref).abs() <= tol)
        if bool(bad.any()):
            i, j = bad.nonzero()[0].tolist()
            return (f"{int(bad.sum())} of {int(ok.sum())} outputs past the bound, first at [{i}, {j}]: got {float(y[i, j])!r}, "
                    f"reference {float(ref[i, j])!r}, bound {float(tol[i, j])!r}")
        return None
    want = out.float()
    if not torch.equal(y.view(torch.int32), want.view(torch.int32)):
        bad = (y.view(torch.int32) != want.view(torch.int32)).nonzero()
        i, j = bad[0].tolist()
        return f"{bad.shape[0]} of {want.numel()} outputs differ, first at [{i}, {j}]: got {float(y[i, j])!r}, want {float(want[i, j])!r}"
    return None


def oracle_output(d, dtype=None):
    """What a correct kernel returns on the valid positions: the reference rounded once (mode 0) or as it is in fp32."""
    _, _, out = reference(d)
    return out.to(dtype) if d["mode"] == 0 else out.float()


def stored_operands(d, poison=True):
    """(aq uint8 [rows, Kp], a_scale fp32 [rows], wq uint8 [E, N, Kp], alpha fp32 [E, N]) on the CPU.  poison: rows of a that no valid
    position names hold code 0xFF (a NaN code) and an a_scale of NaN."""
    E, N, Kp = d["w"].shape
    aq = F.encode_values(d["a"], F.FP8).clone()
    rs = d["rs"].clone()
    if poison:
        aq[~d["named"]] = 0xFF
        rs[~d["named"]] = float("nan")
    return aq, rs, F.encode_values(d["w"].view(E * N, Kp), F.FP8).view(E, N, Kp).contiguous(), d["al"].clone()


# ---- random codes --------------------------------------------------------------------------------------------------------------------
_random = {}


def _draw(g, shape, small):
    """Uniform e4m3 bytes: every code with the two NaN codes moved down by one (fp8_cases.random_codes), or, `small`, magnitudes below
    1.0 only (codes 0x00 .. 0x37 with a random sign): sums of 640 such products stay in the tens."""
    if small:
        return (torch.randint(0, 0x38, shape, generator=g) | (torch.randint(0, 2, shape, generator=g) << 7)).to(torch.uint8)
    q = torch.randint(0, 256, shape, generator=g).to(torch.uint8)
    return torch.where((q & 0x7F) == 0x7F, q - 1, q)


def random_case(mode, routing="edges3", Nout=260, Kp=640, small=False, unit=False):
    """Random e4m3 codes per expert with unit factors (`unit`) or fp8_cases.gaussian_factors (the activation rows' from expert 0's
    draw, alpha from each expert's own) and moe_stage_cases.make_routing_weights -> operands and, over the valid positions in float64,
    val = f acc, mass = f sum |a b|, w (mode 1)."""
    key = (mode, routing, Nout, Kp, small, unit)
    if key in _random:
        return _random[key]
    ro = route_of(routing)
    E, T, k = ro["E"], ro["T"], ro["k"]
    N = 2 * Nout if mode == 0 else Nout
    rows = ro["S"] if mode == 1 else T
    g = torch.Generator().manual_seed(7100 + 10 * mode + small)
    aq, wq = _draw(g, (rows, Kp), small), _draw(g, (E, N, Kp), small)
    if unit:
        rs, al = torch.ones(rows), torch.ones(E, N)
    else:
        rs = F.gaussian_factors(rows, N, 7200 + mode)[0]
        al = torch.stack([F.gaussian_factors(1, N, 7300 + 10 * mode + e)[1] for e in range(E)])
    tab = F.code_table(F.FP8)
    ad = tab[aq.long()]
    assert bool(torch.isfinite(ad).all())
    nvalid, order = ro["nvalid"], ro["order"].long()
    val = torch.zeros(nvalid, N, dtype=torch.float64)
    mass = torch.zeros(nvalid, N, dtype=torch.float64)
    for e in range(E):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            src = torch.arange(lo, hi) if mode == 1 else order[lo:hi] // k
            wd = tab[wq[e].long()]
            f = rs.double()[src][:, None] * al[e].double()[None, :]
            val[lo:hi], mass[lo:hi] = f * (ad[src] @ wd.T), f * (ad[src].abs() @ wd.abs().T)
    d = dict(mode=mode, ro=ro, N=N, Kp=Kp, aq=aq, rs=rs, wq=wq, al=al, rw=S.make_routing_weights(T, k), val=val, mass=mass)
    _random[key] = d
    return d


def random_gate(d, dtype=None):
    """(ref, tol, comparable) of a random case.  The sum inside one instruction is not an fp32 chain: the allowance is PIPE = 2^-8 (half
    a unit in the last place of a product of two e4m3 elements) on every term, d = PIPE mass, plus three fp32 roundings of |ref| (the
    factor product and the one or two epilogue multiplies): modes 2 / 1 |w| d + 3 2^-24 |ref|; mode 0 mode0_tolerance(g, u, dg, du,
    dtype) with dg, du that allowance on g and u, on the outputs the type can hold."""
    val, ro = d["val"], d["ro"]
    dv = PIPE * d["mass"] + 3 * 2.0 ** -24 * val.abs()
    if d["mode"] == 0:
        I = d["N"] // 2
        ref, tol = S.mode0_tolerance(val[:, :I], val[:, I:], dv[:, :I], dv[:, I:], dtype)
        return ref, tol, ref.abs() + tol < float(torch.finfo(dtype).max) / 2
    if d["mode"] == 1:
        w = d["rw"].reshape(-1).double()[ro["order"].long()[:ro["nvalid"]]][:, None]
        return w * val, w.abs() * dv, torch.ones_like(val, dtype=torch.bool)
    return val, dv, torch.ones_like(val, dtype=torch.bool)


# ---- the float emulation of a converted experts module ---------------------------------------------------------------------------------
class FakeQuantExperts(torch.nn.Module):
    """The CPU float emulation of FP8Experts for the model records: both operands of both products through the oracle quantiser
    (fp8_cases.quant_rows / dequant), the products and the SiLU in fp32, per expert that was hit."""

    def __init__(self, module):
        super().__init__()
        self.dev = module.gate_up_proj.device
        self.E = module.gate_up_proj.shape[0]
        deq = lambda p: torch.stack([F.dequant(*F.quant_rows(p[e].detach().cpu()))[:, :p.shape[2]] for e in range(self.E)]).float()  # noqa: E731
        self.gu, self.dn = deq(module.gate_up_proj), deq(module.down_proj)

    @staticmethod
    def _q(a):
        return F.dequant(*F.quant_rows(a))[:, :a.shape[1]].float()

    def forward(self, hidden_states, top_k_index, top_k_weights):
        x = hidden_states.detach().cpu().reshape(-1, hidden_states.shape[-1])
        idx, wts = top_k_index.cpu(), top_k_weights.detach().cpu().float()
        out = torch.zeros(x.shape, dtype=torch.float32)
        for e in range(self.E):
            tok, slot = torch.where(idx == e)
            if tok.numel() == 0:
                continue
            gate, up = (self._q(x[tok]) @ self.gu[e].T).to(hidden_states.dtype).float().chunk(2, dim=-1)
            h = (torch.nn.functional.silu(gate) * up).to(hidden_states.dtype)
            y = self._q(h) @ self.dn[e].T
            out.index_add_(0, tok, y * wts[tok, slot, None])
        return out.to(hidden_states.dtype).reshape(hidden_states.shape).to(self.dev)
