"""Shared by tests/test_mx_moe_cpu.py and tests/test_gpu_mx_moe.py (a helper module, not a conftest): the cases and the float64 oracle
of the routed MX GEMM of the fused MoE experts (inc_mx_moe_gemm, neural_compressor_amd/csrc/gemm_strip_moe.hip).  No GPU code.

Routings and the route oracle come from tests/moe_stage_cases.py, formats, the quantiser oracle and the bounds from tests/mx_cases.py.

Exact operands: values are integers in -3..3 and the scale bytes follow the two rule shapes of mx_cases.SCALE_RULES, the weight rule
taken at row n + 7 e so that experts differ in their scales too; the weight values of expert e come from their own seed, so reading
expert e +- 1 shows.
  modes 2 and 1   bytes 125..129: every product is a multiple of 2^-4 and every partial sum stays below 2^18, so acc is exact in fp32
                  in any order; the routing weights are powers of two (0.25 .. 2 by (37 slot % 101) % 4, so w[order[p]] and w[p]
                  differ), the one fp32 multiply is exact too: the output is BIT-EQUAL to the float64 result.
  mode 0          bytes 122..126 (the rules shifted down by 3): products are multiples of 2^-10 and partial sums stay below 2^14, so g
                  and u are exact and small enough that silu(g) u stays inside fp16:  |h - ref| <= u_out |ref| + 2^-20 |ref| + tiny
                  (moe_stage_cases.mode0_tolerance with dg = du = 0: the output rounding plus a few fp32 ulp for expf, the divide and
                  the product) on the elements with 1.01 |ref| < finfo(dtype).max / 2, whose share must be >= 0.99.
                  The expression is specified in fp32, g / (1.f + expf(-g)) * u, and fp32 has a range: expf(-g) overflows below
                  g = -88.7 (the expression is then -0 where silu(g) u may still be a bf16 number) and just above that the product
                  is an fp32 subnormal.  The gate has no term for that, so the operands keep away from it, as the scale bytes
                  keep away from fp16's overflow: the GATE rows of a mode-0 weight take their values from {-1, 0, 1} with two
                  zeros in three (the up rows and the activations keep -3..3), and every case asserts g >= MODE0_MIN_G = -80 on
                  the CPU: then |silu(g)| >= 2^-110 and |u| >= 2^-10 or u = 0, so every h is zero or an fp32 normal.
"""

import collections

import torch

from tests import moe_stage_cases as S
from tests import mx_cases as C

WAVES = 8                      # INC_MX_MOE_WAVES as built: the ways of the in-workgroup K split, in every mode
STRIP = 16                     # output columns of a workgroup
ROUTING_WEIGHTS = (0.25, 0.5, 1.0, 2.0)
MODE0_SHIFT = 3                # scale bytes 122..126 in mode 0
MIN_SHARE = 0.99
MODE0_MIN_G = -80.0            # the fp32 range condition of mode 0 (module docstring)

Case = collections.namedtuple("Case", "name routing modes Nout Kp pins")
CASES = [
    Case("one_tile_n4", "edges3", (2,), 4, 128, "one K-tile, N < 16 (clamped weight rows)"),
    Case("kW", "edges3", (2, 1, 0), 260, 128 * WAVES, "every wave exactly one K-tile, strip tail of 4 columns"),
    Case("kW_minus1", "edges3", (2,), 264, 128 * (WAVES - 1), "an idle wave"),
    Case("kW_plus1", "edges3", (2, 1, 0), 264, 128 * (WAVES + 1), "second round of one wave"),
    Case("ragged_e8", "edges", (1, 0), 264, 3328, "ragged last round, 16 / 17-row tiles, one-row tile, full 64-row tile"),
    Case("i7", "edges3", (0,), 7, 256, "I not a multiple of 4 (2-byte stores), up strip unaligned to 16"),
    Case("max_e", "max_experts", (2,), 20, 256, "E = 512 > S"),
    Case("spread", "spread", (0,), 36, 384, "128 experts x 4 rows: one row block per tile"),
    Case("many_rows", "many_rows", (1,), 24, 256, "961 / 959 rows: 15 full tiles + 1 row"),
    Case("one_slot", "one_slot", (2, 1, 0), 20, 256, "S = 1"),
    Case("short_waves", "short_waves", (2, 1, 0), 20, 256, "S = 17, k = 1"),
    Case("all_invalid", "all_invalid", (2, 1, 0), 20, 256, "no valid slot: nothing is written"),
]
CASE_MODES = [(c, m) for c in CASES for m in c.modes]
CASE_MODE_IDS = [f"{c.name}-mode{m}" for c, m in CASE_MODES]
RULES = list(C.SCALE_RULES)


def case(name):
    return next(c for c in CASES if c.name == name)


def routing_weights(T, k, dtype=torch.float32):
    """[T, k] from {0.25, 0.5, 1, 2} by (37 slot % 101) % 4: powers of two, exact in every dtype."""
    i = torch.arange(T * k)
    return torch.tensor(ROUTING_WEIGHTS, dtype=torch.float64)[((37 * i) % 101) % 4].to(dtype).view(T, k)


_routes = {}


def route_of(name):
    if name not in _routes:
        r = S.ROUTINGS[name]
        ro = S.route_oracle(S.top_k_index(r), r.E)
        assert ro["counts"] == r.counts
        _routes[name] = ro
    return _routes[name]


def _scaled(v, sb):
    """integer values [R, Kp] x 2^(byte - 127) per block -> float64."""
    R, Kp = v.shape
    s = torch.ldexp(torch.ones(sb.shape, dtype=torch.float64), sb.int() - 127)
    return (v.double().view(R, Kp // 32, 32) * s[:, :, None]).view(R, Kp)


_cases = {}


def exact_case(c, mode, rule):
    """Operands of case c in `mode` under scale rule `rule`, built once: a [T or S, Kp] int8 values, as_ bytes, w [E, N, Kp] int8,
    ws [E, N, Kp/32], rw [T, k] float64, the route oracle ro, and named [rows of a]: which source rows a valid position names."""
    key = (c.name, mode, rule)
    if key in _cases:
        return _cases[key]
    ro = route_of(c.routing)
    T, k, E, Sn = ro["T"], ro["k"], ro["E"], ro["S"]
    N = 2 * c.Nout if mode == 0 else c.Nout
    nb = c.Kp // 32
    shift = MODE0_SHIFT if mode == 0 else 0
    fa, fw = C.SCALE_RULES[rule]
    b = torch.arange(nb)[None, :]
    rows = Sn if mode == 1 else T
    g = torch.Generator().manual_seed(4242 + 31 * CASES.index(c) + mode)
    a = torch.randint(-3, 4, (rows, c.Kp), generator=g, dtype=torch.int8)
    as_ = (fa(torch.arange(rows)[:, None], b) - shift).to(torch.uint8)
    w = torch.empty((E, N, c.Kp), dtype=torch.int8)
    ws = torch.empty((E, N, nb), dtype=torch.uint8)
    for e in range(E):
        ge = torch.Generator().manual_seed(900001 + 7919 * e + 31 * CASES.index(c) + mode)   # expert-dependent: e +- 1 shows
        w[e] = torch.randint(-3, 4, (N, c.Kp), generator=ge, dtype=torch.int8)
        if mode == 0:                                                        # gate rows: {-1, 0, 1}, two zeros in three
            w[e, :N // 2] = (torch.randint(-1, 2, (N // 2, c.Kp), generator=ge, dtype=torch.int8)
                             * torch.randint(0, 2, (N // 2, c.Kp), generator=ge, dtype=torch.int8))
        ws[e] = (fw(torch.arange(N)[:, None] + 7 * e, b) - shift).to(torch.uint8)
    order = ro["order"].long()[:ro["nvalid"]]
    named = torch.zeros(rows, dtype=torch.bool)
    named[torch.arange(ro["nvalid"]) if mode == 1 else order // k] = True
    d = dict(case=c, mode=mode, rule=rule, ro=ro, N=N, a=a, as_=as_, w=w, ws=ws, rw=routing_weights(T, k, torch.float64), named=named,
             ad=_scaled(a, as_))
    _cases[key] = d
    return d


MUTATIONS = ("expert_plus_1", "halves_swapped", "scale_of_next_block", "weight_by_position")


def dense64(d, e, mutate=None):
    """Expert e's weight [N, Kp] in float64 (the CPU self-test asks for mutated weights)."""
    E, N = d["w"].shape[:2]
    if mutate == "expert_plus_1":
        e = (e + 1) % E
    w, ws = d["w"][e], d["ws"][e]
    if mutate == "scale_of_next_block":
        ws = torch.roll(ws, -1, dims=1)
    wd = _scaled(w, ws)
    if mutate == "halves_swapped":
        wd = torch.cat([wd[N // 2:], wd[:N // 2]])
    return wd


def reference(d, mutate=None):
    """float64 over the valid positions: (acc [nvalid, N], mass [nvalid, N], out [nvalid, Nout]).  out is acc (mode 2),
    w[order[p]] acc (mode 1) or silu(g) u (mode 0)."""
    key = ("ref", mutate)
    if key in d:
        return d[key]
    ro, mode, N = d["ro"], d["mode"], d["N"]
    nvalid, order, k = ro["nvalid"], ro["order"].long(), ro["k"]
    acc = torch.zeros(nvalid, N, dtype=torch.float64)
    mass = torch.zeros(nvalid, N, dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo == hi:
            continue
        rows = d["ad"][lo:hi] if mode == 1 else d["ad"][order[lo:hi] // k]
        wd = dense64(d, e, mutate)
        acc[lo:hi], mass[lo:hi] = rows @ wd.T, rows.abs() @ wd.abs().T
    if mode == 0:
        out = S.silu64(acc[:, :N // 2]) * acc[:, N // 2:]
    elif mode == 1:
        by = torch.arange(nvalid) if mutate == "weight_by_position" else order[:nvalid]
        out = d["rw"].reshape(-1)[by][:, None] * acc
    else:
        out = acc
    d[key] = (acc, mass, out)
    return d[key]


def assert_exact_condition(d):
    """modes 2 / 1: products are multiples of 2^-4, partial sums below 2^18 (22 bits: exact in fp32 in any order), times a power of two
    of at most 2.  mode 0: multiples of 2^-10 below 2^14 (24 bits)."""
    acc, mass, out = reference(d)
    lo, hi, unit, top = (122, 126, 2.0 ** 10, 2.0 ** 14) if d["mode"] == 0 else (125, 129, 2.0 ** 4, 2.0 ** 18)
    for sb in (d["as_"], d["ws"]):
        assert int(sb.min()) >= lo and int(sb.max()) <= hi
    if acc.numel() == 0:
        return
    assert float(mass.max()) < top
    assert bool((acc * unit == torch.round(acc * unit)).all()) and bool((acc.float().double() == acc).all())
    if d["mode"] == 0:
        assert float(acc[:, :d["N"] // 2].min()) >= MODE0_MIN_G, float(acc[:, :d["N"] // 2].min())
    if d["mode"] == 1:
        assert float(d["rw"].max()) <= 2.0 and bool((torch.frexp(d["rw"])[0] == 0.5).all())
        assert bool((out.float().double() == out).all())


def mode0_gate(d, dtype):
    """(ref, tol, comparable, share) of mode 0 on exact operands."""
    acc, _, _ = reference(d)
    I = d["N"] // 2
    zero = torch.zeros(())
    ref, tol = S.mode0_tolerance(acc[:, :I], acc[:, I:], zero, zero, dtype)
    ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
    share = float(ok.double().mean()) if ok.numel() else 1.0
    return ref, tol, ok, share


def check_output(d, y, dtype=None, mutate=None):
    """None if y [nvalid, Nout] (CPU) passes the case's gate against the reference (of the mutated weights when asked), else a message."""
    acc, _, out = reference(d, mutate)
    if d["mode"] == 0:
        I = d["N"] // 2
        zero = torch.zeros(())
        ref, tol = S.mode0_tolerance(acc[:, :I], acc[:, I:], zero, zero, dtype)
        ok = 1.01 * ref.abs() < float(torch.finfo(dtype).max) / 2
        err = (y.double() - ref).abs()
        bad = ok & ~(err <= tol)
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


def stored_operands(d, afmt, wfmt, poison=True):
    """(aq, as_, wq, ws) as inc_mx_quant stores them (CPU uint8).  poison: rows of a that no valid position names hold 0xFF codes and
    0xFF scale bytes."""
    E, N, Kp = d["w"].shape
    aq = C.stored(C.encode_values(d["a"], afmt), afmt).clone()
    as_ = d["as_"].clone()
    if poison:
        aq[~d["named"]] = 0xFF
        as_[~d["named"]] = 0xFF
    wq = C.stored(C.encode_values(d["w"].view(E * N, Kp), wfmt), wfmt).view(E, N, -1)
    return aq, as_, wq, d["ws"].clone()


# ---- random operands ---------------------------------------------------------------------------------------------------------------
_random = {}


def random_case(mode, afmt, wfmt, routing="edges3", Nout=260, K=600):
    """Gaussian rows through the oracle quantiser (mx_cases.random_operands per expert; the activations are those of expert 0's draw)."""
    key = (mode, afmt, wfmt, routing, Nout, K)
    if key in _random:
        return _random[key]
    ro = route_of(routing)
    N = 2 * Nout if mode == 0 else Nout
    rows = ro["S"] if mode == 1 else ro["T"]
    per = [C.random_operands(rows if e == 0 else 1, N, K, afmt, wfmt, seed=500 + 10 * mode + e) for e in range(ro["E"])]
    Kp = per[0]["xs"].shape[1] * 32
    d = dict(mode=mode, ro=ro, N=N, Kp=Kp, aq=C.stored(per[0]["xq"], afmt), as_=per[0]["xs"], ad=per[0]["xd"],
             wq=torch.stack([C.stored(p["wq"], wfmt) for p in per]), ws=torch.stack([p["ws"] for p in per]),
             wd=[p["wd"] for p in per], rw=S.make_routing_weights(ro["T"], ro["k"]))
    nvalid, order, k = ro["nvalid"], ro["order"].long(), ro["k"]
    acc = torch.zeros(nvalid, N, dtype=torch.float64)
    mass = torch.zeros(nvalid, N, dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo < hi:
            r = d["ad"][lo:hi] if mode == 1 else d["ad"][order[lo:hi] // k]
            acc[lo:hi], mass[lo:hi] = r @ d["wd"][e].T, r.abs() @ d["wd"][e].abs().T
    d["acc"], d["dacc"] = acc, Kp * 2.0 ** -23 * mass       # an fp32 chain of Kp terms in any order (mx_cases.chain_bound)
    _random[key] = d
    return d


def random_gate(d, dtype=None):
    """(ref, tol, comparable) of a random case: modes 2 / 1 |w| Kp 2^-23 mass with no output rounding; mode 0 mode0_tolerance(g, u,
    dg, du, dtype) on the outputs the type can hold."""
    acc, dacc, ro = d["acc"], d["dacc"], d["ro"]
    if d["mode"] == 0:
        I = d["N"] // 2
        ref, tol = S.mode0_tolerance(acc[:, :I], acc[:, I:], dacc[:, :I], dacc[:, I:], dtype)
        return ref, tol, ref.abs() + tol < float(torch.finfo(dtype).max) / 2
    if d["mode"] == 1:
        w = d["rw"].reshape(-1).double()[ro["order"].long()[:ro["nvalid"]]][:, None]
        return w * acc, w.abs() * dacc, torch.ones_like(acc, dtype=torch.bool)
    return acc, dacc, torch.ones_like(acc, dtype=torch.bool)

