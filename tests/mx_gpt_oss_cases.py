"""Shared by tests/test_mx_gpt_oss_cpu.py and tests/test_gpu_mx_gpt_oss.py (a helper module, not a conftest): the float64 oracle of the
routed MX GEMM with the GPT-OSS epilogue (inc_mx_moe_gemm_glu, neural_compressor_amd/csrc/gemm_strip_moe.hip).  No GPU code.

The operands, routings and accumulators are those of tests/mx_moe_cases.py; this module adds the bias and the clamped SwiGLU.

Bias: b(e, n) = ((5 n + 3 e) % 17 - 8) / 4, multiples of 2^-2 in [-2, 2] that differ between experts and between the gate and the up
half.  With mx_moe_cases.exact_case operands acc + b stays exact in fp32 in all three modes (assert_exact_condition: the same units,
2^-4 in modes 2 / 1 and 2^-10 in mode 0, and the partial sums stay below the same tops with |b| added), so modes 2 and 1 are BIT-EQUAL
to the float64 result.

Mode 0: with g, u the exact sums plus bias and ref the float64 value of (clamp(u) + 1) * min(g, limit) * sigmoid(alpha min(g, limit)),

    |h - ref| <= u_out |ref| + (|alpha g| + 8) 2^-23 |ref| + tiny,        u_out, tiny = moe_stage_cases.out_rounding(dtype)

The first term is the one rounding to bf16 / fp16.  The second: alpha * g is one fp32 rounding, an absolute error of at most
2^-24 |alpha g| in the exponent, and the sigmoid's relative sensitivity to its argument is below 1 (d ln sigmoid(t) / dt = 1 -
sigmoid(t)), so that is 2^-24 |alpha g| relative; expf, the add, the divide, u + 1 (exact here: u is a multiple of 2^-10 below 2^14)
and the product are a few fp32 ulp, 8 2^-23 generously.  Comparable elements are those with alpha * g >= MODE0_MIN_ARG = -80: below
about -88.7 expf overflows and the fp32 expression is -0 (mx_moe_cases' docstring explains this for the SiLU cases), and those whose
value the 16-bit type can hold (1.01 |ref| < finfo.max / 2, as mx_moe_cases.mode0_gate; it binds with limit = +inf only).  The
comparable share must be at least 0.99 per case.
"""

import math

import torch

from tests import moe_stage_cases as S
from tests import mx_moe_cases as M

MODE0_MIN_ARG = -80.0
MIN_SHARE = 0.99
MIN_REGION = 0.01
REGION_CASES = ("kW", "kW_plus1", "ragged_e8")
# (name, alpha, limit): GPT-OSS's own, one where the clamps dominate, one without clamps
PARAMS = [("gpt_oss", 1.702, 7.0), ("tight", 1.0, 0.75), ("no_clamp", 1.702, math.inf)]
PARAM_IDS = [p[0] for p in PARAMS]
MUTATIONS_ALL_MODES = ("bias_expert_plus_1", "bias_halves_swapped")
MUTATIONS_MODE0 = ("no_lower_clamp_u", "g_clamped_both_sides", "u_not_plus_1", "alpha_1")
MUTATIONS_MODE1 = ("bias_after_weight",)


def tiny_gpt_oss(seed=0, dtype=torch.float32):
    """GptOssForCausalLM with the config of moe_models.tiny_gpt_oss_experts and 2 layers; every experts parameter initialised."""
    from transformers import GptOssConfig, GptOssForCausalLM

    torch.manual_seed(seed)
    cfg = GptOssConfig(vocab_size=128, hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                       num_key_value_heads=2, num_local_experts=4, num_experts_per_tok=2, head_dim=16, max_position_embeddings=128)
    m = GptOssForCausalLM(cfg).to(dtype).eval()
    with torch.no_grad():
        for _, mod in gpt_oss_experts_of(m):
            for name in ("gate_up_proj", "down_proj", "gate_up_proj_bias", "down_proj_bias"):
                p = getattr(mod, name)
                if not p.is_meta:
                    p.normal_(0.0, 0.05)
    return m


def gpt_oss_experts_of(model):
    from neural_compressor_amd.torch.utils.utility import is_gpt_oss_experts

    return [(n, m) for n, m in model.named_modules() if is_gpt_oss_experts(m)]


def bias_of(E, N):
    """[E, N] float64."""
    e, n = torch.arange(E)[:, None], torch.arange(N)[None, :]
    return ((5 * n + 3 * e) % 17 - 8).double() / 4


def experts_of_positions(ro):
    """[nvalid]: the expert whose range holds position p."""
    counts = torch.tensor([int(ro["offsets"][e + 1]) - int(ro["offsets"][e]) for e in range(ro["E"])])
    return torch.repeat_interleave(torch.arange(ro["E"]), counts)


def glu64(g, u, alpha, limit, mutate=None):
    """The clamped SwiGLU in float64 (transformers' GptOssExperts._apply_gate)."""
    g = g.clamp(min=-limit, max=limit) if mutate == "g_clamped_both_sides" else g.clamp(max=limit)
    u = u.clamp(max=limit) if mutate == "no_lower_clamp_u" else u.clamp(min=-limit, max=limit)
    a = 1.0 if mutate == "alpha_1" else alpha
    return (u if mutate == "u_not_plus_1" else u + 1.0) * (g / (1.0 + torch.exp(-(a * g))))


def biased(d, acc, mutate=None):
    """acc [nvalid, N] + b(e(p), n) in float64."""
    ro, N = d["ro"], d["N"]
    b = bias_of(ro["E"], N)
    e = experts_of_positions(ro)
    if mutate == "bias_expert_plus_1":
        e = (e + 1) % ro["E"]
    if mutate == "bias_halves_swapped":
        b = torch.cat([b[:, N // 2:], b[:, :N // 2]], 1)
    return acc + b[e]


def reference(d, alpha, limit, mutate=None, acc=None):
    """float64 over the valid positions: (accb [nvalid, N], out [nvalid, Nout]) of an mx_moe_cases case d (exact or random)."""
    key = ("glu_ref", alpha, limit, mutate)
    if acc is None and key in d:
        return d[key]
    base = M.reference(d)[0] if acc is None else acc
    ro, mode, N = d["ro"], d["mode"], d["N"]
    accb = biased(d, base, mutate)
    if mode == 0:
        out = glu64(accb[:, :N // 2], accb[:, N // 2:], alpha, limit, mutate)
    elif mode == 1:
        w = d["rw"].reshape(-1).double()[ro["order"].long()[:ro["nvalid"]]][:, None]
        out = w * base + biased(d, torch.zeros_like(base)) if mutate == "bias_after_weight" else w * accb
    else:
        out = accb
    if acc is None:
        d[key] = (accb, out)
    return accb, out


def assert_exact_condition(d):
    """mx_moe_cases.assert_exact_condition with the bias: b is a multiple of the unit, the partial sums stay below the same tops
    with |b| added, acc + b is an fp32 number, and so is the mode-1 product."""
    M.assert_exact_condition(d)
    acc, mass, _ = M.reference(d)
    if acc.numel() == 0:
        return
    unit, top = (2.0 ** 10, 2.0 ** 14) if d["mode"] == 0 else (2.0 ** 4, 2.0 ** 18)
    b = bias_of(d["ro"]["E"], d["N"])
    assert bool((b * unit == torch.round(b * unit)).all()) and float(b.abs().max()) <= 2.0
    assert float(mass.max()) + 2.0 < top
    accb, out = reference(d, 1.702, 7.0)
    assert bool((accb.float().double() == accb).all())
    if d["mode"] != 0:
        assert bool((out.float().double() == out).all())


def mode0_gate(g, u, alpha, limit, dtype, dg=None, du=None):
    """(ref, tol, comparable) of mode 0 from the float64 g, u (bias added); dg, du: what g and u may be off by (random operands)."""
    u_out, tiny = S.out_rounding(dtype)
    ref = glu64(g, u, alpha, limit)
    gc, uc = g.clamp(max=limit), u.clamp(min=-limit, max=limit)
    tol = u_out * ref.abs() + ((alpha * gc).abs() + 8.0) * 2.0 ** -23 * ref.abs() + tiny
    worst = ref.abs()
    if dg is not None:
        # |d (g sigmoid(alpha g)) / dg| <= 1.1 for every alpha > 0 (silu's derivative in t = alpha g), |g sigmoid| <= |g|; the clamps
        # are 1-Lipschitz: mode0_tolerance's two terms with u + 1 for u
        extra = 1.1 * dg * ((uc + 1.0).abs() + du) + gc.abs() * du
        tol, worst = tol + extra, worst + extra
    ok = (alpha * gc >= MODE0_MIN_ARG) & (1.01 * worst < float(torch.finfo(dtype).max) / 2)
    return ref, tol, ok


def exact_gate(d, alpha, limit, dtype):
    """(ref, tol, comparable, share) of mode 0 on exact operands."""
    accb, _ = reference(d, alpha, limit)
    I = d["N"] // 2
    ref, tol, ok = mode0_gate(accb[:, :I], accb[:, I:], alpha, limit, dtype)
    return ref, tol, ok, (float(ok.double().mean()) if ok.numel() else 1.0)


def region_shares(rule, limit):
    """Shares of g > limit, u > limit, u < -limit and inside over REGION_CASES' mode-0 elements, bias added."""
    gs, us = [], []
    for name in REGION_CASES:
        d = M.exact_case(M.case(name), 0, rule)
        accb, _ = reference(d, 1.702, limit)
        I = d["N"] // 2
        gs.append(accb[:, :I].reshape(-1))
        us.append(accb[:, I:].reshape(-1))
    g, u = torch.cat(gs), torch.cat(us)
    share = lambda m: float(m.double().mean())  # noqa: E731
    return dict(g_above=share(g > limit), u_above=share(u > limit), u_below=share(u < -limit),
                inside=share((g <= limit) & (u.abs() <= limit)))


def check_output(d, y, alpha, limit, dtype=None, mutate=None):
    """None if y [nvalid, Nout] (CPU) passes the case's gate against the reference (the mutated one when asked), else a message."""
    accb, out = reference(d, alpha, limit, mutate)
    if d["mode"] == 0:
        # the bound and the comparable set are the unmutated expression's: a mutation moves the reference only
        good, _ = reference(d, alpha, limit)
        I = d["N"] // 2
        _, tol, ok = mode0_gate(good[:, :I], good[:, I:], alpha, limit, dtype)
        err = (y.double() - out).abs()
        bad = ok & ~(err <= tol)
        if bool(bad.any()):
            i, j = bad.nonzero()[0].tolist()
            return (f"{int(bad.sum())} of {int(ok.sum())} outputs past the bound, first at [{i}, {j}]: got {float(y[i, j])!r}, "
                    f"reference {float(out[i, j])!r}, bound {float(tol[i, j])!r}")
        return None
    want = out.float()
    if not torch.equal(y.view(torch.int32), want.view(torch.int32)):
        bad = (y.view(torch.int32) != want.view(torch.int32)).nonzero()
        i, j = bad[0].tolist()
        return f"{bad.shape[0]} of {want.numel()} outputs differ, first at [{i}, {j}]: got {float(y[i, j])!r}, want {float(want[i, j])!r}"
    return None


def oracle_output(d, alpha, limit, dtype=None):
    """What a correct kernel returns on the valid positions: the reference rounded once (mode 0) or as it is in fp32."""
    _, out = reference(d, alpha, limit)
    return out.to(dtype) if d["mode"] == 0 else out.float()


def fp32_expression(d, alpha, limit):
    """Mode 0 as the header specifies it, evaluated in torch float32 on the CPU (before the rounding to 16 bits)."""
    acc = M.reference(d)[0].float()
    I = d["N"] // 2
    b = bias_of(d["ro"]["E"], d["N"]).float()[experts_of_positions(d["ro"])]
    g, u = acc[:, :I] + b[:, :I], acc[:, I:] + b[:, I:]
    g = torch.minimum(g, torch.tensor(limit, dtype=torch.float32))
    u = torch.clamp(u, min=-limit, max=limit)
    return (u + 1.0) * (g / (1.0 + torch.exp(-(torch.tensor(alpha, dtype=torch.float32) * g))))


def random_gate(d, alpha, limit, dtype=None):
    """(ref, tol, comparable) of an mx_moe_cases.random_case with the bias added: the chain bound of acc plus the one rounding of
    acc + b; mode 0 in the form of moe_stage_cases.mode0_tolerance with the GLU for silu64."""
    ro = d["ro"]
    accb = biased(d, d["acc"])
    dacc = d["dacc"] + 2.0 ** -24 * accb.abs()
    if d["mode"] == 0:
        I = d["N"] // 2
        return mode0_gate(accb[:, :I], accb[:, I:], alpha, limit, dtype, dacc[:, :I], dacc[:, I:])
    if d["mode"] == 1:
        w = d["rw"].reshape(-1).double()[ro["order"].long()[:ro["nvalid"]]][:, None]
        return w * accb, w.abs() * (dacc + 2.0 ** -23 * accb.abs()), torch.ones_like(accb, dtype=torch.bool)  # + the multiply's rounding
    return accb, dacc, torch.ones_like(accb, dtype=torch.bool)
