"""-m gpu: the kernels of the HEADLINE configuration (Llama-2-7B shapes, 16 384-token staged launches, g128 sym,
block size 128) against the oracle -- not toy sizes, not properties.

What is compared (SURVEY.md 8(c) comparator, VERDICT r1 "next round" item 1):
  (a) inc_gptq_hessian_accum at K = 4096 / 11008, T = 16384 per launch (both TAIL variants, beta != 0 included) against
      `O.gptq_add_batch` (gptq.py:1111-1141) on the same bf16 activations: the FULL matrix, every 256x256 tile, with an
      fp64 X^T X as the referee for what "float noise" is at this T.
  (b) GPTQ.fasterquant (gptq.py:1143-1351) at 4096x4096, the N-stacked gate/up solve [22016, 4096] and 4096x11008,
      against `O.gptq_fasterquant` on sampled rows (the column loop is row-independent given Hinv, so the oracle can
      run a row subset of the very same problem in seconds).  With the oracle's Hinv injected: codes identical up to the
      first rounding TIE of a row (|w/scale| within float noise of a .5 boundary in the oracle's own trajectory),
      scales <= 1e-3 (in fact ~1e-6) on rows with identical codes; the mismatch counts are printed.  End to end (own
      factorisation) the same gate with its own budget.
  (c) inverse_cholesky_upper at K = 4096 / 11008 against the fp64 trio, next to the distance of the reference's own
      fp32 LAPACK trio to fp64.
  (d) the fused INT4 -> bf16 GEMM at the BASELINE shapes against `O.woq_linear` directly (sampled rows of x).
The oracle runs on the GPU box's host cores; shapes are chosen so that the whole file costs about a minute of CPU.
"""

import math

import numpy as np
import pytest
import torch

from oracle import woq_oracle as O

pytestmark = pytest.mark.gpu

GS = 128


def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


_CACHE = {}


def _calib(hip, K, T=16384, seed=1):
    """Synthetic calibration activations of SURVEY 8(d): N(0,1), 1 % outlier channels x20, bf16, [8, T/8, K]."""
    key = ("x", K, T, seed)
    if key not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.randn(8, T // 8, K, generator=g)
        x[..., :: 97] *= 20.0
        _CACHE[key] = x.to(torch.bfloat16)
    return _CACHE[key]


def _hessian_pair(hip, K):
    """(H from the HIP kernel [device, upper triangle valid], H from the oracle [CPU]) for one staged launch."""
    from neural_compressor_amd import ops

    key = ("H", K)
    if key not in _CACHE:
        x = _calib(hip, K)
        H = torch.zeros(K, K, device=hip)
        ops.gptq_hessian_accum(H, x.to(hip).reshape(-1, K), 0.0, 2.0 / 8)
        Ho, n = O.gptq_add_batch(torch.zeros(K, K), 0, x.float())
        assert n == 8
        _CACHE[key] = (H, Ho)
    return _CACHE[key]


def _ref_hinv(hip, K):
    """The reference's fp32 LAPACK trio (oracle) on the oracle's H: (Hinv_ref CPU, dead CPU)."""
    key = ("Hinv", K)
    if key not in _CACHE:
        _, Ho = _hessian_pair(hip, K)
        Hinv, dead = O.gptq_hinv(Ho, 0.01)
        _CACHE[key] = (Hinv.contiguous(), dead)
    return _CACHE[key]


def _per_tile_rel(A, B, tile=256):
    """max over the upper-triangular tiles of ||A_t - B_t|| / ||B_t|| (double precision on the device)."""
    K = A.shape[0]
    nt = -(-K // tile)
    worst, where = 0.0, None
    for i in range(nt):
        for j in range(i, nt):
            a = A[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile].double()
            b = B[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile].double()
            if i == j:
                a, b = torch.triu(a), torch.triu(b)
            r = float((a - b).norm() / b.norm().clamp_min(1e-30))
            if r > worst:
                worst, where = r, (i, j)
    return worst, where


# ---------------------------------------------------------------------------------------------------
# (a) Hessian syrk at the staged launch shape
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4096, 11008])
def test_hessian_staged_launch_vs_oracle_full_matrix(hip, K):
    H, Ho = _hessian_pair(hip, K)
    x = _calib(hip, K).to(hip).reshape(-1, K)
    H64 = (x.double().t() @ x.double()) * (2.0 / 8)  # referee: exact products, fp64 accumulation
    Hod = Ho.to(hip)
    iu = torch.triu_indices(K, K, device=hip)
    e_gpu = rel_fro(H[iu[0], iu[1]], H64[iu[0], iu[1]])
    e_cpu = rel_fro(Hod[iu[0], iu[1]], H64[iu[0], iu[1]])
    e_pair = rel_fro(H[iu[0], iu[1]], Hod[iu[0], iu[1]])
    t_gpu, w_gpu = _per_tile_rel(H, H64)
    t_cpu, _ = _per_tile_rel(Hod, H64)
    t_pair, w_pair = _per_tile_rel(H, Hod)
    print(f"\n[hessian K={K} T=16384] rel-Frobenius vs fp64: HIP {e_gpu:.2e}, oracle {e_cpu:.2e}; HIP vs oracle {e_pair:.2e}; "
          f"worst 256-tile: HIP {t_gpu:.2e} at {w_gpu}, oracle {t_cpu:.2e}; HIP vs oracle {t_pair:.2e} at {w_pair}")
    # full matrix and every tile: the HIP result is float noise away from the oracle's, and no farther from the exact
    # product than the oracle's own fp32 GEMM is (x2 slack: different summation trees)
    assert e_pair <= 2e-6
    assert e_gpu <= max(2e-6, 2 * e_cpu)
    assert t_pair <= 4e-6, f"tile {w_pair} differs"
    assert t_gpu <= max(4e-6, 2 * t_cpu)


def test_hessian_running_mean_and_token_tail(hip):
    """Two staged launches (beta != 0 epilogue) and a token count that is not a multiple of the 64-token step (TAIL
    variant) at K = 4096 against two oracle add_batch calls."""
    from neural_compressor_amd import ops

    K = 4096
    g = torch.Generator().manual_seed(11)
    xa = _calib(hip, K)                                   # 8 batches x 2048
    xb = torch.randn(5, 2043, K, generator=g).to(torch.bfloat16)  # 5 batches x 2043 -> 10215 tokens, 10215 % 64 = 39
    H = torch.zeros(K, K, device=hip)
    ops.gptq_hessian_accum(H, xa.to(hip).reshape(-1, K), 0.0, 2.0 / 8)
    ops.gptq_hessian_accum(H, xb.to(hip).reshape(-1, K), 8.0 / 13, 2.0 / 13)
    Ho, n = O.gptq_add_batch(torch.zeros(K, K), 0, xa.float())
    Ho, n = O.gptq_add_batch(Ho, n, xb.float())
    assert n == 13
    Hod = Ho.to(hip)
    iu = torch.triu_indices(K, K, device=hip)
    e = rel_fro(H[iu[0], iu[1]], Hod[iu[0], iu[1]])
    t, where = _per_tile_rel(H, Hod)
    print(f"\n[hessian K=4096 two launches, tail] HIP vs oracle {e:.2e}, worst tile {t:.2e} at {where}")
    assert e <= 2e-6 and t <= 4e-6


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("shapes,T", [((512, 1024, 768, 256), 1000), ((4096, 4096, 4096, 11008), 16384), ((2048,) * 8, 2048)])
def test_hessian_multi_launch_is_bit_identical_to_single_launches(hip, monkeypatch, shapes, T, split):
    """inc_gptq_hessian_accum_multi (all Hessians of one forward in ONE launch -- what the driver issues after every stacked
    calibration forward) computes every tile exactly as inc_gptq_hessian_accum does: same bits, beta != 0 included.  With the
    tail split (default: the tiles of the launch's last, partly filled round are cut into token ranges summed in order) the
    tiles of that round -- 74 of the 1354 of a Llama block's launch -- carry the rounding of two to four partial sums instead.
    The last case is the smallest with a split tail on 256 CUs: 8 x 36 = 288 tiles, 32 of them in the last round, two ranges each."""
    from neural_compressor_amd import ops

    monkeypatch.setattr(ops, "HESSIAN_TAIL_SPLIT", split)
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(T, K, generator=g).to(torch.bfloat16).to(hip) for K in shapes]
    single = [torch.full((K, K), 0.25, device=hip) for K in shapes]
    multi = [h.clone() for h in single]
    for h, x in zip(single, xs):
        ops.gptq_hessian_accum(h, x, 0.5, 0.125)
    assert ops.gptq_hessian_accum_multi([(h, x, 0.5, 0.125) for h, x in zip(multi, xs)])
    n_diff = 0
    for a, b, K in zip(single, multi, shapes):
        iu = torch.triu_indices(K, K, device=hip)
        av, bv = a[iu[0], iu[1]], b[iu[0], iu[1]]
        if not split:
            assert torch.equal(av, bv), K
        else:
            n_diff += int((av != bv).sum())
            # (a long fp32 sum against the sum of its three parts: 20 ulps on the diagonal at 16384 tokens; either is 1e-5 from fp64)
            assert float((av - bv).abs().max()) <= 5e-6 * float(av.abs().max()), K
    if split:  # at most one round's worth of tiles may differ at all (256 CUs x 256 x 256), and none where the library splits no tail
        cus = torch.cuda.get_device_properties(hip).multi_processor_count
        first = sum((-(-K // 256)) * (-(-K // 256) + 1) // 2 for K in shapes)  # 256 x 256 tiles of the upper triangles
        tail, steps = first % cus, -(-T // 64)
        has_tail = first > cus and 0 < tail and 2 * tail <= cus and min(4, cus // tail, steps // 16) >= 2
        assert n_diff <= 128 * 256 * 256 and (n_diff > 0) == has_tail
    # fp32 inputs are declined (nothing launched): the caller falls back to the exact-fp32 single launches
    assert not ops.gptq_hessian_accum_multi([(multi[0], xs[0].float(), 0.5, 0.125), (multi[0], xs[0].float(), 0.5, 0.125)])


# ---------------------------------------------------------------------------------------------------
# (c) inverse Cholesky factor
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4096, 11008])
def test_inverse_cholesky_upper_baseline_size_vs_fp64(hip, K):
    from neural_compressor_amd.torch.algorithms.weight_only.gptq import inverse_cholesky_upper

    _, Ho = _hessian_pair(hip, K)
    Hinv_ref, dead = _ref_hinv(hip, K)
    Hd_cpu, dead2 = O.gptq_damped(Ho, 0.01)  # the very matrix the oracle's trio factorises
    assert torch.equal(dead, dead2)
    Hd = Hd_cpu.to(hip)
    U = inverse_cholesky_upper(Hd)
    H64 = Hd.double()
    L = torch.linalg.cholesky(H64)
    U64 = torch.linalg.cholesky(torch.cholesky_inverse(L), upper=True)
    e_hip = rel_fro(U, U64)
    e_ref = rel_fro(Hinv_ref.to(hip), U64)
    # what the column loop consumes: the diagonal (divisor d) and the rows of the factor
    d_hip = float(((torch.diagonal(U).double() - torch.diagonal(U64)) / torch.diagonal(U64)).abs().max())
    d_ref = float(((torch.diagonal(Hinv_ref.to(hip)).double() - torch.diagonal(U64)) / torch.diagonal(U64)).abs().max())
    print(f"\n[inverse_cholesky_upper K={K}] rel-Frobenius vs fp64 trio: HIP {e_hip:.2e}, reference fp32 LAPACK trio {e_ref:.2e}; "
          f"worst relative diagonal error: HIP {d_hip:.2e}, reference {d_ref:.2e}")
    assert torch.equal(torch.triu(U), U), "the factor must be upper triangular"
    assert e_hip <= max(1e-5, 2 * e_ref)
    assert d_hip <= max(1e-5, 2 * d_ref)


# ---------------------------------------------------------------------------------------------------
# (b) fasterquant at the bench's shapes
# ---------------------------------------------------------------------------------------------------
def _first_mismatch_report(codes_gpu, ref, rows, sym, bits):
    """Per sampled row: position of the first code that differs from the oracle's and how far the oracle's own
    pre-rounding value was from a rounding boundary there (in quantisation steps)."""
    Q, scale, zero, Win = ref["Q"], ref["scale"], ref["zero"], ref["Win"]
    K = Q.shape[1]
    sc = scale.repeat_interleave(GS, 1)[:, :K]
    zp = zero.repeat_interleave(GS, 1)[:, :K]
    ref_codes = torch.round(Q / sc + zp).to(torch.int32)  # Q = sc * (q - zp) exactly -> recovers q
    assert int(ref_codes.min()) >= 0 and int(ref_codes.max()) <= 2**bits - 1
    got = codes_gpu[rows].cpu().to(torch.int32)
    neq = got != ref_codes
    total = int(neq.sum())
    bad_rows = torch.nonzero(neq.any(1)).flatten()
    tie_dist = []
    for r in bad_rows.tolist():
        c = int(torch.nonzero(neq[r]).flatten()[0])
        u = float(Win[r, c] / sc[r, c])
        tie_dist.append(abs((u - math.floor(u)) - 0.5))
        assert abs(int(got[r, c]) - int(ref_codes[r, c])) == 1, f"row {r} col {c}: codes {int(got[r, c])} vs {int(ref_codes[r, c])}"
    return dict(total=total, rows=len(bad_rows), frac=total / neq.numel(), tie=max(tie_dist) if tie_dist else 0.0,
                clean=~neq.any(1), ref_codes=ref_codes)


# budgets of the end-to-end run (own factorisation) = 2 x measured (profiles/r5/parity_report.txt; the same on both kinds of pool host):
# (differing rows, differing-code fraction); measured 2 rows / 1.45e-4, 3 / 1.10e-4, 18 / 3.67e-3, ties <= 3.3e-6 steps
OWN_FACTOR_BUDGET = {"o_proj 4096x4096": (4, 3.0e-4), "gate+up stacked 22016x4096": (6, 2.5e-4), "down_proj 4096x11008": (36, 7.5e-3)}


@pytest.mark.parametrize("name,N,K,nsample", [("o_proj 4096x4096", 4096, 4096, 384), ("gate+up stacked 22016x4096", 22016, 4096, 384),
                                              ("down_proj 4096x11008", 4096, 11008, 256)])
def test_fasterquant_baseline_shapes_vs_oracle(hip, name, N, K, nsample):
    from neural_compressor_amd.torch.algorithms.weight_only.gptq import GPTQ, HessianAccumulator

    H_dev, Ho = _hessian_pair(hip, K)
    Hinv_ref, dead = _ref_hinv(hip, K)
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    rows = torch.sort(torch.randperm(N, generator=g)[:nsample])[0]
    rows[0], rows[-1] = 0, N - 1
    ref = O.gptq_fasterquant(W[rows].float(), Ho, bits=4, sym=True, blocksize=128, percdamp=0.01, groupsize=GS, Hinv=Hinv_ref, trace=True)

    layer = torch.nn.Linear(K, N, bias=False, device=hip, dtype=torch.bfloat16)
    layer.weight.data.copy_(W.to(hip))

    def run(inject):
        acc = HessianAccumulator(K, hip)
        acc.H = Ho.to(hip).clone()  # the oracle's H: isolates the solve from the (separately tested) syrk
        acc._n = 8
        if inject:
            acc.finalized = ((0.01, False), Hinv_ref.to(hip), dead.to(torch.uint8).to(hip), None)
        gq = GPTQ(layer, device=hip, accumulator=acc)
        gq.configure(dict(bits=4, sym=True, dtype="int", mse=False))
        scale, _, zero, Q = gq.fasterquant(layer.weight.data.clone(), blocksize=128, percdamp=0.01, groupsize=GS)
        return gq.codes, scale, Q

    # -- column loop in isolation: the oracle's Hinv injected -------------------------------------------
    codes, scale, Q = run(inject=True)
    rep = _first_mismatch_report(codes, ref, rows, True, 4)
    clean = rep["clean"]
    s_gpu, s_ref = scale[rows].cpu(), ref["scale"]
    s_rel = float(((s_gpu[clean] - s_ref[clean]).abs() / s_ref[clean]).max()) if bool(clean.any()) else 0.0
    print(f"\n[fasterquant {name}, injected Hinv] {nsample} sampled rows x {K} columns: {rep['total']} codes differ "
          f"({rep['frac']:.2e}) in {rep['rows']} rows; every first difference is a +-1 flip, largest distance of the oracle's own "
          f"value from the rounding boundary there {rep['tie']:.2e} steps; max scale rel diff on the {int(clean.sum())} identical rows {s_rel:.2e}")
    # measured: 0 codes differ at all three shapes, scales bit-identical.  Gate: at most two rows may flip at a tie closer than 1e-5
    # steps (the oracle's CPU GEMM order is the host's MKL's), nothing else
    assert rep["tie"] <= 1e-5, "a code differs where the oracle's value was not at a rounding tie"
    assert rep["rows"] <= 2 and rep["frac"] <= 5e-4
    assert s_rel <= 1e-6
    # the first reference block is untouched by any lazy update: bit-exact codes AND scales there, flips or not
    assert torch.equal(codes[rows][:, :128].cpu().to(torch.int32), rep["ref_codes"][:, :128])
    assert torch.equal(s_gpu[:, 0], s_ref[:, 0])
    # Q is scale * (code - 8) rounded once to the weight dtype
    grid = (codes.float() - 8.0) * scale.repeat_interleave(GS, dim=1)
    assert torch.equal(grid.to(torch.bfloat16), Q)

    # -- end to end: own blocked inverse-Cholesky factor instead of the LAPACK trio -----------------------
    codes2, scale2, _ = run(inject=False)
    rep2 = _first_mismatch_report(codes2, ref, rows, True, 4)
    clean2 = rep2["clean"]
    s2 = float(((scale2[rows].cpu()[clean2] - s_ref[clean2]).abs() / s_ref[clean2]).max()) if bool(clean2.any()) else 0.0
    print(f"[fasterquant {name}, own factorisation] {rep2['total']} codes differ ({rep2['frac']:.2e}) in {rep2['rows']} rows; "
          f"largest first-difference tie distance {rep2['tie']:.2e} steps; max scale rel diff on identical rows {s2:.2e}")
    if K == 11008:
        # the same rows with the factorisation's large products as exact-fp32 MFMA GEMMs instead of three-way bf16 splits (the default):
        # both factors are equally far from the fp64 one, so they flip DIFFERENT ties of the same kind -- reported side by side
        import neural_compressor_amd.torch.algorithms.weight_only.gptq as G

        G.CHOL_BF16X3 = False
        try:
            codes3, _, _ = run(inject=False)
        finally:
            G.CHOL_BF16X3 = True
        rep3 = _first_mismatch_report(codes3, ref, rows, True, 4)
        both = int((rep2["clean"] & rep3["clean"]).sum())
        print(f"[fasterquant {name}, own factorisation with exact-fp32 products] {rep3['total']} codes differ ({rep3['frac']:.2e}) in {rep3['rows']} rows, "
              f"largest tie distance {rep3['tie']:.2e} steps; rows identical to the oracle under BOTH factors: {both} of {nsample} "
              f"(split products alone: {int(rep2['clean'].sum())}, exact-fp32 products alone: {int(rep3['clean'].sum())})")
        assert rep3["tie"] <= 1e-5 and rep3["rows"] <= OWN_FACTOR_BUDGET[name][0] and rep3["frac"] <= OWN_FACTOR_BUDGET[name][1]
    max_rows, max_frac = OWN_FACTOR_BUDGET[name]
    assert rep2["tie"] <= 1e-5, "a code differs where the oracle's value was not at a rounding tie"
    assert rep2["rows"] <= max_rows and rep2["frac"] <= max_frac, (rep2["rows"], rep2["frac"])
    assert s2 <= 1e-5


# ---------------------------------------------------------------------------------------------------
# (d) fused GEMM against the oracle at the BASELINE shapes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 16, 64, 512, 4096])
@pytest.mark.parametrize("N,K", [(4096, 4096), (11008, 4096), (4096, 11008)])
def test_fused_gemm_baseline_shapes_vs_oracle(hip, M, N, K):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear
    from neural_compressor_amd.torch.algorithms.weight_only.utility import quant_tensor

    key = ("packed", N, K)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(N + 3 * K)
        w = (torch.randn(N, K, generator=g) * 0.02).to(hip)
        iw, sc, _ = quant_tensor(w, bits=4, group_size=GS, scheme="sym", return_int=True)
        m = MI355XWeightOnlyLinear(K, N, bits=4, group_size=GS, device=hip)
        m.pack(iw, sc, None, None)
        m.bias = None
        qw, scs, qz = m.qweight.cpu().numpy(), m.scales.cpu().numpy(), m.qzeros.cpu().numpy()
        _CACHE[key] = (m, qw, scs, qz, O.woq_dense_weight(qw, scs, qz, N, K, 4, GS, torch.bfloat16))
    m, qw, scs, qz, dense = _CACHE[key]
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    y = m(x.to(hip))
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    sel = torch.arange(M) if M <= 64 else torch.sort(torch.randperm(M, generator=g)[:48])[0]
    ref = O.woq_linear(x[sel], qw, scs, qz, None, N, K, 4, GS, compute_dtype=torch.bfloat16, dense=dense)
    got = y[sel.to(hip)].float().cpu()
    e_round = rel_fro(got, ref.to(torch.bfloat16).float())
    e_exact = rel_fro(got, ref)
    print(f"\n[fused gemm M={M} N={N} K={K}] vs oracle rounded to bf16 {e_round:.2e}, vs oracle fp32 {e_exact:.2e}")
    assert e_round <= 1e-3
    assert e_exact <= 4e-3  # bf16 output rounding alone is 2^-9 / sqrt(3) ~ 1.1e-3


# ---------------------------------------------------------------------------------------------------
# (e) AWQ grid searches at a BASELINE-size layer against the oracle
# ---------------------------------------------------------------------------------------------------
def test_awq_scale_and_clip_search_4096_vs_oracle(hip):
    """ActAwareWeightQuant.search_scale / apply_scale / search_clip (awq.py:264-361, 364-391, 393-470) on one
    self-absorbed 4096x4096 Linear, g128 asym, 8 x 256 calibration tokens, fp32: all 20 + 10 losses and both chosen grid
    points against `O.awq_search_scale_module` / `O.awq_search_clip_module` (pinned to the unmodified reference's own
    traces by tests/test_oracle_golden.py).  At this size one flipped rounding tie moves a loss by ~1e-7, so the loss
    curves must agree to float noise and the argmins exactly."""
    from neural_compressor_amd.torch.algorithms.weight_only.awq import ActAwareWeightQuant
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MulLinear

    N = K = 4096
    g = torch.Generator().manual_seed(5)
    W = torch.randn(N, K, generator=g) * 0.02
    xs = []
    for _ in range(8):
        x = torch.randn(1, 256, K, generator=g)
        x[..., ::53] *= 12.0  # salient channels: gives the alpha grid a real optimum
        xs.append(x)

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(K, N, bias=False)

        def forward(self, x):
            return self.lin(x)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = torch.nn.ModuleList([Block()])

        def forward(self, x):
            return self.blocks[0](x)

    model = Model()
    model.blocks[0].lin.weight.data.copy_(W)
    xd = [x.to(hip) for x in xs]
    awq = ActAwareWeightQuant(model, bits=4, group_size=GS, scheme="asym", total_block_args=[[x] for x in xd],
                              total_block_kwargs=[{} for _ in xd])
    name, tup = "blocks.0.lin", ("blocks.0.lin",)
    inputs = {"lin": {"input": xd}}
    with torch.no_grad():
        info = awq.search_scale(model.blocks[0], "blocks.0", [tup], inputs)
        awq.absorb_of = {tup: name}
        awq.apply_scale(info)
        assert isinstance(model.blocks[0].lin, MulLinear)
        awq.search_clip("blocks.0", [tup], inputs)
    s_hist, s_best = awq.search_log["scale"][name]
    c_hist, c_best = awq.search_log["clip"][name]

    r = O.awq_search_scale_module(W, None, xs, group_size=GS, scheme="asym")
    isc = 1.0 / r["best_scales"]
    c = O.awq_search_clip_module(W / isc.view(1, -1), None, xs, group_size=GS, scheme="asym", input_scale=isc)
    s_rel = float(np.max(np.abs(np.array(s_hist) - np.array(r["history"])) / np.array(r["history"])))
    c_rel = float(np.max(np.abs(np.array(c_hist) - np.array(c["history"])) / np.array(c["history"])))
    sr = np.sort(np.array(r["history"]))
    cr = np.sort(np.array(c["history"]))
    print(f"\n[awq 4096x4096 g128] scale search: chosen alpha index HIP {s_best} / oracle {r['best_index']}, max rel diff of the 20 losses "
          f"{s_rel:.2e} (oracle's best-to-runner-up gap {(sr[1] - sr[0]) / sr[0]:.2e}); clip search: index HIP {c_best} / oracle "
          f"{c['best_index']}, max rel diff of the 10 losses {c_rel:.2e} (gap {(cr[1] - cr[0]) / cr[0]:.2e})")
    assert s_best == r["best_index"] and c_best == c["best_index"]
    assert s_rel <= 1e-4 and c_rel <= 1e-4
    got = info[tup].float().cpu()
    assert float(((got - r["best_scales"]).abs() / r["best_scales"]).max()) <= 1e-5
