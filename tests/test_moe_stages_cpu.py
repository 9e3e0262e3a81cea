"""CPU: what tests/test_gpu_moe_stages.py relies on, without a GPU -- the K-slice count every GEMM case asserts (the workspace query is
host-only), the route buffer's layout, the routings' exact counts, and a self-test of the comparators: each of six mutations of a
correct result is rejected by the comparator meant to catch it.  No GPU call anywhere in this file."""

import itertools

import numpy as np
import pytest
import torch

from oracle import woq_oracle as O
from tests import moe_stage_cases as M


# ---- host-side plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,mode", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_case_splitk(c, mode):
    """Every case takes the K-slice count it was written for: (bytes - 4096) / (S N 4), or 0 bytes => 1.  A retuned moe_plan shows up
    here first: move the shape so that the branch keeps its case."""
    r = M.ROUTINGS[c.routing]
    S, N = r.T * r.k, M.n_of(c, mode)
    assert M.splitk_from_workspace(M.workspace_bytes(mode, r.T, r.k, r.E, N, c.K), S, N) == c.splitk
    assert M.plan_splitk(mode, S, r.E, N, c.K) == c.splitk


def test_cases_cover_every_branch():
    by = {c.name: c for c in M.CASES}
    assert len(by) == len(M.CASES) and all(c.pins for c in M.CASES)
    steps = {n: c.K // 32 for n, c in by.items()}
    assert steps["k32_n8"] == 1 and by["k32_n8"].Nout < M.MOE_BN                          # one-step K, Nout < 256
    assert by["k96_tail"].Nout % M.MOE_BN == 8 and steps["k96_tail"] == 3 and by["k96_tail"].splitk == 1  # strip tail, ragged chunk
    assert steps["k480_split"] - 4 * (by["k480_split"].splitk - 1) == 3                   # ragged last slice
    assert {by[n].group_size for n in ("k480_split", "k480_split_g1", "k640_g128", "k512_g64")} == {32, -1, 128, 64}
    assert by["gu_nibble4"].Nout % 8 == 4 and by["gu_onepass"].Nout % 8 == 4              # up-stream zero points at nibble 4
    assert steps["multi_chunk"] == 33 and by["multi_chunk"].splitk == 3                   # 12 + 12 + 9 steps
    r = M.ROUTINGS[by["units_512"].routing]
    assert -(-by["units_512"].Nout // M.MOE_BN) * M.tiles_max(r.T * r.k, r.E) >= 512 and steps["units_512"] > 4
    assert M.ROUTINGS[by["max_e"].routing].E == 512
    assert {m for c in M.CASES for m in c.modes} == {0, 1, 2}
    assert {c.splitk for c in M.CASES} == {1, 3, 4, 5}
    for n in ("k96_tail", "k480_split", "gu_nibble4"):                                   # ... and on the edges routing
        assert by[n + "_e8"].routing == "edges" and by[n + "_e8"][3:6] == by[n][3:6]


def test_route_bytes_match_the_layout():
    from neural_compressor_amd import _lib

    for T, k, E in itertools.product((1, 3, 17, 32, 64, 65, 960), (1, 2, 8), (1, 2, 8, 128, 512)):
        S = T * k
        L = M.route_layout(S, E)
        assert L.total == 1 + (E + 1) + 2 * S + 2 * (-(-S // 64) + min(E, S))
        assert _lib.lib.inc_moe_route_bytes(T, k, E) == 4 * L.total, (T, k, E)


def test_workspace_query_sweep():
    """The query never faults and returns 0 exactly when the plan is one pass, over small shapes (K < 128, N = 8, E > S)."""
    checked = 0
    for mode, T, k, E, N, K in itertools.product((0, 1, 2), (1, 3, 17, 64, 70, 256), (1, 2), (1, 3, 8, 512), (8, 16, 264, 520, 1024),
                                                 (32, 64, 96, 128, 480, 1056)):
        S = T * k
        sk = M.plan_splitk(mode, S, E, N, K)
        got = M.workspace_bytes(mode, T, k, E, N, K)
        assert got == (0 if sk == 1 else M.COUNTER_BYTES + sk * S * N * 4), (mode, T, k, E, N, K, sk, got)
        checked += 1
    assert checked == 3 * 6 * 2 * 4 * 5 * 6


def test_workspace_query_accepts_shapes_the_gemm_rejects():
    """Regression: in mode 0 with N = 1 the plan had Nout = N / 2 = 0 columns, hence 0 strips and 0 (tile slot, strip) pairs, and divided
    512 by them: the process died with SIGFPE inside the query.  inc_woq_moe_gemm rejects N % 8 != 0 and K % 32 != 0 before it plans
    (INC_ERR_UNSUPPORTED); the query now returns 0 for them: a shape that cannot run needs no workspace."""
    for mode, N, K in itertools.product((0, 1, 2), (1, 2, 4, 7, 12, 260), (32, 33, 100, 480)):
        if N % 8 == 0 and K % 32 == 0:
            continue
        assert M.workspace_bytes(mode, 1, 2, 8, N, K) == 0, (mode, N, K)
    assert M.workspace_bytes(0, 1, 2, 8, 8, 480) == M.COUNTER_BYTES + 4 * 2 * 8 * 4  # the smallest gate_up that runs still splits


# ---- routings ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", M.INDEX_DTYPES, ids=["int64", "int32"])
@pytest.mark.parametrize("name", list(M.ROUTINGS))
def test_routings_have_the_stated_counts(name, index_dtype):
    r = M.ROUTINGS[name]
    idx = M.top_k_index(r, index_dtype)
    assert idx.dtype is index_dtype and idx.shape == (r.T, r.k)
    assert M.counted(idx, r.E) == list(r.counts)
    ro = M.route_oracle(idx, r.E)
    assert ro["counts"] == list(r.counts) and ro["nvalid"] == sum(r.counts)
    assert ro["ntiles"] == sum(-(-c // 64) for c in r.counts) <= M.tiles_max(ro["S"], r.E)


def test_routing_edges():
    e = M.ROUTINGS["edges"]
    assert list(e.counts[:7]) == [65, 64, 0, 1, 16, 17, 0] and e.E == 8 and (e.T * e.k) % 64 != 0
    assert -1 in e.flat and e.E in e.flat
    assert M.ROUTINGS["one_slot"].T * M.ROUTINGS["one_slot"].k == 1
    s = M.ROUTINGS["short_waves"]
    assert s.T * s.k == 17 and -(-17 // 16) == 2  # seg = 2: wave w owns slots 2 w, 2 w + 1; waves 9..15 start past S
    a = M.ROUTINGS["all_invalid"]
    assert set(a.flat) == {-1, a.E} and M.route_oracle(M.top_k_index(a), a.E)["ntiles"] == 0
    m = M.ROUTINGS["max_experts"]
    assert m.E == 512 > m.T * m.k
    assert max(M.ROUTINGS["many_rows"].counts) >= 15 * 64


def test_route_oracle_is_a_stable_sort():
    r = M.ROUTINGS["edges"]
    ro = M.route_oracle(M.top_k_index(r), r.E)
    order, pos, off = ro["order"].long(), ro["pos"].long(), ro["offsets"].long()
    assert torch.equal(pos[order], torch.arange(ro["S"]))
    flat = torch.tensor(r.flat)
    for e in range(r.E):
        seg = order[off[e]:off[e + 1]]
        assert bool((flat[seg] == e).all()) and bool((seg[1:] > seg[:-1]).all())
    assert bool(((flat[order[ro["nvalid"]:]] < 0) | (flat[order[ro["nvalid"]:]] >= r.E)).all())
    assert ro["tiles"].tolist() == [[0, 0], [0, 64], [1, 65], [3, 129], [4, 130], [5, 146], [7, 163]]
    M.assert_route(M.route_buffer(ro), ro)
    M.assert_route(M.route_buffer(ro, fill=-7), ro)  # entries past the tile count are unspecified


# ---- the comparators reject six mutations of a correct result ----------------------------------------------------------------------------
NOUT, KK, GS = 12, 96, 32  # Nout % 8 == 4: the up half of gate_up starts in the high half of a zero-point word


@pytest.fixture(scope="module", params=M.DTYPES, ids=M.DTYPE_IDS)
def small(request):
    dtype = request.param
    r = M.ROUTINGS["edges3"]
    ro = M.route_oracle(M.top_k_index(r), r.E)
    return dict(dtype=dtype, r=r, ro=ro, gate_up=M.make_experts(r.E, 2 * NOUT, KK, GS), plain=M.make_experts(r.E, 16, KK, GS),
                x=M.make_x(r.T, KK, dtype), h=M.make_x(r.T * r.k, KK, dtype, seed=1), rw=M.make_routing_weights(r.T, r.k))


def _dense_with(ex, e, dtype, zp_from=None, k_keep=None):
    """oracle.woq_dense_weight restated so that a mutation can be put in: column n takes the zero point of column zp_from[n]; only
    the first k_keep k contribute."""
    N, K, G = ex["N"], ex["K"], ex["G"]
    iw, z = O.woq_unpack_optimum(ex["qweight"][e], ex["qzeros"][e], N, K, G, 4)
    if zp_from is not None:
        z = z[zp_from]
    gi = np.arange(K) // (K if G == 1 else ex["group_size"])
    d = (iw.astype(np.int16) - z[:, gi].astype(np.int16)).astype(np.float32) * np.ascontiguousarray(ex["scales"][e].T).astype(np.float32)[:, gi]
    w = torch.from_numpy(d).to(dtype).double()
    if k_keep is not None:
        w[:, k_keep:] = 0
    return w


def _rejects(y, ref, tol):
    with pytest.raises(AssertionError, match="is off by"):
        M.assert_elementwise(y, ref, tol, "mutation")


def test_restated_dense_weight_is_the_oracles(small):
    s = small
    for ex in (s["gate_up"], s["plain"]):
        for e in range(ex["E"]):
            assert torch.equal(_dense_with(ex, e, s["dtype"]), M.dense_expert64(ex, e, s["dtype"]))
    w0, w1 = M.dense_expert64(s["gate_up"], 0, s["dtype"]), M.dense_expert64(s["gate_up"], 1, s["dtype"])
    assert not torch.equal(w0, w1) and not torch.equal(w0[:NOUT], w0[NOUT:])  # experts differ; gate and up halves differ


def test_comparators_accept_the_exact_results(small):
    s = small
    ref, tol = M.gemm_reference(0, s["ro"], s["gate_up"], s["x"], s["dtype"])
    assert ref.shape == (135, NOUT) and bool(torch.isfinite(ref.to(s["dtype"]).float()).all())
    assert M.assert_elementwise(ref.to(s["dtype"]), ref, tol) <= 1.0
    ref, tol = M.gemm_reference(2, s["ro"], s["plain"], s["x"], s["dtype"])
    assert M.assert_elementwise(ref.float(), ref, tol) <= 0.01  # fp32 output: the rounding is far below the accumulation bound
    ref, tol = M.gemm_reference(1, s["ro"], s["plain"], s["h"], s["dtype"], rw=s["rw"])
    assert M.assert_elementwise(ref.float(), ref, tol) <= 0.01


def test_mutation_1_gate_and_up_swapped(small):
    s = small
    ref, tol = M.gemm_reference(0, s["ro"], s["gate_up"], s["x"], s["dtype"])
    bad, _ = M.gemm_reference(0, s["ro"], s["gate_up"], s["x"], s["dtype"],
                              dense=lambda ex, e, dt: torch.cat([M.dense_expert64(ex, e, dt)[NOUT:], M.dense_expert64(ex, e, dt)[:NOUT]]))
    _rejects(bad.to(s["dtype"]), ref, tol)


def test_mutation_2_up_zero_point_from_nibble_0(small):
    """The up column Nout + j sits at nibble (Nout + j) % 8 of its zero-point word; taking nibble j % 8 instead reads the zero point
    four columns away (Nout % 8 == 4).  Only the up half of one expert is mutated."""
    s = small
    ref, tol = M.gemm_reference(0, s["ro"], s["gate_up"], s["x"], s["dtype"])
    n = np.arange(2 * NOUT)
    zp_from = np.where(n >= NOUT, (n // 8) * 8 + (n - NOUT) % 8, n)
    assert not np.array_equal(zp_from, n) and np.array_equal(zp_from[:NOUT], n[:NOUT])
    bad, _ = M.gemm_reference(0, s["ro"], s["gate_up"], s["x"], s["dtype"],
                              dense=lambda ex, e, dt: _dense_with(ex, e, dt, zp_from=zp_from if e == 2 else None))
    lo = int(s["ro"]["offsets"][2])
    assert torch.equal(bad[:lo], ref[:lo])
    _rejects(bad.to(s["dtype"]), ref, tol)


def test_mutation_3_last_k_step_dropped(small):
    s = small
    ref, tol = M.gemm_reference(2, s["ro"], s["plain"], s["x"], s["dtype"])
    bad, _ = M.gemm_reference(2, s["ro"], s["plain"], s["x"], s["dtype"], dense=lambda ex, e, dt: _dense_with(ex, e, dt, k_keep=KK - 32))
    _rejects(bad.float(), ref, tol)


def test_mutation_4_routing_weight_by_sorted_position(small):
    s = small
    ro = s["ro"]
    ref, tol = M.gemm_reference(1, ro, s["plain"], s["h"], s["dtype"], rw=s["rw"])
    flat = s["rw"].reshape(-1).double()
    right, wrong = flat[ro["order"].long()[:ro["nvalid"]]], flat[:ro["nvalid"]]
    assert int((right != wrong).sum()) > ro["nvalid"] // 2
    _rejects((ref / right[:, None] * wrong[:, None]).float(), ref, tol)


def test_mutation_5_a_row_block_from_the_next_tile(small):
    """Tiles of edges3 start at positions 0, 64 (expert 0), 65, 129 (expert 2): the first 6 rows of the tile at 65 get the rows of the
    tile at 129 -- the same expert, the same columns, other tokens."""
    s = small
    ref, tol = M.gemm_reference(2, s["ro"], s["plain"], s["x"], s["dtype"])
    assert s["ro"]["tiles"].tolist() == [[0, 0], [0, 64], [2, 65], [2, 129]]
    bad = ref.clone()
    bad[65:71] = ref[129:135]
    _rejects(bad.float(), ref, tol)


def test_mutation_6_order_inside_an_expert_reversed(small):
    """A valid partition by expert whose order inside expert 2 descends: offsets, the tile table and the tile count are unchanged, the
    GEMM stages would still pair every row with its own token -- only the route comparator can see it."""
    ro = small["ro"]
    bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ro.items()}
    lo, hi = int(ro["offsets"][2]), int(ro["offsets"][3])
    bad["order"][lo:hi] = ro["order"][lo:hi].flip(0)
    bad["pos"][bad["order"].long()] = torch.arange(ro["S"], dtype=torch.int32)
    buf = M.route_buffer(bad)
    with pytest.raises(AssertionError, match=r"route order\["):
        M.assert_route(buf, ro)
    M.assert_route(M.route_buffer(ro), ro)


def test_combine_oracle_is_a_slot_ordered_fp32_sum(small):
    s = small
    ro, r = s["ro"], s["r"]
    y = torch.randn(r.T * r.k, 8, generator=torch.Generator().manual_seed(3)) * 3.0
    y[ro["nvalid"]:] = float("nan")
    out = M.combine_oracle(y, ro, s["dtype"])
    assert out.dtype is s["dtype"] and bool(torch.isfinite(out.float()).all())
    pos = ro["pos"].long().view(r.T, r.k)
    for t in (0, 1, r.T - 1):
        acc = torch.zeros(8)
        for j in range(r.k):
            if pos[t, j] < ro["nvalid"]:
                acc = acc + y[pos[t, j]]
        assert torch.equal(out[t], acc.to(s["dtype"]))
    a = M.ROUTINGS["all_invalid"]
    roa = M.route_oracle(M.top_k_index(a), a.E)
    assert not bool(M.combine_oracle(torch.full((a.T * a.k, 4), float("nan")), roa, s["dtype"]).float().any())
