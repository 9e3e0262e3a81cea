"""CPU: the routing of the fused weight-only GEMM (inc_woq_gemm_route is host-only), the workspace bound, and a self-test of the
element-wise comparator that tests/test_gpu_gemm_routes.py relies on.  No GPU call anywhere in this file."""

import itertools

import pytest
import torch

from tests import gemm_route_cases as R

FAKE_X, FAKE_Y, FAKE_BIAS, FAKE_WS = 0x7F0000010000, 0x7F0000200000, 0x7F0000400000, 0x7F0000800000  # never dereferenced


def _ws_bytes(M, N, K):
    from neural_compressor_amd import _lib

    return _lib.lib.inc_woq_gemm_workspace_bytes(M, N, K)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_route_table(c, dtype):
    """Every case of the GPU file takes the kernel and the variant it was written for.  A threshold change in woq_gemm_plan shows up
    here first: move the shape so that the route keeps its case, then update the table."""
    got = R.query_route(c, dtype, FAKE_X + R.misalign(c.x_align), FAKE_Y + R.misalign(c.y_align), FAKE_BIAS, FAKE_WS, _ws_bytes(c.M, c.N, c.K))
    need = got.pop("need")
    assert got == R.expected(c)
    assert need <= _ws_bytes(c.M, c.N, c.K)
    assert (need > 0) == (c.splitk > 1 or c.route in ("STREAM_W4", "STREAM_W8", "SMALL") or c.name == "d2r_slab_y2_one_pass")
    # without a workspace: one pass where the route can, the same plan (and INC_ERR_WORKSPACE from inc_woq_gemm) where it cannot
    bare = R.query_route(c, dtype, FAKE_X + R.misalign(c.x_align), FAKE_Y + R.misalign(c.y_align), FAKE_BIAS, None, 0)
    assert bare["route"] == c.route and bare["need"] == need
    assert bare["splitk"] == (c.splitk if c.route in ("STREAM_W4", "STREAM_W8", "SMALL") else 1)


def test_route_table_covers_every_route_and_variant():
    assert {c.route for c in R.CASES} == set(R.ROUTES)
    stream4 = {(c.row_blocks, c.steps) for c in R.CASES if c.route == "STREAM_W4"}
    assert stream4 == {(1, 4), (2, 4), (4, 4), (1, 8)}
    assert {c.row_blocks for c in R.CASES if c.route == "STREAM_W8"} == {1, 2, 4}
    assert {c.group_size >= 128 for c in R.CASES if c.route in ("STREAM_W4", "STREAM_W8")} == {True, False}  # both group-lookup forms
    assert {c.y_vec_ok for c in R.CASES if c.route == "D2R" and c.splitk == 1} == {0, 1, 3}
    for route in R.ONE_PASS_FALLBACK:  # with and without K-slices
        assert {c.splitk > 1 for c in R.CASES if c.route == route} == {True, False}, route
    assert {c.x_vec_ok for c in R.CASES if c.route == "TILE"} == {0, 1}
    assert {(c.bits, c.g_idx) for c in R.CASES if c.route == "TILE"} >= {(4, False), (8, False), (4, True), (8, True)}
    assert {c.bits for c in R.CASES if c.route == "TILE_ANYW"} == {3, 6}
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)


def test_route_query_rejects_what_the_gemm_rejects():
    from neural_compressor_amd import _lib

    q = _lib.lib.inc_woq_gemm_route
    tail = (FAKE_X, FAKE_Y, FAKE_BIAS, None, 0, None, None, None, None, None, None)
    assert q(0, 64, 64, 32, 4, _lib.INC_BF16, 0, *tail) == -1
    assert q(8, 64, 64, 32, 9, _lib.INC_BF16, 0, *tail) == -2
    assert q(8, 64, 64, 32, 4, _lib.INC_F32, 0, *tail) == -2
    assert q(8, 64, 64, 20, 4, _lib.INC_BF16, 0, *tail) == -2      # a group boundary inside a packed word
    assert q(8, 64, 64, 20, 4, _lib.INC_BF16, 1, *tail) == R.ROUTES["SMALL"]  # ... is fine with a per-element g_idx
    assert q(1, 4096, 4096, 128, 4, _lib.INC_BF16, 0, *tail) == R.ROUTES["GEMV16"]  # out-parameters may all be NULL


def test_workspace_bytes_accepts_k_below_one_tile_step():
    """Regression: for M > 16, N >= 64 and K < 64 the bound used to plan the 256-row kernels' K-slices over K / 64 = 0 steps and divided
    by zero (the process died with SIGFPE inside ops.woq_gemm before any launch).  Those kernels need K % 128 == 0."""
    from neural_compressor_amd import _lib

    for K in (1, 8, 60, 63):
        assert _lib.lib.inc_woq_gemm_workspace_bytes(17, 64, K) >= 0
        assert _lib.lib.inc_woq_gemm_workspace_bytes(1025, 4096, K) == 0
    assert _lib.lib.inc_woq_gemm_workspace_bytes(17, 64, 60) == 16384 + 17 * 64 * 4  # the streaming kernel's single K-slice


SWEEP_M = (1, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 1024, 1025)
SWEEP_NK = (60, 64, 68, 70, 96, 128, 130, 192, 200, 256, 264, 320, 416, 4096, 11008, 33280)


def test_workspace_bound_covers_every_route():
    """inc_woq_gemm_workspace_bytes(M, N, K) knows neither bits nor group size nor alignment: it must be an upper bound on what the
    chosen route uses, whatever they are."""
    from neural_compressor_amd import _lib

    checked = 0
    for M, N, K in itertools.product(SWEEP_M, SWEEP_NK, SWEEP_NK):
        bound = _lib.lib.inc_woq_gemm_workspace_bytes(M, N, K)
        for bits, gs, (xa, ya), gi in itertools.product((4, 8), (32, 128, K), ((16, 16), (16, 2), (2, 16)), (False, True)):
            c = R.Case("sweep", M, N, K, gs, bits, ya, xa, gi, None, 0, 0, 0, 0, 0)
            got = R.query_route(c, torch.bfloat16, FAKE_X + R.misalign(xa), FAKE_Y + R.misalign(ya), FAKE_BIAS, FAKE_WS, bound)
            assert got["route"] in R.ROUTES, (M, N, K, bits, gs, got)
            assert got["need"] <= bound, (M, N, K, bits, gs, xa, ya, gi, got, bound)
            assert got["splitk"] == 1 or got["need"] > 0
            checked += 1
    assert checked == len(SWEEP_M) * len(SWEEP_NK) ** 2 * 36


# ---- the comparator must see what a relative Frobenius norm does not -----------------------------------------------------------------
@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def exact(request):
    """An otherwise exact result on CPU tensors: float64, rounded once to the output type."""
    dtype = request.param
    M, N, K, gs = 24, 40, 256, 64
    layer = R.make_layer(N, K, gs, 4)
    x, bias = R.make_x(M, K, dtype), R.make_bias(N, dtype)
    w64 = R.dense_weight64(layer, dtype)
    ref, S = R.reference(x, w64, bias)
    return dict(dtype=dtype, M=M, N=N, K=K, gs=gs, layer=layer, x=x, bias=bias, w64=w64, ref=ref, S=S, y=ref.to(dtype))


def _rejects(e, y):
    r, _ = R.worst_ratio(y, e["ref"], e["S"], e["K"], e["dtype"])
    with pytest.raises(AssertionError, match="is off by"):
        R.assert_elementwise(y, e["ref"], e["S"], e["K"], e["dtype"], "mutation")
    return r


def test_comparator_accepts_the_exact_result(exact):
    e = exact
    # (a correctly rounded value may sit half an ulp = up to u_out * |ref| away: the first term of the bound has no slack to give)
    assert 0.25 <= R.assert_elementwise(e["y"], e["ref"], e["S"], e["K"], e["dtype"]) <= 1.0


def test_comparator_rejects_one_dropped_k_term(exact):
    e = exact
    i, j = 7, 13
    terms = e["x"][i].double() * e["w64"][j]
    k = int(torch.argsort(terms.abs())[e["K"] // 2])  # a term of median size, not the largest
    y = e["y"].clone()
    y[i, j] = (e["ref"][i, j] - terms[k]).to(e["dtype"])
    assert int((y != e["y"]).sum()) == 1
    _rejects(e, y)


def test_comparator_rejects_a_neighbour_columns_scale(exact):
    e = exact
    j = 17
    w = e["w64"].clone()
    s = e["layer"]["scales"].astype("float64")  # [G, N]
    ratio = torch.from_numpy(s[:, j + 1] / s[:, j]).repeat_interleave(e["gs"])
    w[j] = (w[j] * ratio).to(e["dtype"]).double()
    y = e["y"].clone()
    y[:, j] = (e["x"].double() @ w[j] + e["bias"].double()[j]).to(e["dtype"])
    _rejects(e, y)


def test_comparator_rejects_a_zero_point_off_by_one(exact):
    e = exact
    j, g = 5, 2
    w = e["w64"].clone()
    sc = float(e["layer"]["scales"][g, j])
    w[j, g * e["gs"]:(g + 1) * e["gs"]] -= sc  # (q - (zp + 1)) * scale, exact in the compute type for 4-bit codes
    w[j] = w[j].to(e["dtype"]).double()
    y = e["y"].clone()
    y[:, j] = (e["x"].double() @ w[j] + e["bias"].double()[j]).to(e["dtype"])
    _rejects(e, y)


def test_comparator_rejects_a_repeated_last_row(exact):
    e = exact
    y = e["y"].clone()
    y[-1] = y[-2]
    _rejects(e, y)


def test_comparator_rejects_two_output_ulps(exact):
    e = exact
    # where rounding dominates the bound (|ref| large against S): y is then >= 1.5 ulp > 1.5 * u_out * |ref| away from ref
    idx = int(torch.argmax(e["ref"].abs() / e["S"]))
    i, j = divmod(idx, e["N"])
    y = e["y"].clone()
    bits = y.view(torch.int16)
    bits[i, j] += 2  # the same sign, two representable values further from zero
    assert int((y != e["y"]).sum()) == 1
    _rejects(e, y)
