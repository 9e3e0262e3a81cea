"""CPU: the plan of the SmoothQuant W8A8 GEMM (inc_w8a8_gemm_workspace_bytes is host-only) against its Python mirror and the route
table of tests/w8a8_route_cases.py, what that table covers, and a self-test of the comparators tests/test_gpu_w8a8_routes.py relies on.
No GPU call anywhere in this file."""

import itertools

import pytest
import torch

from tests import w8a8_route_cases as R


def _ws_bytes(M, N, K):
    from neural_compressor_amd import _lib

    return _lib.lib.inc_w8a8_gemm_workspace_bytes(M, N, K)


@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_route_table(c):
    """Every case of the GPU file takes the kernel, the split and the store form it was written for, and the library reserves exactly
    the slabs of that plan.  A threshold change in i8_tail_plan shows up here first: move the shape so that the route keeps its case."""
    assert R.plan(c.M, c.N, c.K, c.y_align) == R.expected(c)
    need = _ws_bytes(c.M, c.N, c.K)
    assert need == R.workspace_bytes(c.M, c.N, c.K)
    assert need == ((c.tiles - c.full_tiles) * c.split * 256 * 256 * 4 if c.split > 1 else 0)
    assert (need > 0) == (c.split > 1)
    if c.split > 1:  # ... and without a workspace the same call is one pass over every tile
        bare = R.plan(c.M, c.N, c.K, c.y_align, workspace=False)
        assert (bare["split"], bare["full_tiles"], bare["steps"]) == (1, c.tiles, c.K // 128)
        steps, per_split = R.split_steps(c.K // 128, c.split)
        assert steps == c.steps and per_split[-1][1] == c.nk_last
        assert sum(max(nk, 0) for _, nk in per_split) == c.K // 128, "the splits do not cover K once"
        for kbase, nk in per_split:  # the K-tiles a split loads (issue() clamps to its last one; an empty split loads one tile, unused)
            assert 0 <= kbase + min(0, nk - 1) and kbase + nk - 1 < c.K // 128


def test_route_table_covers_every_path():
    mfma = [c for c in R.CASES if c.kernel == "MFMA"]
    assert {c.split for c in mfma} >= {1, 2, 8}
    assert any(c.split > 1 and c.nk_last <= 0 for c in mfma), "no case with an empty last K-split"
    assert any(c.split > 1 and 0 < c.nk_last < c.steps for c in mfma), "no case with uneven K-splits"
    assert any(c.full_tiles > 0 and c.split > 1 for c in mfma), "no case with full tiles followed by split tail tiles"
    assert any(c.split == 1 and c.full_tiles % 8 != 0 and c.full_tiles > 8 for c in mfma), "XCD remap with q > 0 and r > 0"
    assert any(R.tiles_m(c) % 8 != 0 and R.tiles_m(c) > 8 for c in mfma), "no case with a partial last band"
    assert {c.y_vec_ok for c in mfma if c.split == 1} == {0, 1}
    assert {c.y_vec_ok for c in mfma if c.split > 1} == {0, 1}
    for split in (False, True):  # a misaligned y with N % 4 == 0, in either epilogue
        assert any(c.y_align == 2 and c.N % 4 == 0 and (c.split > 1) == split for c in mfma)
    gemv = [c for c in R.CASES if c.kernel == "GEMV"]
    assert {c.M for c in gemv} == set(range(1, 17))
    assert {c.mt for c in gemv} == {1, 4, 8, 16}
    assert any(c.K == 128 for c in gemv) and any(c.K % R.GV_KC == 0 for c in gemv) and any(c.K % R.GV_KC == 128 for c in gemv)
    assert any(c.N % 16 != 0 for c in gemv)
    # the hand-over: M = 16 and M = 17 on one layer
    a, b = R.BY_NAME["gemv_m16"], R.BY_NAME["handover_m17"]
    assert (a.N, a.K, a.kernel) == (b.N, b.K, "GEMV") and b.kernel == "MFMA" and (a.M, b.M) == (16, 17)
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)


def test_workspace_is_zero_where_nothing_is_split():
    for M in range(1, 17):
        assert _ws_bytes(M, 4096, 4096) == 0
    for K in (1, 64, 127, 1000, 4100):  # K % 128 != 0: the GEMM refuses these
        assert _ws_bytes(64, 256, K) == 0
    assert _ws_bytes(64, 0, 1024) == 0 and _ws_bytes(64, 256, 0) == 0
    assert _ws_bytes(64, 256, 384) == 0          # too few K-steps
    assert _ws_bytes(4096, 4096, 11008) == 0     # 256 tiles: no tail
    assert _ws_bytes(64, 256, 1024) == 2 * 256 * 256 * 4


SWEEP_M = (17, 32, 33, 256, 257, 1024, 4097)
SWEEP_N = (1, 255, 256, 257, 4096, 8200)
SWEEP_K = (128, 512, 1024, 3072, 4224, 6144, 11008)


def test_mirror_follows_the_library_over_a_sweep():
    splits = set()
    for M, N, K in itertools.product(SWEEP_M, SWEEP_N, SWEEP_K):
        assert _ws_bytes(M, N, K) == R.workspace_bytes(M, N, K), (M, N, K)
        p = R.plan(M, N, K)
        assert R.workspace_bytes(M, N, K) == ((p["tiles"] - p["full_tiles"]) * p["split"] * R.SLAB_BYTES if p["split"] > 1 else 0)
        splits.add(p["split"])
    assert splits >= {1, 2, 3, 8}  # the sweep walks down the split ladder, not only its ends


def test_mirror_of_the_tile_maps_is_a_bijection():
    """The mirror's XCD remap and banded decode visit every tile once (what a GPU case with r > 0 / a partial band checks on the kernel)."""
    for full in (1, 3, 8, 12, 18, 256):
        assert sorted(R.xcd_remap(wg, full) for wg in range(full)) == list(range(full))
    for tm, tn in ((1, 1), (2, 6), (9, 2), (17, 16), (8, 3)):
        assert sorted(R.banded_tile_decode(i, tm, tn) for i in range(tm * tn)) == sorted(itertools.product(range(tm), range(tn)))


# ---- the comparators --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def exact(request):
    """An exact result on CPU tensors for a small shape of the table's making."""
    dtype = request.param
    c = R.Case("cpu", 24, 40, 256, "MFMA", 1, 1, 1, 2, 2, 1, 16, "uniform", 0)
    i = R.make_inputs(c)
    acc = R.accumulate(i["xq"], i["wq"])
    bias = i["bias"].to(dtype)
    return dict(dtype=dtype, acc=acc, y0=R.expect_no_bias(i["alpha"], acc, dtype), ex=R.exact_with_bias(i["alpha"], acc, i["corr"], bias), **i)


def _bump(y, i, j, by):
    """y with element (i, j) moved `by` representable values away from zero."""
    y = y.clone()
    y.view(torch.int16)[i, j] += by
    return y


def test_comparators_accept_the_exact_result(exact):
    e = exact
    R.assert_bit_equal(e["y0"], e["y0"].clone(), "exact")
    R.assert_within_ulp(e["ex"].to(e["dtype"]), e["ex"], e["dtype"], "exact")


def test_bit_comparator_rejects_one_output_ulp(exact):
    e = exact
    y = _bump(e["y0"], 7, 13, 1)
    assert int((y != e["y0"]).sum()) == 1
    with pytest.raises(AssertionError, match=r"1 of 960 elements differ in bits, first at \(7, 13\)"):
        R.assert_bit_equal(y, e["y0"], "mutation")


def test_bit_comparator_rejects_a_neighbour_columns_alpha(exact):
    e = exact
    y = e["y0"].clone()
    y[:, 17] = (e["alpha"][18] * e["acc"][:, 17].float()).to(e["dtype"])
    with pytest.raises(AssertionError, match="differ in bits"):
        R.assert_bit_equal(y, e["y0"], "mutation")


def test_ulp_comparator_rejects_three_output_ulps_and_a_dropped_k_step(exact):
    e = exact
    # a correctly rounded value is <= 0.5 spacing from exact; 3 values further it is >= 2.5 spacings away, and the bound
    # ulp * |exact| is < 2 spacings (the spacing at |exact| is >= ulp * |exact| / 2)
    idx = int(torch.argmax(e["ex"].abs()))
    i, j = divmod(idx, e["ex"].shape[1])
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_within_ulp(_bump(e["ex"].to(e["dtype"]), i, j, 3), e["ex"], e["dtype"], "mutation")
    # the last 128-byte K-step missing from one row
    acc = e["acc"].clone()
    acc[5] = R.accumulate(e["xq"][5:6, :128], e["wq"][:, :128])[0]
    y = R.exact_with_bias(e["alpha"], acc, e["corr"], e["bias"].to(e["dtype"])).to(e["dtype"])
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_within_ulp(y, e["ex"], e["dtype"], "mutation")
    nan = e["ex"].to(e["dtype"])
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_within_ulp(nan, e["ex"], e["dtype"], "mutation")
