"""-m gpu: every route of inc_w8a8_gemm (SmoothQuant W8A8, csrc/gemm_i8.hip) against an exact oracle, through the C entry point with
buffers the test owns.

For every case of tests/w8a8_route_cases.py (CASES), with bf16 and fp16 outputs:
  exact     without corr / bias y is bit-equal to (alpha * acc.float()).to(dtype), acc = xq @ wq^T in float64 (exact);
  bound     with corr and bias |y - exact| <= ulp * |exact| + 1e-6 per element (ulp = 2^-7 bf16 / 2^-10 fp16, exact in float64);
  split     a K-split plan gives the same bits with its workspace, with workspace = NULL and with one byte too few (both one pass);
  stale     the workspace is 0x7F-filled before every call and exactly inc_w8a8_gemm_workspace_bytes long with a 4 KiB canary after
            it: same bits as with a zeroed workspace, canary intact, and a one-pass call leaves the whole workspace alone;
  ragged    y is a window in a sentinel-filled buffer (16- or only 2-byte aligned as the case asks) with two more rows after row M:
            every guard element is unchanged;
  hand-over the first 16 rows of M = 17 (MFMA kernel) equal M = 16 (GEMV) bit for bit;
and W8A8Linear at the module level (its own workspace, 3-D inputs).
"""

import pytest
import torch

import oracle.woq_oracle as O
from tests import w8a8_route_cases as R

pytestmark = pytest.mark.gpu

Y_SENTINEL = 0x7B5A          # as bf16 / fp16 a large finite value no case produces
WS_STALE = 0x7F
WS_CANARY = 0xA5
WS_TAIL = 4096
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "fp16"]
SPLIT_CASES = [c for c in R.CASES if c.split > 1]

_dev = {}


def _case(hip, c):
    """The case's operands on the device and its exact accumulator, computed once and shared (nothing writes to them)."""
    if c.name not in _dev:
        d = {k: (None if v is None else v.to(hip)) for k, v in R.make_inputs(c).items()}
        d["acc"] = R.accumulate(d["xq"], d["wq"])
        _dev[c.name] = d
    return _dev[c.name]


class _Call:
    """One shape at one output type through inc_w8a8_gemm: owns y (guards around the [M, N] window) and the workspace."""

    def __init__(self, hip, c, dtype, M=None):
        from neural_compressor_amd import _lib

        self.lib, self.c, self.dtype = _lib.lib, c, dtype
        self.M, self.N, self.K = (c.M if M is None else M), c.N, c.K
        self.code = _lib.INC_BF16 if dtype is torch.bfloat16 else _lib.INC_F16
        self.lead = 16 + R.misalign(c.y_align) // 2
        count = self.M * self.N
        self.ybits = torch.empty(self.lead + count + 2 * self.N + 16, dtype=torch.int16, device=hip)
        assert self.ybits.data_ptr() % 16 == 0
        self.ywin = self.ybits[self.lead:self.lead + count]
        p = self.ywin.data_ptr()
        assert p % c.y_align == 0 and (c.y_align == 16 or p % (2 * c.y_align) != 0)
        self.need = self.lib.inc_w8a8_gemm_workspace_bytes(self.M, self.N, self.K)
        self.ws = torch.empty(self.need + WS_TAIL, dtype=torch.uint8, device=hip)

    def run(self, d, with_bias, ws="full", stale=True):
        """-> y [M, N].  ws: "full" (need bytes), "short" (need - 1), "null".  Checks the guards of y and of the workspace."""
        self.ybits.fill_(Y_SENTINEL)
        self.ws.fill_(WS_STALE if stale else 0)
        self.ws[self.need:] = WS_CANARY
        ws_ptr, ws_bytes = {"full": (self.ws.data_ptr(), self.need), "short": (self.ws.data_ptr(), self.need - 1), "null": (None, 0)}[ws]
        corr = d["corr"].data_ptr() if with_bias else None
        bias = d["bias"].to(self.dtype) if with_bias else None
        rc = self.lib.inc_w8a8_gemm(d["xq"].data_ptr(), d["wq"].data_ptr(), d["alpha"].data_ptr(), corr,
                                    None if bias is None else bias.data_ptr(), self.ywin.data_ptr(), self.code, self.M, self.N, self.K,
                                    ws_ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, rc
        what = f"{self.c.name} M={self.M} ws={ws}"
        assert bool((self.ybits[:self.lead] == Y_SENTINEL).all()), f"{what}: wrote in front of y"
        assert bool((self.ybits[self.lead + self.M * self.N:] == Y_SENTINEL).all()), f"{what}: wrote past row M of y"
        assert bool((self.ws[self.need:] == WS_CANARY).all()), f"{what}: wrote past the workspace"
        if ws != "full" and stale:
            assert bool((self.ws[:self.need] == WS_STALE).all()), f"{what}: a one-pass call touched the workspace"
        return self.ywin.clone().view(self.dtype).view(self.M, self.N)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_without_bias_is_bit_exact(hip, c, dtype):
    assert R.plan(c.M, c.N, c.K, c.y_align) == R.expected(c), "the case no longer reaches the route it was written for"
    d = _case(hip, c)
    y = _Call(hip, c, dtype).run(d, with_bias=False)
    R.assert_bit_equal(y, R.expect_no_bias(d["alpha"], d["acc"], dtype), c.name)
    if c.fill == "saturated":  # 16384 * K, rounded once (2^25: exact in bf16, beyond fp16's range)
        assert bool((y.double() == (16384.0 * c.K if dtype is torch.bfloat16 else float("inf"))).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("c", [c for c in R.CASES if c.fill == "uniform"], ids=[c.name for c in R.CASES if c.fill == "uniform"])
def test_with_corr_and_bias_is_within_one_ulp(hip, c, dtype):
    d = _case(hip, c)
    y = _Call(hip, c, dtype).run(d, with_bias=True)
    R.assert_within_ulp(y, R.exact_with_bias(d["alpha"], d["acc"], d["corr"], d["bias"].to(dtype)), dtype, c.name)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("c", SPLIT_CASES, ids=[c.name for c in SPLIT_CASES])
def test_split_equals_one_pass_and_ignores_stale_slabs(hip, c, dtype):
    """"Integer addition is associative: bit-identical to the unsplit kernel" (gemm_i8.hip).  Both sides are the one-rounding value."""
    d = _case(hip, c)
    call = _Call(hip, c, dtype)
    assert call.need == (c.tiles - c.full_tiles) * c.split * R.SLAB_BYTES > 0
    want = R.expect_no_bias(d["alpha"], d["acc"], dtype)
    y_split = call.run(d, with_bias=False)
    R.assert_bit_equal(y_split, want, c.name + " split")
    R.assert_bit_equal(call.run(d, with_bias=False, stale=False), y_split, c.name + " zeroed against 0x7F-filled workspace")
    for ws in ("null", "short"):
        R.assert_bit_equal(call.run(d, with_bias=False, ws=ws), y_split, f"{c.name} one pass (workspace {ws}) against split")
    if c.fill == "uniform":
        ex = R.exact_with_bias(d["alpha"], d["acc"], d["corr"], d["bias"].to(dtype))
        for ws in ("full", "null", "short"):
            R.assert_within_ulp(call.run(d, with_bias=True, ws=ws), ex, dtype, f"{c.name} workspace {ws}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_gemv_hands_over_to_the_mfma_kernel(hip, dtype):
    c = R.BY_NAME["handover_m17"]
    d = _case(hip, c)
    y17 = _Call(hip, c, dtype).run(d, with_bias=False)
    d16 = dict(d, xq=d["xq"][:16].contiguous())
    assert R.plan(16, c.N, c.K)["kernel"] == "GEMV" and R.plan(17, c.N, c.K)["kernel"] == "MFMA"
    y16 = _Call(hip, c, dtype, M=16).run(d16, with_bias=False)
    R.assert_bit_equal(y16, y17[:16], "M = 16 (GEMV) against the first 16 rows of M = 17 (MFMA)")
    R.assert_bit_equal(y16, R.expect_no_bias(d["alpha"], d["acc"][:16], dtype), "M = 16")


# ---- module level ---------------------------------------------------------------------------------------------------------------------
def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


_modules = {}


def _module(hip, K):
    """W8A8Linear.from_float of a Linear(K, 264) with bias, its float weights and the calibrated input range (built once)."""
    if K not in _modules:
        from neural_compressor_amd.torch.algorithms.smooth_quant import W8A8Linear

        g = torch.Generator().manual_seed(K)
        lin = torch.nn.Linear(K, 264, bias=True).half()
        lin.weight.data.copy_(torch.randn(264, K, generator=g) * 0.05)
        lin.bias.data.copy_(torch.randn(264, generator=g))
        mn, mx = torch.full((K,), -4.0), torch.full((K,), 5.0)
        _modules[K] = (W8A8Linear.from_float(lin.to(hip), mn, mx, device=hip), lin.weight.detach().float().cpu(), lin.bias.detach().float().cpu(), mn, mx)
    return _modules[K]


@pytest.mark.parametrize("K,lead", [(200, (1, 1)), (200, (2, 10)), (200, (3, 100)), (1024, (1, 33))],
                         ids=["k200_1tok", "k200_20tok", "k200_300tok", "k1024_33tok_split"])
def test_w8a8_linear_is_the_composition_and_matches_the_oracle(hip, K, lead):
    from neural_compressor_amd import ops

    m, w, b, mn, mx = _module(hip, K)
    T = lead[0] * lead[1]
    assert m.kp == R.ceil_div(K, 128) * 128 and m.qweight.shape == (264, m.kp)
    route = R.plan(T, 264, m.kp)
    assert (route["kernel"], route["split"]) == {1: ("GEMV", 1), 20: ("MFMA", 1), 300: ("MFMA", 1), 33: ("MFMA", 2)}[T]
    g = torch.Generator().manual_seed(T)
    x = (torch.randn(*lead, K, generator=g) * 1.2 + 0.3).half()
    y = m(x.to(hip))
    assert y.shape == (*lead, 264) and y.dtype is torch.float16
    sx, zp = float(m.act_scale), int(m.act_zp)
    assert zp == O.sq_act_qparams(torch.ones(K), mn, mx)[1] == 113
    xq = ops.sq_quant_act(x.to(hip).reshape(T, K), None, sx, zp, m.kp)
    y2 = ops.w8a8_gemm(xq, m.qweight, m.alpha, m.corr, m.bias, torch.float16)
    R.assert_bit_equal(y.reshape(T, 264), y2, "forward against sq_quant_act -> w8a8_gemm")
    want = O.sq_w8a8_linear(x.float().reshape(T, K), w, None, sx, zp, b)
    assert rel_fro(y.reshape(T, 264).float().cpu(), want) <= 1e-3  # fp16 output rounding
