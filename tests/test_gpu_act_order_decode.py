"""-m gpu: inc_woq_gemm_perm (y = x[:, k_order] . W_sorted^T + bias in one launch) and the act_order module on top of it.

For every case of tests/act_order_cases.py, in bf16 and fp16, with a random permutation, the reversal and the identity:
  route     ops.woq_gemm_route for the shape names the kernel and variant of the route table (tests/gemm_route_cases.py);
  exact     the output is torch.equal to inc_woq_gemm on x.index_select(1, perm) with the same workspace (same body, same plan),
            and for the identity to inc_woq_gemm on x itself; an x that is only 2-byte aligned gives the same bits;
  oracle    element by element against the float64 reference of x[:, perm] within gemm_route_cases.tolerance;
  guards    sentinels around y and behind the workspace are intact, the arrival counters are back at zero, a second call is
            bit-identical;
  clamp     a k_order with the entries -1 and K gives the finite result of the same array with 0 and K - 1 in their place.
Then the rejections (M = 65, a k_order off by 4 bytes, a route without a gathering form: INC_ERR_UNSUPPORTED, y untouched) and
MI355XWeightOnlyLinear on the "fused_act_order" plan: one launch without torch's index_select up to 64 rows, through a prepared
call that is reused, rebuilt after g_idx is rewritten, and capturable in a graph.
"""

import pytest
import torch

from tests import act_order_cases as A
from tests import gemm_route_cases as R

pytestmark = pytest.mark.gpu

Y_SENTINEL = 0x7B5A          # as bf16 / fp16 a large finite value no case produces
WS_SENTINEL = 0xA5
WS_TAIL = 4096
COUNTER_BYTES = 16384
INC_ERR_UNSUPPORTED = -2

_dev_layers = {}


def _device_layer(hip, c):
    if c.name not in _dev_layers:
        L = A.layer(c)
        _dev_layers[c.name] = {k: torch.from_numpy(L[k]).to(hip) for k in ("qweight", "scales", "qzeros")}
    return A.layer(c), _dev_layers[c.name]


class _Buffers:
    """x, bias, a sentinel-guarded y window and an exactly sized workspace with a sentinel tail for one (layer, M, dtype)."""

    def __init__(self, hip, N, K, M, x_cpu, bias_cpu):
        from neural_compressor_amd import _lib

        self.M, self.N, self.K = M, N, K
        self.x = x_cpu.to(hip)
        xbuf = torch.zeros(M * K + 8, dtype=x_cpu.dtype, device=hip)  # the same values one element (2 bytes) off a 16-byte boundary
        self.x_off2 = xbuf[1:1 + M * K].view(M, K)
        self.x_off2.copy_(x_cpu)
        assert self.x.data_ptr() % 16 == 0 and self.x_off2.data_ptr() % 16 == 2
        self.bias = bias_cpu.to(hip)
        guard = (N + 7) // 8 * 8 + 8
        self.start = guard
        self.ybits = torch.full((guard + M * N + guard + 8,), Y_SENTINEL, dtype=torch.int16, device=hip)
        self.ywin = self.ybits[guard:guard + M * N]
        assert self.ywin.data_ptr() % 16 == 0
        self.ws_bytes = _lib.lib.inc_woq_gemm_workspace_bytes(M, N, K)
        self.ws = torch.zeros(self.ws_bytes + WS_TAIL, dtype=torch.uint8, device=hip)
        self.ws[self.ws_bytes:] = WS_SENTINEL

    def guards_intact(self):
        s, n = self.start, self.M * self.N
        assert bool((self.ybits[:s] == Y_SENTINEL).all()) and bool((self.ybits[s + n:] == Y_SENTINEL).all()), "wrote outside y[M, N]"
        assert bool((self.ws[self.ws_bytes:] == WS_SENTINEL).all()), "wrote past the workspace"
        if self.ws_bytes >= COUNTER_BYTES:
            assert not bool(self.ws[:COUNTER_BYTES].any()), "arrival counters are not back at zero"

    def untouched(self):
        return bool((self.ybits == Y_SENTINEL).all())

    def result(self, dtype):
        return self.ywin.clone().view(dtype).view(self.M, self.N)


def _launch(b, dl, G, group_size, bits, dtype, x, k_order):
    """inc_woq_gemm_perm (k_order given) or inc_woq_gemm into b's y window with b's workspace -> return code."""
    from neural_compressor_amd import _lib

    lib, dt, stream = _lib.lib, R.dtype_code(dtype), torch.cuda.current_stream().cuda_stream
    b.ybits.fill_(Y_SENTINEL)
    tail = (b.bias.data_ptr(), b.ywin.data_ptr(), b.M, b.N, b.K, G, group_size, bits, b.ws.data_ptr(), b.ws_bytes, stream)
    if k_order is None:
        rc = lib.inc_woq_gemm(x.data_ptr(), dt, dl["qweight"].data_ptr(), dl["scales"].data_ptr(), dl["qzeros"].data_ptr(), None, *tail)
    else:
        rc = lib.inc_woq_gemm_perm(x.data_ptr(), dt, k_order.data_ptr(), dl["qweight"].data_ptr(), dl["scales"].data_ptr(),
                                   dl["qzeros"].data_ptr(), *tail)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c,M", A.PARAMS, ids=A.PARAM_IDS)
def test_perm_decode_exact_and_against_the_oracle(hip, c, M, dtype):
    from neural_compressor_amd import ops

    N, K = c.N, c.K
    layer, dl = _device_layer(hip, c)
    G = layer["G"]
    x_cpu, bias_cpu = A.reference(c, M, dtype, "identity")[:2]
    b = _Buffers(hip, N, K, M, x_cpu, bias_cpu)

    want = A.route_case(c, M)
    got = ops.woq_gemm_route(M, N, K, c.group_size, c.bits, dtype, False, b.x.data_ptr(), b.ywin.data_ptr(), b.bias.data_ptr(),
                             b.ws.data_ptr(), b.ws_bytes)
    assert got.pop("need") <= b.ws_bytes
    assert got == R.expected(want), "the case no longer reaches the kernel it was written for"

    def run(x, k_order):
        assert _launch(b, dl, G, c.group_size, c.bits, dtype, x, k_order) == 0
        b.guards_intact()
        return b.result(dtype)

    y_plain = run(b.x, None)
    for kind in A.PERM_KINDS:
        p = torch.from_numpy(A.perm(K, kind)).to(hip)
        assert p.dtype is torch.int32 and p.data_ptr() % 16 == 0
        y = run(b.x, p)
        assert torch.equal(run(b.x, p), y), f"{kind}: a second call is not bit-identical"
        assert torch.equal(y, run(b.x.index_select(1, p), None)), f"{kind}: differs from inc_woq_gemm on the gathered x"
        if kind == "identity":
            assert torch.equal(y, y_plain), "the identity differs from inc_woq_gemm"
        _, _, ref, S = A.reference(c, M, dtype, kind)
        r = R.assert_elementwise(y, ref, S, K, dtype, f"{c.name} M = {M} {kind}")
        print(f"\n[act_order decode] {c.name} m{M} {str(dtype)[6:]} {want.route} {kind}: worst err / tol {r:.3f}")
        if kind == "random":
            assert torch.equal(run(b.x_off2, p), y), "an x that is only 2-byte aligned gives other bits"
            # entries outside [0, K-1] are clamped, never followed
            bad, clamped = p.clone(), p.clone()
            bad[3], clamped[3] = -1, 0
            bad[K - 5], clamped[K - 5] = K, K - 1
            y_bad = run(b.x, bad)
            assert bool(torch.isfinite(y_bad.float()).all())
            assert torch.equal(y_bad, run(b.x, clamped)), "out-of-range entries are not clamped to 0 / K - 1"


@pytest.mark.parametrize("what", ["m65", "k_order_off_by_4_bytes", "route_small", "route_tile"])
def test_perm_rejections_leave_y_untouched(hip, what):
    M, N, K, gs = {"m65": (65, 200, 416, 32), "k_order_off_by_4_bytes": (5, 200, 416, 32), "route_small": (16, 60, 256, 128),
                   "route_tile": (40, 70, 200, 40)}[what]
    dtype = torch.bfloat16
    L = R.make_layer(N, K, gs, 4)
    dl = {k: torch.from_numpy(L[k]).to(hip) for k in ("qweight", "scales", "qzeros")}
    b = _Buffers(hip, N, K, M, R.make_x(M, K, dtype), R.make_bias(N, dtype))
    pbuf = torch.arange(-1, K + 3, dtype=torch.int32, device=hip)
    p = pbuf[1:1 + K]                                    # 0 .. K-1, 4 bytes off a 16-byte boundary
    assert p.data_ptr() % 16 == 4 and int(p[0]) == 0
    if what != "k_order_off_by_4_bytes":
        p = p.clone()
        assert p.data_ptr() % 16 == 0
    assert _launch(b, dl, L["G"], gs, 4, dtype, b.x, p) == INC_ERR_UNSUPPORTED
    assert b.untouched(), "y was written although the call returned INC_ERR_UNSUPPORTED"
    b.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------------
MN, MK, MGS = 264, 1024, 128


def _act_order_module(hip, seed=31):
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    g = torch.Generator().manual_seed(seed)
    iw = torch.randint(0, 16, (MN, MK), generator=g, dtype=torch.int32)
    sc = torch.rand(MN, MK // MGS, generator=g) * 0.02 + 0.002
    zp = torch.randint(1, 16, (MN, MK // MGS), generator=g, dtype=torch.int32)
    bias = torch.randn(MN, generator=g)
    m = MI355XWeightOnlyLinear(MK, MN, bits=4, group_size=MGS, zp=True, bias=True, g_idx=True, device=hip)
    m.pack(iw.to(hip), sc.to(hip), zp.to(hip), bias.to(hip), g_idx=torch.randperm(MK, generator=g).to(hip))
    return m, g


def _two_launch(m, x):
    """Today's form: index_select + ops.woq_gemm per call."""
    cls = type(m)
    assert cls.ACT_ORDER_FUSED_GATHER is True
    cls.ACT_ORDER_FUSED_GATHER = False
    try:
        y = m(x)
        assert m.__dict__.get("_call") is None
        return y
    finally:
        cls.ACT_ORDER_FUSED_GATHER = True


def _forbid_index_select(monkeypatch):
    calls = []

    def raiser(self, *a, **k):
        calls.append(1)
        raise AssertionError("index_select on the decode path")

    monkeypatch.setattr(torch.Tensor, "index_select", raiser)
    return calls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_module_decodes_in_one_launch_without_index_select(hip, monkeypatch, dtype):
    m, g = _act_order_module(hip)
    xs = {M: (torch.randn(M, MK, generator=g) * 0.5).to(dtype).to(hip) for M in (1, 5, 64)}
    want = {M: _two_launch(m, x) for M, x in xs.items()}
    assert m._plan == "fused_act_order"
    w = m.recover(dtype=torch.float32)
    for M, x in xs.items():  # (the two-launch form itself is what the module has always computed)
        ref = x.float() @ w.T + m.bias.float()
        assert float((want[M].float() - ref).norm() / ref.norm()) <= 5e-3
    _forbid_index_select(monkeypatch)
    for M, x in xs.items():
        assert torch.equal(m(x), want[M]), f"M = {M}"
    call = m.__dict__["_call"]
    assert call is not None and call.ko is not None
    assert call.current(m.qweight, m.scales, m.qzeros, m.bias, m.g_idx)
    for M, x in xs.items():
        assert torch.equal(m(x), want[M])
        assert torch.equal(m(x.view(1, M, MK)), want[M].view(1, M, MN))
        assert m.__dict__["_call"] is call, "the prepared call was rebuilt"


def test_module_above_64_rows_gathers_with_index_select(hip, monkeypatch):
    m, g = _act_order_module(hip)
    x = (torch.randn(65, MK, generator=g) * 0.5).to(torch.bfloat16).to(hip)
    want = _two_launch(m, x)
    real, calls = torch.Tensor.index_select, []

    def counting(self, *a, **k):
        calls.append(self.shape)
        return real(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "index_select", counting)
    assert torch.equal(m(x), want)          # builds the prepared call
    assert torch.equal(m(x), want)          # ... and goes through it
    assert calls == [x.shape, x.shape]
    call = m.__dict__["_call"]
    assert call is not None
    assert torch.equal(_two_launch(m, x), want)  # the switch off: the call is dropped (asserted there), the same bits
    assert torch.equal(m(x), want) and m.__dict__["_call"] not in (None, call)  # ... and on again: rebuilt


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("bits", [4, 8])
def test_plan_sorts_the_words_as_sort_packed_k_does(hip, bits, M):
    """The K-sorted words of the 4 / 8-bit act_order plan are ops.sort_packed_k's, and the forward is inc_woq_gemm on them and the
    gathered x, bit for bit."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.weight_only.modules import MI355XWeightOnlyLinear

    N, K, gs = 64, 256, 32
    g = torch.Generator().manual_seed(900 + bits)
    iw = torch.randint(0, 1 << bits, (N, K), generator=g, dtype=torch.int32)
    sc = torch.rand(N, K // gs, generator=g) * 0.02 + 0.002
    zp = torch.randint(1, 1 << bits, (N, K // gs), generator=g, dtype=torch.int32)
    m = MI355XWeightOnlyLinear(K, N, bits=bits, group_size=gs, zp=True, bias=True, g_idx=True, device=hip)
    m.pack(iw.to(hip), sc.to(hip), zp.to(hip), torch.randn(N, generator=g).to(hip), g_idx=torch.randperm(K, generator=g).to(hip))
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).to(hip)
    y = m(x)
    assert m._plan == "fused_act_order"
    assert torch.equal(m._qweight_sorted, ops.sort_packed_k(m.qweight, m._k_order, K, bits))
    assert torch.equal(y, ops.woq_gemm(x.index_select(1, m._k_order), m._qweight_sorted, m.scales, m.qzeros, m.bias, N, K, gs, bits))


def test_module_rebuilds_plan_and_call_after_g_idx_is_rewritten(hip, monkeypatch):
    m, g = _act_order_module(hip)
    x = (torch.randn(5, MK, generator=g) * 0.5).to(torch.bfloat16).to(hip)
    y1 = m(x)
    call1, sorted1 = m.__dict__["_call"], m._qweight_sorted
    assert call1 is not None
    # the same codes under another permutation of whole groups, written into the same g_idx storage
    perm2 = torch.randperm(MK, generator=g)
    m.g_idx.copy_((torch.argsort(perm2) // MGS).to(torch.int32))
    assert not call1.current(m.qweight, m.scales, m.qzeros, m.bias, m.g_idx)
    want = _two_launch(m, x)
    _forbid_index_select(monkeypatch)
    y2 = m(x)
    call2 = m.__dict__["_call"]
    assert m._plan == "fused_act_order" and call2 is not None and call2 is not call1 and m._qweight_sorted is not sorted1
    assert torch.equal(y2, want) and not torch.equal(y2, y1)
    ref = x.float() @ m.recover(dtype=torch.float32).T + m.bias.float()
    assert float((y2.float() - ref).norm() / ref.norm()) <= 5e-3


def test_module_decode_captured_in_a_graph(hip, monkeypatch):
    m, g = _act_order_module(hip)
    x = (torch.randn(1, MK, generator=g) * 0.5).to(torch.bfloat16).to(hip)
    assert m._forward_plan() == "fused_act_order"  # (sorting the words once per packed state may gather as it likes)
    _forbid_index_select(monkeypatch)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        eager = m(x)  # builds the prepared call and the stream's workspace outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = m(x)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_((torch.randn(1, MK, generator=g) * 0.5).to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(out, m(x))
