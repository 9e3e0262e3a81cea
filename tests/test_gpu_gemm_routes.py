"""-m gpu: every route of inc_woq_gemm against an element-wise float64 oracle, through the C entry point with buffers the test owns.

For every case of tests/gemm_route_cases.py (CASES: one or more per kernel family and variant), in bf16 and fp16:
  route     inc_woq_gemm_route, asked with the real addresses, names the kernel and the variant the case is written for;
  oracle    y against x64 @ woq_dense_weight64.T + bias64 within the per-element bound of gemm_route_cases.tolerance;
  guards    y is a window in a sentinel-filled buffer (>= one row before and after, start 16- / 8- / 2-byte aligned as the case asks),
            the workspace is exactly inc_woq_gemm_workspace_bytes long with a sentinel tail: every guard byte is unchanged;
  counters  the first 16 KiB of the workspace are zero afterwards;
  repeat    a second call is bit-identical;
  bare      with workspace = NULL the tile-shaped routes still meet the bound in one pass, the streaming / small routes return
            INC_ERR_WORKSPACE and leave y untouched.
The worst err / tol per route is printed when the module finishes.
"""

import pytest
import torch

from tests import gemm_route_cases as R

pytestmark = pytest.mark.gpu

Y_SENTINEL = 0x7B5A          # as bf16 / fp16 a large finite value no case produces
WS_SENTINEL = 0xA5
WS_TAIL = 4096
COUNTER_BYTES = 16384

_worst = {}
_dev_layers = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\n[gemm routes] worst |y - ref| / tol per route (<= 1 passes)")
        for (route, dt), (r, name) in sorted(_worst.items()):
            print(f"[gemm routes] {route:10s} {dt:5s} {r:.3f}  ({name})")


def _device_layer(hip, c):
    key = (c.N, c.K, c.group_size, c.bits, c.g_idx)
    if key not in _dev_layers:
        L = R.make_layer(*key)
        _dev_layers[key] = dict(
            qweight=torch.from_numpy(L["qweight"]).to(hip), scales=torch.from_numpy(L["scales"]).to(hip),
            qzeros=torch.from_numpy(L["qzeros"]).to(hip), g_idx=None if L["g_idx"] is None else torch.from_numpy(L["g_idx"]).to(hip))
    return R.make_layer(*key), _dev_layers[key]


def _placed(hip, t, align):
    """A copy of t on the device whose first element sits `align`-byte aligned and no better."""
    off = R.misalign(align) // t.element_size()
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=hip)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % align == 0 and (align == 16 or view.data_ptr() % (2 * align) != 0)
    return view


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", R.CASES, ids=R.CASE_IDS)
def test_route_against_elementwise_oracle(hip, c, dtype):
    from neural_compressor_amd import _lib

    lib = _lib.lib
    M, N, K = c.M, c.N, c.K
    layer, dl = _device_layer(hip, c)
    x_cpu, bias_cpu = R.make_x(M, K, dtype), R.make_bias(N, dtype)
    ref, S = R.reference(x_cpu, R.dense_weight64(layer, dtype), bias_cpu)
    x = _placed(hip, x_cpu, c.x_align)
    bias = _placed(hip, bias_cpu, 16)

    # y: a window in a sentinel-filled 16-bit buffer, at least one row of guard on either side
    guard = (N + 7) // 8 * 8 + 8
    start = guard + R.misalign(c.y_align) // 2
    ybits = torch.full((start + M * N + guard + 8,), Y_SENTINEL, dtype=torch.int16, device=hip)
    assert ybits.data_ptr() % 16 == 0
    ywin = ybits[start:start + M * N]
    y_ptr = ywin.data_ptr()
    assert y_ptr % c.y_align == 0 and (c.y_align == 16 or y_ptr % (2 * c.y_align) != 0)

    # workspace: zeroed, exactly the documented size, then a sentinel tail
    ws_bytes = lib.inc_woq_gemm_workspace_bytes(M, N, K)
    ws = torch.zeros(ws_bytes + WS_TAIL, dtype=torch.uint8, device=hip)
    ws[ws_bytes:] = WS_SENTINEL

    got = R.query_route(c, dtype, x.data_ptr(), y_ptr, bias.data_ptr(), ws.data_ptr(), ws_bytes)
    need = got.pop("need")
    assert got == R.expected(c), "the case no longer reaches the kernel it was written for"
    assert need <= ws_bytes

    stream = torch.cuda.current_stream().cuda_stream
    dt = R.dtype_code(dtype)

    def call(ws_ptr, nbytes):
        ybits.fill_(Y_SENTINEL)
        rc = lib.inc_woq_gemm(x.data_ptr(), dt, dl["qweight"].data_ptr(), dl["scales"].data_ptr(), dl["qzeros"].data_ptr(),
                              None if dl["g_idx"] is None else dl["g_idx"].data_ptr(), bias.data_ptr(), y_ptr, M, N, K, layer["G"],
                              c.group_size, c.bits, ws_ptr, nbytes, stream)
        torch.cuda.synchronize()
        return rc

    def guards_intact():
        assert bool((ybits[:start] == Y_SENTINEL).all()) and bool((ybits[start + M * N:] == Y_SENTINEL).all()), "wrote outside y[M, N]"
        assert bool((ws[ws_bytes:] == WS_SENTINEL).all()), "wrote past the workspace"
        if ws_bytes >= COUNTER_BYTES:
            assert not bool(ws[:COUNTER_BYTES].any()), "arrival counters are not back at zero"

    assert call(ws.data_ptr(), ws_bytes) == 0
    guards_intact()
    y1 = ywin.clone().view(dtype).view(M, N)
    r = R.worst_ratio(y1, ref, S, K, dtype)[0]
    print(f"\n[gemm routes] {c.name} {str(dtype)[6:]} {c.route} splitk {c.splitk}: worst err / tol {r:.3f}")
    key = (c.route, "bf16" if dtype is torch.bfloat16 else "fp16")
    if r > _worst.get(key, (-1.0, ""))[0]:
        _worst[key] = (r, c.name)
    R.assert_elementwise(y1, ref, S, K, dtype, c.name)

    assert call(ws.data_ptr(), ws_bytes) == 0
    guards_intact()
    assert torch.equal(ywin, y1.view(torch.int16).view(-1)), "a second call is not bit-identical"

    if need > 0:  # the route can use K-slices: what it does without a workspace
        bare = R.query_route(c, dtype, x.data_ptr(), y_ptr, bias.data_ptr(), None, 0)
        rc = call(None, 0)
        guards_intact()
        if c.route in R.ONE_PASS_FALLBACK:
            assert rc == 0 and bare["route"] == c.route and bare["splitk"] == 1
            y3 = ywin.clone().view(dtype).view(M, N)
            r3 = R.assert_elementwise(y3, ref, S, K, dtype, c.name + " without a workspace")
            print(f"[gemm routes] {c.name} {str(dtype)[6:]} {c.route} without a workspace (one pass): worst err / tol {r3:.3f}")
            if r3 > _worst[key][0]:
                _worst[key] = (r3, c.name + " (no workspace)")
        else:
            assert c.route in ("STREAM_W4", "STREAM_W8", "SMALL")
            assert rc == R.INC_ERR_WORKSPACE
            assert bool((ybits == Y_SENTINEL).all()), "y was written although the call returned INC_ERR_WORKSPACE"
