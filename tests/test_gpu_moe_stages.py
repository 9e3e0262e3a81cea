"""-m gpu: every stage of the fused MoE experts forward (csrc/gemm_moe.hip) against an oracle of its own (tests/moe_stage_cases.py).

  route     inc_moe_route on every routing, int64 and int32 ids: offsets, order, pos, the tile table and the tile count equal the stable
            argsort's, exactly; nothing is written outside the route buffer.
  gemm      inc_woq_moe_gemm, every case x mode x dtype, fed the ORACLE's route buffer and (mode 1) test data for h, so a stage fails on
            its own: the element-wise float64 bound on the valid rows; rows past the valid slots, the guards around `out` and around the
            workspace bit-untouched; arrival counters back at zero; a second call bit-identical.
  weights   fp32 / bf16 / fp16 routing weights on one mode-1 case.
  shared    a mode-0 call then a mode-1 call with another strip count in one workspace == the same calls with a workspace each.
  invalid   a routing with no valid id: tile count 0, both GEMM modes write nothing, combine returns exact zeros.
  combine   inc_moe_combine in bf16 and fp16, H = 264 and H = 4, y rows past the valid slots NaN: equal to the fp32 slot-order sum.
  chain     MI355XWeightOnlyExperts.forward at tail shapes against the chained oracle with the stage bounds carried forward.
The worst err / tol per stage is printed when the module finishes.
"""

import pytest
import torch

from tests import moe_stage_cases as M

pytestmark = pytest.mark.gpu

OUT_SENTINEL = 0x7B   # 0x7B7B (bf16 1.3e36, fp16 61280) / 0x7B7B7B7B (fp32 1.3e36): finite values no case produces
WS_SENTINEL = 0xA5
GUARD = 4096          # bytes before and after every window (a multiple of 16: the windows start 16-byte aligned)
ROUTE_SENTINEL = -12345

_worst = {}
_dev = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\n[moe stages] worst |y - ref| / tol per stage (<= 1 passes)")
        for (stage, dt), (r, name) in sorted(_worst.items()):
            print(f"[moe stages] {stage:8s} {dt:5s} {r:.3f}  ({name})")


def _note(stage, dtype, r, name):
    key = (stage, M.DTYPE_IDS[M.DTYPES.index(dtype)])
    if r > _worst.get(key, (-1.0, ""))[0]:
        _worst[key] = (r, name)


def _device_experts(hip, ex):
    key = (ex["E"], ex["N"], ex["K"], ex["group_size"])
    if key not in _dev:
        _dev[key] = {n: torch.from_numpy(ex[n]).to(hip) for n in ("qweight", "scales", "qzeros")}
    return _dev[key]


def _routing(hip, name, index_dtype=torch.int64):
    """(routing, oracle, the oracle's route buffer on the device); the counts are asserted on the CPU before any launch."""
    r = M.ROUTINGS[name]
    idx = M.top_k_index(r, index_dtype)
    assert M.counted(idx, r.E) == list(r.counts)
    ro = M.route_oracle(idx, r.E)
    return r, ro, M.route_buffer(ro).to(hip)


def _window(hip, nbytes, sentinel):
    """(buffer, window): `nbytes` at a 16-byte aligned offset inside a sentinel-filled uint8 buffer, GUARD bytes on either side."""
    buf = torch.full((GUARD + nbytes + GUARD,), sentinel, dtype=torch.uint8, device=hip)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes, sentinel, what):
    assert bool((buf[:GUARD] == sentinel).all()), f"wrote before {what}"
    assert bool((buf[GUARD + nbytes:] == sentinel).all()), f"wrote past {what}"


def _out_shape(mode, S, Nout, dtype):
    return (S, Nout), (dtype if mode == 0 else torch.float32)


class _Gemm:
    """One GEMM case on the device: `out` and the workspace are windows in sentinel-filled buffers, the workspace exactly
    inc_woq_moe_gemm_workspace_bytes long and zeroed."""

    def __init__(self, hip, mode, r, ro, route, ex, a, dtype, rw=None, ws=None):
        self.mode, self.r, self.ro, self.route, self.ex, self.rw = mode, r, ro, route, ex, rw
        self.dex = _device_experts(hip, ex)
        self.a = a.to(hip)
        self.rwd = None if rw is None else rw.to(hip)
        self.S = r.T * r.k
        self.Nout = ex["N"] // 2 if mode == 0 else ex["N"]
        shape, odt = _out_shape(mode, self.S, self.Nout, dtype)
        self.out_bytes = self.S * self.Nout * torch.empty(0, dtype=odt).element_size()
        self.out_buf, win = _window(hip, self.out_bytes, OUT_SENTINEL)
        self.out = win.view(odt).view(shape)
        assert self.out.data_ptr() % 16 == 0
        self.need = M.workspace_bytes(mode, r.T, r.k, r.E, ex["N"], ex["K"])
        if ws is None:
            self.ws_buf, self.ws = _window(hip, self.need, WS_SENTINEL)
            self.ws.zero_()
        else:
            self.ws_buf, self.ws = None, ws
            assert ws.numel() >= self.need
        assert self.ws.data_ptr() % 16 == 0

    def __call__(self):
        from neural_compressor_amd import ops

        self.out_buf.fill_(OUT_SENTINEL)
        got = ops.woq_moe_gemm(self.mode, self.a, self.route, self.dex["qweight"], self.dex["scales"], self.dex["qzeros"], self.r.T, self.r.k,
                               self.ex["group_size"], routing_weights=self.rwd, out=self.out, workspace=self.ws)
        torch.cuda.synchronize()
        assert got is self.out
        return self.out_buf.clone()

    def check_untouched(self):
        nvalid = self.ro["nvalid"]
        _guards_intact(self.out_buf, self.out_bytes, OUT_SENTINEL, "out")
        tail = self.out_buf[GUARD:GUARD + self.out_bytes].view(self.S, -1)[nvalid:]
        assert bool((tail == OUT_SENTINEL).all()), "rows of out past the valid slots were written"
        if self.ws_buf is not None:
            _guards_intact(self.ws_buf, self.need, WS_SENTINEL, "the workspace")
        if self.need > 0:
            assert not bool(self.ws[:M.COUNTER_BYTES].any()), "arrival counters are not back at zero"


# ---- route ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", M.INDEX_DTYPES, ids=["int64", "int32"])
@pytest.mark.parametrize("name", list(M.ROUTINGS))
def test_route_equals_the_stable_argsort(hip, name, index_dtype):
    from neural_compressor_amd import _lib, ops

    r = M.ROUTINGS[name]
    idx = M.top_k_index(r, index_dtype)
    assert M.counted(idx, r.E) == list(r.counts)
    ro = M.route_oracle(idx, r.E)
    nbytes = _lib.lib.inc_moe_route_bytes(r.T, r.k, r.E)
    assert nbytes == 4 * M.route_layout(ro["S"], r.E).total
    pad = GUARD // 4
    buf = torch.full((pad + nbytes // 4 + pad,), ROUTE_SENTINEL, dtype=torch.int32, device=hip)
    win = buf[pad:pad + nbytes // 4]
    assert ops.moe_route(idx.to(hip), r.E, route=win) is win
    torch.cuda.synchronize()
    M.assert_route(win.cpu(), ro)
    assert bool((buf[:pad] == ROUTE_SENTINEL).all()) and bool((buf[pad + nbytes // 4:] == ROUTE_SENTINEL).all()), "wrote outside the route buffer"


# ---- GEMM -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.DTYPE_IDS)
@pytest.mark.parametrize("c,mode", M.CASE_MODES, ids=M.CASE_MODE_IDS)
def test_gemm_against_elementwise_oracle(hip, c, mode, dtype):
    r, ro, route = _routing(hip, c.routing)
    S, N, K = r.T * r.k, M.n_of(c, mode), c.K
    ex = M.make_experts(r.E, N, K, c.group_size)
    assert M.splitk_from_workspace(M.workspace_bytes(mode, r.T, r.k, r.E, N, K), S, N) == c.splitk, "the case moved off its K-slice count"
    rw = M.make_routing_weights(r.T, r.k) if mode == 1 else None
    a = M.make_x(S, K, dtype, seed=1) if mode == 1 else M.make_x(r.T, K, dtype)
    ref, tol = M.gemm_reference(mode, ro, ex, a, dtype, rw=rw)
    if mode == 0:
        assert bool(torch.isfinite(ref.to(dtype).float()).all())
    g = _Gemm(hip, mode, r, ro, route, ex, a, dtype, rw=rw)
    first = g()
    g.check_untouched()
    y = g.out[:ro["nvalid"]].cpu()
    ratio = M.worst_ratio(y, ref, tol)[0]
    name = f"{c.name} mode {mode}"
    print(f"\n[moe stages] {name} {M.DTYPE_IDS[M.DTYPES.index(dtype)]} splitk {c.splitk}: worst err / tol {ratio:.3f}")
    _note(f"gemm{mode}", dtype, ratio, c.name)
    M.assert_elementwise(y, ref, tol, name)
    second = g()
    g.check_untouched()
    assert torch.equal(first, second), "a second call into the same workspace is not bit-identical"


@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.DTYPE_IDS)
@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16, torch.float16], ids=["w_fp32", "w_bf16", "w_fp16"])
def test_routing_weight_dtypes(hip, wdtype, dtype):
    c = M.case("k480_split")
    r, ro, route = _routing(hip, c.routing)
    ex = M.make_experts(r.E, c.Nout, c.K, c.group_size)
    rw = M.make_routing_weights(r.T, r.k, wdtype)
    assert rw.dtype is wdtype and torch.equal(rw.float(), M.make_routing_weights(r.T, r.k))  # exact in every weight type
    a = M.make_x(r.T * r.k, c.K, dtype, seed=1)
    ref, tol = M.gemm_reference(1, ro, ex, a, dtype, rw=rw)
    g = _Gemm(hip, 1, r, ro, route, ex, a, dtype, rw=rw)
    g()
    g.check_untouched()
    _note("gemm1", dtype, M.assert_elementwise(g.out[:ro["nvalid"]].cpu(), ref, tol, f"routing weights {wdtype}"), f"k480_split {wdtype}")


@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.DTYPE_IDS)
def test_modes_0_and_1_share_one_workspace(hip, dtype):
    """gate_up with 4 strips and 3 K slices, then down with 2 strips and 4 K slices, on 31 tiles: the counters of (tile, strip) sit at
    tile * strips + strip, so the two calls use overlapping counter ranges with another meaning, and the slabs overlap too."""
    r, ro, route = _routing(hip, "many_rows")
    c0 = M.case("multi_chunk")
    gu = M.make_experts(r.E, 2 * c0.Nout, c0.K, c0.group_size)
    dn = M.make_experts(r.E, 264, 480, 32)
    x, h = M.make_x(r.T, c0.K, dtype), M.make_x(r.T * r.k, 480, dtype, seed=1)
    rw = M.make_routing_weights(r.T, r.k)
    need = [M.workspace_bytes(0, r.T, r.k, r.E, gu["N"], gu["K"]), M.workspace_bytes(1, r.T, r.k, r.E, dn["N"], dn["K"])]
    assert M.splitk_from_workspace(need[0], r.T * r.k, gu["N"]) == 3 and M.splitk_from_workspace(need[1], r.T * r.k, dn["N"]) == 4
    ws_buf, ws = _window(hip, max(need), WS_SENTINEL)
    ws.zero_()
    shared = [_Gemm(hip, 0, r, ro, route, gu, x, dtype, ws=ws), _Gemm(hip, 1, r, ro, route, dn, h, dtype, rw=rw, ws=ws)]
    own = [_Gemm(hip, 0, r, ro, route, gu, x, dtype), _Gemm(hip, 1, r, ro, route, dn, h, dtype, rw=rw)]
    for rounds in range(2):  # the second round starts from the workspace the first one left
        for a, b in zip(shared, own):
            ya, yb = a(), b()
            a.check_untouched()
            b.check_untouched()
            assert torch.equal(ya, yb), f"mode {a.mode} differs between a shared workspace and its own (round {rounds})"
    _guards_intact(ws_buf, max(need), WS_SENTINEL, "the shared workspace")


# ---- no valid id ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.DTYPE_IDS)
def test_all_invalid_routing_writes_nothing(hip, dtype):
    from neural_compressor_amd import ops

    r, ro, _ = _routing(hip, "all_invalid")
    assert ro["ntiles"] == 0 and ro["nvalid"] == 0
    route = ops.moe_route(M.top_k_index(r).to(hip), r.E)  # the route kernel's own buffer: tile-table entries are whatever was there
    torch.cuda.synchronize()
    M.assert_route(route.cpu(), ro)
    S = r.T * r.k
    for mode, ex, a in ((0, M.make_experts(r.E, 520, 480, 32), M.make_x(r.T, 480, dtype)),
                        (1, M.make_experts(r.E, 264, 480, 32), M.make_x(S, 480, dtype, seed=1))):
        g = _Gemm(hip, mode, r, ro, route, ex, a, dtype, rw=M.make_routing_weights(r.T, r.k) if mode == 1 else None)
        assert g.need > 0
        g()
        g.check_untouched()  # nvalid = 0: every row of out is past the valid slots
        assert not bool(g.ws.any()), "the workspace was written"
    y = torch.full((S, 264), float("nan"), device=hip)
    out_buf, win = _window(hip, r.T * 264 * 2, OUT_SENTINEL)
    out = ops.moe_combine(y, route, r.T, r.k, r.E, dtype, out=win.view(dtype).view(r.T, 264))
    torch.cuda.synchronize()
    assert not bool(out.view(torch.int16).any()), "combine of no valid slot is not exact (+0) zeros"
    _guards_intact(out_buf, r.T * 264 * 2, OUT_SENTINEL, "out")


# ---- combine ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.DTYPE_IDS)
@pytest.mark.parametrize("H", [264, 4])
def test_combine_is_exact(hip, H, dtype):
    from neural_compressor_amd import ops

    r, ro, route = _routing(hip, "edges")
    S = r.T * r.k
    y = torch.randn(S, H, generator=torch.Generator().manual_seed(11 + H)) * 3.0
    y[ro["nvalid"]:] = float("nan")  # positions past the valid slots: never read
    want = M.combine_oracle(y, ro, dtype)
    out_buf, win = _window(hip, r.T * H * 2, OUT_SENTINEL)
    out = ops.moe_combine(y.to(hip), route, r.T, r.k, r.E, dtype, out=win.view(dtype).view(r.T, H))
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isfinite(got.float()).all()), "combine read a row past the valid slots"
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        t, j = (int(v) for v in bad[0])
        raise AssertionError(f"combine: {bad.shape[0]} elements differ; out[{t}, {j}] = {float(got[t, j])!r}, expected {float(want[t, j])!r}")
    _guards_intact(out_buf, r.T * H * 2, OUT_SENTINEL, "out")


# ---- the whole forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", M.DTYPES, ids=M.DTYPE_IDS)
def test_module_forward_against_chained_oracle(hip, monkeypatch, dtype):
    """MI355XWeightOnlyExperts.forward at H = 288 (down: strip tail of 32 columns, gate_up: 9 K steps), I = 160 (gate_up: one strip of 160
    columns, down: 5 K steps), gs = 32, on the edges routing, against moe_stage_cases.chain_reference."""
    from neural_compressor_amd.torch.algorithms.weight_only.experts import MI355XWeightOnlyExperts

    E, H, I, gs = 8, 288, 160, 32
    r, ro, _ = _routing(hip, "edges")
    gu, dn = M.make_experts(E, 2 * I, H, gs), M.make_experts(E, H, I, gs)
    m = MI355XWeightOnlyExperts(E, H, I, bits=4, group_size=gs, device=hip)
    for prefix, ex in (("gate_up", gu), ("down", dn)):
        for part, buf in zip(("qweight", "scales", "qzeros"), m._bufs(prefix)):
            assert buf.shape == ex[part].shape
            buf.copy_(torch.from_numpy(ex[part]))
    assert m._fusable() and r.T * r.k <= m.MOE_MAX_ROWS * E

    def boom(*a, **k):
        raise AssertionError("recover(): the forward left the fused route")

    monkeypatch.setattr(MI355XWeightOnlyExperts, "recover", boom)
    x, rw = M.make_x(r.T, H, dtype), M.make_routing_weights(r.T, r.k)
    ref, tol = M.chain_reference(x, ro, rw, gu, dn, dtype)
    with torch.no_grad():
        y = m(x.to(hip), M.top_k_index(r).to(hip), rw.to(hip))
    torch.cuda.synchronize()
    assert y.dtype is dtype and y.shape == (r.T, H)
    _note("forward", dtype, M.assert_elementwise(y.cpu(), ref, tol, "experts forward"), "H 288 I 160 gs 32 edges")
