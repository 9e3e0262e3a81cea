"""Shared by tests/test_moe_stages_cpu.py and tests/test_gpu_moe_stages.py (a helper module, not a conftest): the stages of the fused MoE
experts forward (neural_compressor_amd/csrc/gemm_moe.hip: route, grouped dequant-GEMM in three modes, combine), each against an oracle
of its own so that the stages fail independently.

  * ROUTINGS: deterministic top_k_index tensors with an exact number of slots per expert (never drawn from topk(softmax): a case cannot
    drift off its edge), in int64 and int32.
  * CASES: the GEMM shapes, one or more per branch of woq_moe_gemm_kernel, each with the K-slice count moe_plan gives it.  A retune of
    moe_plan moves a case off its branch: move the shape so that the branch keeps a case, never drop the case.
  * packed experts (oracle.woq_oracle packing, the scale / zero-point pattern of gemm_route_cases.make_layer plus an expert-dependent
    offset, so that reading expert e +- 1, a neighbouring column or the other half of gate_up is visible), activations, routing weights;
  * the oracles: the route buffer from a stable argsort (exact), the GEMM modes in float64 with a per-element bound, combine in fp32 in
    slot order (exact), and the chained forward with the per-stage bounds carried along.

Bounds (float64, per output element; none of them is taken from a kernel's output).  d(K, A) = 2 (K + 5) 2^-24 A with
A = sum_k |a_k| |W_k|: products of two 16-bit values are exact in fp32, any order of K fp32 additions errs by at most K 2^-24 A, the
factor 2 and the + 5 cover the slab re-sum of split-K and the routing-weight product.
    modes 2 and 1   |y - ref| <= |w| d(K, A)                    (fp32 output, no output rounding; w = 1 in mode 2)
    mode 0          |h - ref| <= u_out |ref| + 1.1 dg (|u| + du) + |g| du + 2^-20 |ref| + tiny,   ref = silu(g) u
                    (|silu'| <= 1.1, |silu(g)| <= |g|; 2^-20 = a few fp32 ulp for expf, the divide and the product; u_out and tiny
                    as in gemm_route_cases.tolerance: one rounding to the output type)
    combine         exact
"""

import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import woq_oracle as O  # noqa: E402

MOE_BM, MOE_BN = 64, 256      # rows per tile, columns per strip (gemm_moe.hip)
COUNTER_BYTES = 4096          # split-K arrival counters at the start of the workspace
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "fp16"]
INDEX_DTYPES = [torch.int64, torch.int32]


# ---------------------------------------------------------------------------------------------------------------------------------------
# routings
# ---------------------------------------------------------------------------------------------------------------------------------------
Routing = collections.namedtuple("Routing", "name T k E flat counts")  # flat: python list of S ids; counts: expected, per expert


def _spread(ids, stride, shift):
    """ids placed at (i * stride + shift) % S: experts interleave, so the sort has work to do."""
    S = len(ids)
    assert np.gcd(stride, S) == 1
    flat = [None] * S
    for i, e in enumerate(ids):
        flat[(i * stride + shift) % S] = e
    return flat


def _edges():
    """E = 8, S = 200 (S % 64 = 8): a full tile plus one row, exactly one tile, an idle expert, one row, the 16 / 17 row-block skip boundary,
    an idle expert, the rest; 9 invalid slots (ids -1 and E)."""
    counts = [65, 64, 0, 1, 16, 17, 0, 28]
    ids = [e for e, c in enumerate(counts) for _ in range(c)] + [-1] * 5 + [8] * 4
    return Routing("edges", 100, 2, 8, _spread(ids, 37, 11), counts)


def _edges3():
    """E = 3, S = 140 (the shape the GEMM case table was planned at): a full tile plus one row, an idle expert, a tile plus 6 rows (no
    skipped row block in its second tile but three); 5 invalid slots."""
    counts = [65, 0, 70]
    ids = [e for e, c in enumerate(counts) for _ in range(c)] + [-1] * 3 + [3] * 2
    return Routing("edges3", 70, 2, 3, _spread(ids, 37, 11), counts)


def _short_waves():
    """S = 17: the route kernel's 16 waves own seg = 2 slots each, so waves 9..15 own nothing (wave 8 owns one)."""
    flat = [i % 3 for i in range(17)]
    flat[5] = -1
    return Routing("short_waves", 17, 1, 4, flat, [6, 6, 4, 0])


def _max_experts():
    """E = 512 > S = 40: 38 experts with one slot, the last expert with two."""
    flat = [(i * 13) % 512 for i in range(38)] + [511, 511]
    counts = [0] * 512
    for e in flat:
        counts[e] += 1
    return Routing("max_experts", 20, 2, 512, flat, counts)


def _many_rows():
    """S = 1920 over two experts: 16 tiles (15 full and one row) and 15 tiles (the last with 63 rows)."""
    flat = [i % 2 for i in range(1920)]
    flat[1] = 0
    return Routing("many_rows", 960, 2, 2, flat, [961, 959])


ROUTINGS = collections.OrderedDict((r.name, r) for r in (
    _edges(),
    _edges3(),
    Routing("one_slot", 1, 1, 4, [2], [0, 0, 1, 0]),
    _short_waves(),
    Routing("all_invalid", 10, 2, 8, [-1, 8] * 10, [0] * 8),
    _max_experts(),
    _many_rows(),
    Routing("spread", 256, 2, 128, [(i * 37) % 128 for i in range(512)], [4] * 128),  # every expert four slots, none adjacent
))


def top_k_index(r, index_dtype=torch.int64):
    """top_k_index [T, k] of routing r (CPU)."""
    return torch.tensor(r.flat, dtype=index_dtype).view(r.T, r.k)


def counted(idx, E):
    """Per-expert counts of the valid ids of idx, on the CPU (what every test asserts before a launch)."""
    flat = idx.reshape(-1).long()
    return torch.bincount(flat[(flat >= 0) & (flat < E)], minlength=E).tolist()


# ---------------------------------------------------------------------------------------------------------------------------------------
# route oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
RouteLayout = collections.namedtuple("RouteLayout", "offsets order pos tiles total")  # int32 offsets inside the route buffer


def tiles_max(S, E):
    return -(-S // MOE_BM) + min(E, S)


def route_layout(S, E):
    """include/inc_mi355x.h, K4e: [0] tile count, offsets [E + 1], order [S], pos [S], tiles [2 * (ceil(S / 64) + min(E, S))]."""
    offsets = 1
    order = offsets + E + 1
    pos = order + S
    tiles = pos + S
    return RouteLayout(offsets, order, pos, tiles, tiles + 2 * tiles_max(S, E))


def route_oracle(idx, E):
    """The route of top_k_index idx [T, k] from a stable argsort of the bucket ids (ids outside 0..E-1 go to bucket E, after every
    expert): offsets [E + 1], order [S] (ascending flat slot inside a bucket), pos [S], the tile table [(expert, first position)] with
    ceil(count / 64) tiles per expert in expert order."""
    T, k = idx.shape
    flat = idx.reshape(-1).long()
    S = flat.numel()
    bucket = torch.where((flat >= 0) & (flat < E), flat, torch.full_like(flat, E))
    order = torch.argsort(bucket, stable=True)
    pos = torch.empty(S, dtype=torch.int64)
    pos[order] = torch.arange(S)
    counts = torch.bincount(bucket, minlength=E + 1)
    offsets = torch.zeros(E + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)[:E]
    tiles = [(e, int(offsets[e]) + MOE_BM * j) for e in range(E) for j in range(-(-int(counts[e]) // MOE_BM))]
    return dict(T=T, k=k, S=S, E=E, offsets=offsets.int(), order=order.int(), pos=pos.int(), counts=counts[:E].tolist(),
                tiles=torch.tensor(tiles, dtype=torch.int32).view(-1, 2), ntiles=len(tiles), nvalid=int(offsets[E]))


def route_buffer(ro, fill=0):
    """The int32 buffer inc_moe_route writes for oracle ro; tile-table entries past the tile count (unspecified) are `fill`."""
    L = route_layout(ro["S"], ro["E"])
    buf = torch.full((L.total,), fill, dtype=torch.int32)
    buf[0] = ro["ntiles"]
    buf[L.offsets:L.order] = ro["offsets"]
    buf[L.order:L.pos] = ro["order"]
    buf[L.pos:L.tiles] = ro["pos"]
    buf[L.tiles:L.tiles + 2 * ro["ntiles"]] = ro["tiles"].reshape(-1)
    return buf


def assert_route(buf, ro):
    """buf (int32, CPU) equals the oracle over the defined regions: the tile count, offsets, order, pos and the first `count` tiles."""
    L = route_layout(ro["S"], ro["E"])
    assert buf.dtype is torch.int32 and buf.numel() >= L.total
    assert int(buf[0]) == ro["ntiles"], f"route[0] = {int(buf[0])} tiles, expected {ro['ntiles']}"
    for name, lo, hi, want in (("offsets", L.offsets, L.order, ro["offsets"]), ("order", L.order, L.pos, ro["order"]),
                               ("pos", L.pos, L.tiles, ro["pos"]),
                               ("tiles", L.tiles, L.tiles + 2 * ro["ntiles"], ro["tiles"].reshape(-1))):
        got = buf[lo:hi]
        if not torch.equal(got, want):
            i = int(torch.nonzero(got != want)[0])
            raise AssertionError(f"route {name}[{i}] = {int(got[i])}, expected {int(want[i])} ({int((got != want).sum())} entries differ)")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GEMM cases
# ---------------------------------------------------------------------------------------------------------------------------------------
# Nout: output columns (N = 2 * Nout in mode 0); splitk: what moe_plan gives for (routing, Nout, K) -- the same in every mode of a case
Case = collections.namedtuple("Case", "name routing modes Nout K group_size splitk pins")

CASES = [
    Case("k32_n8", "edges3", (2,), 8, 32, -1, 1, "one K step, Nout < 256 (one strip, lanes past column 7 clamp to Nout - 4), G4 with one group"),
    Case("k96_tail", "edges3", (2, 1), 264, 96, 32, 1, "one pass whose only chunk is ragged (3 of 4 steps), strip tail of 8 columns"),
    Case("k480_split", "edges3", (2, 1), 264, 480, 32, 4, "ragged last K slice (3 steps), per-step group parameters (non-G4, gs 32)"),
    Case("k480_split_g1", "edges3", (2, 1), 264, 480, -1, 4, "ragged last K slice (3 steps), G4 with one group per row (gs -1)"),
    Case("k640_g128", "edges3", (2, 1), 264, 640, 128, 5, "G4 with real groups (gs 128): one group per 4-step chunk, 5 slices"),
    Case("k512_g64", "edges3", (2,), 264, 512, 64, 4, "non-G4 with two steps per group (gs 64)"),
    Case("gu_nibble4", "edges3", (0,), 260, 480, 32, 4, "Nout % 8 == 4: up-stream zero points at nibble 4, strip tail of 4 columns, split-K"),
    Case("gu_onepass", "edges3", (0,), 260, 96, -1, 1, "up-stream zero points at nibble 4 in one pass, G4, ragged chunk"),
    Case("multi_chunk", "many_rows", (2, 0), 776, 1056, 32, 3, "slices of 12 steps (three chunks), last slice 9 steps (two chunks and one step)"),
    Case("units_512", "spread", (2,), 1024, 480, 32, 1, "no split because (tile slot, strip) pairs reach 512, K above one chunk"),
    Case("max_e", "max_experts", (2,), 264, 480, 32, 4, "E = 512 (E > S): one-row tiles, most tile slots idle"),
    # the edges routing (E = 8, S = 200): 16 / 17-row tiles, an exactly full tile, idle experts between busy ones
    Case("k96_tail_e8", "edges", (2, 1), 264, 96, 32, 1, "k96_tail on the edges routing: row-block skip at 16 / 17 rows, one-row tile"),
    Case("k480_split_e8", "edges", (2, 1), 264, 480, 32, 4, "k480_split on the edges routing"),
    Case("gu_nibble4_e8", "edges", (0,), 260, 480, 32, 4, "gu_nibble4 on the edges routing"),
]
CASE_MODES = [(c, m) for c in CASES for m in c.modes]
CASE_MODE_IDS = [f"{c.name}-mode{m}" for c, m in CASE_MODES]


def case(name):
    return next(c for c in CASES if c.name == name)


def n_of(c, mode):
    return 2 * c.Nout if mode == 0 else c.Nout


def plan_splitk(mode, S, E, N, K):
    """K slices of moe_plan, restated from its description: about 512 workgroups counting every tile slot, whole 4-step chunks per
    slice, at least one chunk, no split once the (tile slot, strip) pairs alone reach 512."""
    Nout = N // 2 if mode == 0 else N
    units = -(-Nout // MOE_BN) * tiles_max(S, E)
    steps = K // 32
    want = 1 if units >= 512 else -(-512 // units)
    want = max(1, min(want, -(-steps // 4)))
    per = -(-(-(-steps // want)) // 4) * 4
    return -(-steps // per)


def splitk_from_workspace(nbytes, S, N):
    """(bytes - 4096) / (S N 4), or 0 bytes => 1."""
    if nbytes == 0:
        return 1
    q, rem = divmod(nbytes - COUNTER_BYTES, S * N * 4)
    assert rem == 0 and q > 1, nbytes
    return q


def workspace_bytes(mode, T, k, E, N, K):
    from neural_compressor_amd import _lib

    return _lib.lib.inc_woq_moe_gemm_workspace_bytes(mode, T, k, E, N, K)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
_experts = {}


def make_experts(E, N, K, group_size):
    """E packed INT4 layers in the optimum layout stacked on the expert axis (numpy): qweight [E, K/8, N] int32, scales [E, G, N] fp16,
    qzeros [E, G, N/8] int32.  Asymmetric; scale and zero point of (expert e, column n, group g) follow gemm_route_cases.make_layer's
    pattern (strides 7 / 5 along n, 3 along g through 41 / 16 values) shifted by 11 e / 7 e, so a neighbouring expert, column or
    group differs clearly, and so do the gate and the up half of a gate_up matrix.  Experts are packed as rows of one tall layer
    (N % 8 == 0: no packed word straddles two experts), a few at a time.  Cached: the tests share it and must not write to it."""
    key = (E, N, K, group_size)
    if key in _experts:
        return _experts[key]
    assert N % 8 == 0 and K % 32 == 0
    rng = np.random.default_rng(1000003 * N + 1009 * K + 17 * group_size + 131 * E)
    G = 1 if group_size == -1 or group_size >= K else K // group_size
    step = max(1, (1 << 22) // (N * K))
    qw, sc, qz = [], [], []
    for e0 in range(0, E, step):
        ne = min(step, E - e0)
        e = np.repeat(np.arange(e0, e0 + ne), N)[:, None]
        n = np.tile(np.arange(N), ne)[:, None]
        g = np.arange(G)[None, :]
        scales = (0.004 * (1.0 + 0.05 * ((7 * n + 3 * g + 11 * e) % 41))).astype(np.float32)
        zp = (5 * n + 3 * g + 7 * e) % 16
        iw = rng.integers(0, 16, size=(ne * N, K), dtype=np.int8)
        q, z, s = O.woq_pack_optimum(iw, scales, zp, 4)  # [K/8, ne N], [G, ne N/8], [G, ne N]
        qw.append(q.reshape(K // 8, ne, N).transpose(1, 0, 2))
        qz.append(z.reshape(G, ne, N // 8).transpose(1, 0, 2))
        sc.append(s.reshape(G, ne, N).transpose(1, 0, 2))
    ex = dict(E=E, N=N, K=K, G=G, group_size=group_size, qweight=np.ascontiguousarray(np.concatenate(qw)),
              scales=np.ascontiguousarray(np.concatenate(sc)), qzeros=np.ascontiguousarray(np.concatenate(qz)))
    _experts[key] = ex
    return ex


def dense_expert64(ex, e, dtype):
    """Expert e's dense weight [N, K] as the kernels decode it (oracle.woq_dense_weight, compute dtype = x dtype), in float64."""
    gs = ex["K"] if ex["G"] == 1 else ex["group_size"]
    return O.woq_dense_weight(ex["qweight"][e], ex["scales"][e], ex["qzeros"][e], ex["N"], ex["K"], 4, gs, compute_dtype=dtype).double()


def make_x(rows, K, dtype, seed=0):
    """Activations [rows, K] with a few large entries, already rounded to dtype (as gemm_route_cases.make_x; `seed` tells the mode-1
    input h, which is test data in the route's sorted order and not the kernel's own mode-0 output, from x)."""
    g = torch.Generator().manual_seed(7919 * rows + K + 104729 * seed)
    x = torch.randn(rows, K, generator=g)
    flat = x.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[: max(4, flat.numel() // 512)]] *= 12.0
    return x.to(dtype)


def make_routing_weights(T, k, dtype=torch.float32):
    """[T, k], distinct per flat slot among neighbours: a permuted ramp of multiples of 1/128 in [0.25, 1.04), exact in bf16, fp16 and
    fp32, so rw[order[p]] and rw[p] differ wherever p - order[p] is no multiple of 101."""
    i = torch.arange(T * k, dtype=torch.float32)
    return (0.25 + ((i * 37) % 101) / 128.0).to(dtype).view(T, k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GEMM oracle and comparator
# ---------------------------------------------------------------------------------------------------------------------------------------
def accum_bound(K, A):
    return 2.0 * (K + 5) * 2.0 ** -24 * A


def out_rounding(dtype):
    """(u_out, tiny) of gemm_route_cases.tolerance."""
    return (2.0 ** -8, 0.0) if dtype is torch.bfloat16 else (2.0 ** -11, 2.0 ** -24)


def silu64(g):
    return g / (1.0 + torch.exp(-g))


def mode0_tolerance(g, u, dg, du, dtype):
    u_out, tiny = out_rounding(dtype)
    ref = silu64(g) * u
    return ref, u_out * ref.abs() + 1.1 * dg * (u.abs() + du) + g.abs() * du + 2.0 ** -20 * ref.abs() + tiny


def gemm_reference(mode, ro, ex, a, dtype, rw=None, dense=dense_expert64):
    """(ref, tol) in float64 over the valid positions [nvalid, Nout] of the route's sorted order.
    modes 0 / 2: a = x [T, K], row p is x[order[p] // k]; mode 1: a [S, K] in sorted order, row p is a[p], scaled by rw.view(-1)[order[p]].
    `dense(ex, e, dtype)` supplies expert e's weight (the CPU self-test swaps in mutated weights)."""
    K, N = ex["K"], ex["N"]
    Nout = N // 2 if mode == 0 else N
    nvalid, order = ro["nvalid"], ro["order"].long()
    ref = torch.zeros(nvalid, Nout, dtype=torch.float64)
    tol = torch.zeros(nvalid, Nout, dtype=torch.float64)
    a64 = a.double()
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo == hi:
            continue
        rows = a64[lo:hi] if mode == 1 else a64[order[lo:hi] // ro["k"]]
        w = dense(ex, e, dtype)
        acc, A = rows @ w.t(), rows.abs() @ w.abs().t()
        d = accum_bound(K, A)
        if mode == 0:
            ref[lo:hi], tol[lo:hi] = mode0_tolerance(acc[:, :Nout], acc[:, Nout:], d[:, :Nout], d[:, Nout:], dtype)
        elif mode == 1:
            wt = rw.reshape(-1).double()[order[lo:hi]][:, None]
            ref[lo:hi], tol[lo:hi] = wt * acc, wt.abs() * d
        else:
            ref[lo:hi], tol[lo:hi] = acc, d
    return ref, tol


def worst_ratio(y, ref, tol):
    """max over the elements of |y - ref| / tol and where (0 / 0 counts as 0, a non-finite output as infinitely wrong)."""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0, (0, 0)
    err = (y.double().cpu() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    idx = int(torch.argmax(ratio))
    return float(ratio.view(-1)[idx]), divmod(idx, ref.shape[1])


def assert_elementwise(y, ref, tol, what=""):
    r, (i, j) = worst_ratio(y, ref, tol)
    assert r <= 1.0, (f"{what}: element ({i}, {j}) is off by {r:.3g} x its bound: got {float(y[i, j])!r}, reference {float(ref[i, j])!r}, "
                      f"bound {float(tol[i, j])!r}")
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------
# combine oracle, chained forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def combine_oracle(y, ro, dtype):
    """Exact: fp32 accumulation from zero over s = 0 .. k-1 in order, valid slots only, one rounding to dtype.  y [S, H] fp32 (CPU)."""
    T, k, nvalid = ro["T"], ro["k"], ro["nvalid"]
    pos = ro["pos"].long().view(T, k)
    acc = torch.zeros(T, y.shape[1], dtype=torch.float32)
    for s in range(k):
        p = pos[:, s]
        ok = p < nvalid
        acc[ok] = acc[ok] + y[p[ok]]
    return acc.to(dtype)


def chain_reference(x, ro, rw, gate_up, down, dtype):
    """combine-oracle(mode-1-oracle(mode-0-oracle(x))) in float64 with the per-stage bounds carried forward -> (ref, tol) [T, H].

      h    = h_ref + eh,  |eh| <= th (mode 0's bound, output rounding included)
      y    = w (h . Wd) computed in fp32: |y - y_ref| <= ty = |w| (th . |Wd|) + |w| d(I, (|h_ref| + th) . |Wd|)
      out  = rd(sum_s y_s), k fp32 additions from zero: |sum - ref| <= ea = sum_s ty_s + k 2^-24 sum_s (|y_ref_s| + ty_s)
      |out - ref| <= ea + u_out (|ref| + ea) + tiny                                                   (one rounding to dtype)
    """
    T, k, nvalid, order = ro["T"], ro["k"], ro["nvalid"], ro["order"].long()
    h_ref, th = gemm_reference(0, ro, gate_up, x, dtype)
    H = down["N"]
    y_ref = torch.zeros(nvalid, H, dtype=torch.float64)
    ty = torch.zeros(nvalid, H, dtype=torch.float64)
    for e in range(ro["E"]):
        lo, hi = int(ro["offsets"][e]), int(ro["offsets"][e + 1])
        if lo == hi:
            continue
        w = dense_expert64(down, e, dtype)
        wt = rw.reshape(-1).double()[order[lo:hi]][:, None]
        y_ref[lo:hi] = wt * (h_ref[lo:hi] @ w.t())
        ty[lo:hi] = wt.abs() * (th[lo:hi] @ w.abs().t() + accum_bound(down["K"], (h_ref[lo:hi].abs() + th[lo:hi]) @ w.abs().t()))
    pos = ro["pos"].long().view(T, k)
    ref = torch.zeros(T, H, dtype=torch.float64)
    ea = torch.zeros(T, H, dtype=torch.float64)
    mag = torch.zeros(T, H, dtype=torch.float64)
    for s in range(k):
        p = pos[:, s]
        ok = p < nvalid
        ref[ok] += y_ref[p[ok]]
        ea[ok] += ty[p[ok]]
        mag[ok] += y_ref[p[ok]].abs() + ty[p[ok]]
    ea = ea + k * 2.0 ** -24 * mag
    u_out, tiny = out_rounding(dtype)
    return ref, ea + u_out * (ref.abs() + ea) + tiny
