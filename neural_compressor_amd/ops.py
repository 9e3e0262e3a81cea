"""Tensor-level wrappers over the C-ABI (device memory and streams come from PyTorch-ROCm, arithmetic does not).

Every function takes torch tensors that already live in HBM (`device.type == "cuda"`, i.e. HIP on ROCm),
passes `data_ptr()` + sizes + the current HIP stream to libinc_mi355x.so and returns torch tensors.
Host tensors are rejected: there is no CPU path.
"""

import torch

from ._lib import INC_BF16, INC_F16, INC_F32, INC_SCHEME_ASYM, INC_SCHEME_SYM, check, lib

_DT = {torch.float32: INC_F32, torch.float16: INC_F16, torch.bfloat16: INC_BF16}


def dtype_code(dtype):
    try:
        return _DT[dtype]
    except KeyError as e:
        raise TypeError(f"unsupported floating dtype {dtype}; expected fp32/fp16/bf16") from e


def _dev(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                f"MI355X op got a tensor on {t.device}; tensors must be resident in HBM (device 'cuda' = HIP). "
                "There is no CPU fallback."
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
        if not t.is_contiguous():
            raise RuntimeError("MI355X ops need contiguous tensors")
    return dev


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------
# K1/K2 generic row packers
# ---------------------------------------------------------------------------------------------------
_CT = {8: torch.int8, 16: torch.int16, 32: torch.int32, 64: torch.int64}


def pack_rows(raw, bits, compress_bits):
    """== INCWeightOnlyLinear.pack_tensor (modules.py:580): [R,C] ints -> [R, ceil(C/n_pack)] words."""
    raw = raw.to(torch.int32).contiguous()
    dev = _dev(raw)
    n_pack = compress_bits // bits
    rows, cols = raw.shape
    out = torch.empty((rows, (cols + n_pack - 1) // n_pack), dtype=_CT[compress_bits], device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_pack_rows(_ptr(raw), _ptr(out), rows, cols, bits, compress_bits, _stream()), "inc_pack_rows")
    return out


def unpack_rows(packed, bits, compress_bits, mask_sign):
    """== INCWeightOnlyLinear.unpack_tensor (modules.py:587): -> int16 [R, C*n_pack]."""
    packed = packed.contiguous()
    dev = _dev(packed)
    n_pack = compress_bits // bits
    rows, pcols = packed.shape
    out = torch.empty((rows, pcols * n_pack), dtype=torch.int16, device=dev)
    with torch.cuda.device(dev):
        check(
            lib.inc_unpack_rows(_ptr(packed), _ptr(out), rows, pcols, bits, compress_bits, int(bool(mask_sign)), _stream()),
            "inc_unpack_rows",
        )
    return out


# ---------------------------------------------------------------------------------------------------
# optimum-format pack / unpack / recover
# ---------------------------------------------------------------------------------------------------
def woq_pack(int_weight, scales, zp, bits, shift, qweight=None, qzeros=None, scales_out=None):
    """== INCWeightOnlyLinear.pack (optimum format, modules.py:321-375).

    int_weight [N,K] int32 or int8/uint8; scales [N,G] fp32; zp [N,G] int32 or None (sym -> `shift`).
    Returns (qweight [K/np, N] int32, qzeros [G, N/np] int32, scales fp16 [G, N]).
    """
    N, K = int_weight.shape
    G = scales.shape[1]
    n_pack = 32 // bits
    if int_weight.dtype in (torch.int8, torch.uint8):
        in_bytes = 1
    else:
        int_weight = int_weight.to(torch.int32)
        in_bytes = 4
    int_weight = int_weight.contiguous()
    scales = scales.to(torch.float32).contiguous()
    zp = None if zp is None else zp.to(torch.int32).contiguous()
    dev = _dev(int_weight, scales, zp)
    if qweight is None:
        qweight = torch.empty(((K + n_pack - 1) // n_pack, N), dtype=torch.int32, device=dev)
    if qzeros is None:
        qzeros = torch.empty((G, (N + n_pack - 1) // n_pack), dtype=torch.int32, device=dev)
    if scales_out is None:
        scales_out = torch.empty((G, N), dtype=torch.float16, device=dev)
    _dev(qweight, qzeros, scales_out)
    with torch.cuda.device(dev):
        check(
            lib.inc_woq_pack(
                _ptr(int_weight), in_bytes, _ptr(scales), _ptr(zp), _ptr(qweight), _ptr(qzeros), _ptr(scales_out),
                N, K, G, bits, shift, _stream(),
            ),
            "inc_woq_pack",
        )
    return qweight, qzeros, scales_out


def woq_unpack(qweight, qzeros, N, K, G, bits, want_weight=True, want_zp=True, scales=None):
    """== INCWeightOnlyLinear.unpack (modules.py:377-411): (int_weight [N,K] int16, zp [N,G] int16).  `scales` [G,N] fp16 (optional,
    with the weights): a third result, the scales as [N,G] (`scales.T.contiguous()`, modules.py:382), written by the same launch."""
    dev = _dev(qweight, qzeros, scales)
    iw = torch.empty((N, K), dtype=torch.int16, device=dev) if want_weight else None
    zp = torch.empty((N, G), dtype=torch.int16, device=dev) if want_zp else None
    sc_t = None
    if scales is not None:
        assert want_weight and scales.dtype == torch.float16 and scales.shape == (G, N) and scales.is_contiguous()
        sc_t = torch.empty((N, G), dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        check(
            lib.inc_woq_unpack(_ptr(qweight), _ptr(qzeros), _ptr(iw), _ptr(zp), N, K, G, bits, _ptr(scales), _ptr(sc_t), _stream()),
            "inc_woq_unpack",
        )
    return (iw, zp) if scales is None else (iw, zp, sc_t)


def awq_repack(awq_qweight, awq_qzeros, bits=4):
    """AutoAWQ GEMM-format words -> optimum layout (== repack_awq_to_optimum_format, utility.py:1426-1459).
    awq_qweight [K, N/8] int32, awq_qzeros [G, N/8] int32 -> (qweight [K/8, N], qzeros [G, N/8]); scales are shared."""
    dev = _dev(awq_qweight, awq_qzeros)
    assert awq_qweight.dtype == torch.int32 and awq_qzeros.dtype == torch.int32
    awq_qweight, awq_qzeros = awq_qweight.contiguous(), awq_qzeros.contiguous()
    K, NW = awq_qweight.shape
    G = awq_qzeros.shape[0]
    N = NW * (32 // bits)
    qweight = torch.empty((K // (32 // bits), N), dtype=torch.int32, device=dev)
    qzeros = torch.empty((G, NW), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_awq_repack(_ptr(awq_qweight), _ptr(awq_qzeros), K, N, G, bits, _ptr(qweight), _ptr(qzeros), _stream()),
              "inc_awq_repack")
    return qweight, qzeros


def woq_dequant(qweight, scales, qzeros, g_idx, N, K, group_size, bits, out_dtype=torch.float16):
    """== INCWeightOnlyLinear.recover (modules.py:413-443) from the optimum layout -> dense [N,K]."""
    dev = _dev(qweight, scales, qzeros, g_idx)
    assert scales.dtype == torch.float16, "optimum-format scales are fp16 (modules.py:245)"
    G = scales.shape[0]
    out = torch.empty((N, K), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(
            lib.inc_woq_dequant(
                _ptr(qweight), _ptr(scales), _ptr(qzeros), _ptr(g_idx), _ptr(out), dtype_code(out_dtype),
                N, K, G, group_size, bits, _stream(),
            ),
            "inc_woq_dequant",
        )
    return out


def dequant_ints(int_weight, scales, zp, g_idx, group_size, out_dtype):
    """recover() for non-optimum layouts: int16 [N,K], scales [N,G] (any float dtype), zp int16 [N,G] or None."""
    int_weight = int_weight.to(torch.int16).contiguous()
    zp = None if zp is None else zp.to(torch.int16).contiguous()
    scales = scales.contiguous()
    dev = _dev(int_weight, scales, zp, g_idx)
    N, K = int_weight.shape
    G = scales.shape[1]
    out = torch.empty((N, K), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(
            lib.inc_dequant_ints(
                _ptr(int_weight), _ptr(scales), dtype_code(scales.dtype), _ptr(zp), _ptr(g_idx), _ptr(out),
                dtype_code(out_dtype), N, K, G, group_size, _stream(),
            ),
            "inc_dequant_ints",
        )
    return out


# ---------------------------------------------------------------------------------------------------
# K4 fused GEMM
# ---------------------------------------------------------------------------------------------------
_ws_cache = {}


def _workspace(dev, nbytes):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)  # one workspace per (device, stream): see header
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        # zero-filled: the first 16 KiB are the split-K arrival counters of the M <= 16 kernel, which must be zero on
        # first use (the kernel re-arms them); one workspace per (device, stream) so concurrent streams never share them
        if buf is not None:
            # the outgrown buffer stays allocated: a captured graph (or a launch in flight) may still hold its address, and a replay
            # into freed memory is an illegal access.  Growth is rare (sizes are per shape) and the buffers are a few MB.
            _ws_retired.append(buf)
        buf = torch.zeros(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _ws_cache[key] = buf
    return buf


_ws_retired = []


_ws_bytes_cache = {}

_raw_stream = torch._C._cuda_getCurrentRawStream  # (device index) -> hipStream_t of torch's current stream, no Stream object
_cur_device = torch._C._cuda_getDevice


def _ws_lookup(dev, idx, need):
    """(address, bytes, stream) for a launch on torch's current stream of device `dev` (index `idx`) that needs `need` workspace
    bytes: the (device, stream) workspace, grown when it is too small; (None, 0, stream) when the launch needs none."""
    stream = _raw_stream(idx)
    if need <= 0:
        return None, 0, stream
    buf = _ws_cache.get((idx, stream))
    if buf is None or buf.numel() < need:
        buf = _workspace(dev, need)
    return buf.data_ptr(), buf.numel(), stream


def _launch(dev, idx, fn, name, args, may_decline=False):
    """rc = fn(*args), under the device guard only when `dev` (index `idx`) is not the current device; a non-zero rc raises through
    check(rc, name) -- except INC_ERR_UNSUPPORTED (-2: nothing was launched) with `may_decline`, which the caller turns into None."""
    if _cur_device() == idx:
        rc = fn(*args)
    else:
        with torch.cuda.device(dev):
            rc = fn(*args)
    if rc != 0 and not (may_decline and rc == -2):
        check(rc, name)
    return rc


def _check_k_order(k_order, K):
    """An act_order gather order: int32 [K]."""
    if k_order.dtype is not torch.int32:
        raise TypeError(f"k_order must be int32, got {k_order.dtype}")
    if k_order.dim() != 1 or k_order.shape[0] != K:
        raise ValueError(f"k_order must hold K = {K} entries, got {tuple(k_order.shape)}")


def woq_gemm(x2d, qweight, scales, qzeros, bias, N, K, group_size, bits, g_idx=None):
    """y[M,N] = x[M,K] @ dequant(qweight)^T + bias, fused (== INCWeightOnlyLinear.forward, modules.py:594-610).

    This is the decode-path entry (M = 1 runs in ~8 us on the GPU), so the host side is kept lean: argument checks are
    attribute reads, the workspace size is memoised, and the device guard is only entered when the tensor's device is
    not already current."""
    dev = x2d.device
    if dev.type != "cuda" or qweight.device != dev or not x2d.is_contiguous():
        _dev(x2d, qweight, scales, qzeros, bias, g_idx)  # raises the descriptive error
    if x2d.dtype is not torch.bfloat16 and x2d.dtype is not torch.float16:
        raise TypeError("woq_gemm computes in bf16 or fp16")
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    M = x2d.shape[0]
    y = torch.empty((M, N), dtype=x2d.dtype, device=dev)
    key = (M, N, K)
    nbytes = _ws_bytes_cache.get(key)
    if nbytes is None:
        nbytes = _ws_bytes_cache[key] = lib.inc_woq_gemm_workspace_bytes(M, N, K)
    # (M <= 16: arrival counters + split-K partials; medium M: split-K slabs of the 256x256 kernel)
    wp, wn, stream = _ws_lookup(dev, dev.index, nbytes)
    _launch(dev, dev.index, lib.inc_woq_gemm, "inc_woq_gemm", (
        x2d.data_ptr(), INC_BF16 if x2d.dtype is torch.bfloat16 else INC_F16, qweight.data_ptr(), scales.data_ptr(),
        qzeros.data_ptr(), _ptr(g_idx), _ptr(bias), y.data_ptr(), M, N, K, scales.shape[0], group_size, bits, wp, wn, stream))
    return y


def woq_gemm_perm(x2d, k_order, qweight_sorted, scales, qzeros, bias, N, K, group_size, bits):
    """y[M,N] = x[:, k_order] @ dequant(qweight_sorted)^T + bias in ONE launch (inc_woq_gemm_perm: the decode form of act_order /
    HF desc_act modules, reference modules.py:427-431, 594-610).

    `qweight_sorted` is the packed weight with its K axis sorted by group and `k_order` [K] int32 that order (what
    MI355XWeightOnlyLinear builds once per packed state); the activations are gathered inside the decode kernels, entries of
    k_order outside [0, K-1] are clamped.  Bit-identical to woq_gemm(x2d.index_select(1, k_order), qweight_sorted, ...).  Only the
    streaming decode routes have this form (M <= 64; ops.woq_gemm_route says GEMV16 / STREAM_W4 / STREAM_W8 for the shape):
    anything else raises -- gather x and call woq_gemm there, which WoqGemmCall(k_order=...) does by itself."""
    if k_order.dtype is not torch.int32:
        raise TypeError(f"k_order must be int32, got {k_order.dtype}")
    if k_order.dim() != 1 or k_order.shape[0] != K or x2d.dim() != 2 or x2d.shape[1] != K:  # (one message for both shapes)
        raise ValueError(f"k_order must hold K = {K} entries and x2d be [M, {K}]; got {tuple(k_order.shape)} and {tuple(x2d.shape)}")
    dev = x2d.device
    if k_order.device != dev:
        raise RuntimeError(f"tensors on different devices: {dev} vs {k_order.device}")
    if dev.type != "cuda" or qweight_sorted.device != dev or not x2d.is_contiguous():
        _dev(x2d, k_order, qweight_sorted, scales, qzeros, bias)  # raises the descriptive error
    if x2d.dtype is not torch.bfloat16 and x2d.dtype is not torch.float16:
        raise TypeError("woq_gemm computes in bf16 or fp16")
    if bias is not None and bias.dtype != x2d.dtype:
        bias = bias.to(x2d.dtype)
    M = x2d.shape[0]
    y = torch.empty((M, N), dtype=x2d.dtype, device=dev)
    nbytes = _ws_bytes_cache.get((M, N, K))
    if nbytes is None:
        nbytes = _ws_bytes_cache[(M, N, K)] = lib.inc_woq_gemm_workspace_bytes(M, N, K)
    wp, wn, stream = _ws_lookup(dev, dev.index, nbytes)
    _launch(dev, dev.index, lib.inc_woq_gemm_perm, "inc_woq_gemm_perm", (
        x2d.data_ptr(), INC_BF16 if x2d.dtype is torch.bfloat16 else INC_F16, k_order.data_ptr(), qweight_sorted.data_ptr(),
        scales.data_ptr(), qzeros.data_ptr(), _ptr(bias), y.data_ptr(), M, N, K, scales.shape[0], group_size, bits, wp, wn, stream))
    return y


WOQ_GEMM_ROUTES = {
    1: "TILE_ANYW", 2: "STRIP8", 3: "STRIP", 4: "3A2B_W8", 5: "D2R", 6: "3A2B_W4", 7: "BIG", 8: "TILE", 9: "GEMV16", 10: "STREAM_W4",
    11: "STREAM_W8", 12: "SMALL",
}  # INC_WOQ_ROUTE_* of include/inc_mi355x.h


def woq_gemm_route(M, N, K, group_size, bits, dtype, has_g_idx=False, x_ptr=0, y_ptr=0, bias_ptr=0, ws_ptr=None, ws_bytes=0):
    """Which kernel inc_woq_gemm launches for this call (inc_woq_gemm_route: the dispatcher's own decision, computed on the host --
    works without a GPU).  Of the addresses only the alignment is used, of `ws_ptr` only whether it is None.  Returns a dict:
    route (a name of WOQ_GEMM_ROUTES), splitk, row_blocks, steps, y_vec_ok, x_vec_ok, need (workspace bytes the route uses).  Not on
    the forward path: woq_gemm / WoqGemmCall never call it."""
    import ctypes

    o = [ctypes.c_int() for _ in range(5)]
    need = ctypes.c_int64()
    rc = lib.inc_woq_gemm_route(M, N, K, group_size, bits, dtype_code(dtype), int(bool(has_g_idx)), x_ptr or None, y_ptr or None,
                                bias_ptr or None, ws_ptr or None, ws_bytes, *[ctypes.byref(v) for v in o], ctypes.byref(need))
    if rc < 0:
        check(rc, "inc_woq_gemm_route")
    return dict(route=WOQ_GEMM_ROUTES[rc], splitk=o[0].value, row_blocks=o[1].value, steps=o[2].value, y_vec_ok=o[3].value,
                x_vec_ok=o[4].value, need=need.value)


def _none():
    return None


def _versions(tensors):
    return tuple(None if t is None else t._version for t in tensors)


def _unchanged(kept, versions, tensors):
    """`tensors` are the very objects of `kept` (None entries included), none written to since `versions` = _versions(kept)?"""
    if len(kept) != len(tensors):
        return False
    for a, v, b in zip(kept, versions, tensors):
        if a is not b or (a is not None and a._version != v):
            return False
    return True


class _PreparedCall:
    """What the prepared calls below share.  Each resolves once whatever does not change between the calls of one packed module (or
    group of modules): the device, the compute dtype and its code, the bias in the compute dtype, the addresses.  Each holds the
    tensors whose addresses it caches and remembers their version counters, so that current() can tell the owner whether it still
    describes the owner's buffers (same objects, not written to since); the owner rebuilds it otherwise.  Per call a subclass looks up
    the workspace (_ws_lookup) and launches (_launch); argument layout, entry point and row limits are the subclass's."""

    __slots__ = ("dev", "dev_index", "dtype", "dt", "bias_conv", "bi", "keep", "versions", "hold")
    lut = False  # (WoqGemmLutCall: True)
    anyw = False  # (WoqGemvAnywCall: True)
    ko = None  # (the act_order gather of WoqGemmCall / WoqGemvAnywCall; the batched calls: their members' orders)
    gather_max_mn = None  # (WoqGemvAnywCall with a gather: the limit it was built for)
    COMPUTES = (TypeError, "woq_gemm computes in bf16 or fp16")  # what a compute dtype other than bf16 / fp16 raises

    # a cache, not state: copies and pickles of the owning module start without it
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_none, ())

    def _compute_dt(self, dtype):
        if dtype is torch.bfloat16:
            return INC_BF16
        if dtype is torch.float16:
            return INC_F16
        exc, msg = self.COMPUTES
        raise exc(msg.format(dtype))

    def _bind(self, dev, dtype=None, dt=None, bias=None):
        """The device side of the constructor; the bias is converted once (the packed module stores fp16, a bf16 model multiplies in
        bf16)."""
        self.dev, self.dev_index = dev, dev.index if dev.index is not None else torch.cuda.current_device()
        self.dtype, self.dt = dtype, dt
        if bias is not None and bias.dtype != dtype:
            bias = bias.to(dtype)
        self.bias_conv, self.bi = bias, _ptr(bias)

    def _track(self, tensors):
        """The tensors (entries may be None) current() is asked about."""
        self.keep = tuple(tensors)
        self.versions = _versions(self.keep)

    def current(self, qweight, scales, qzeros, bias, owner_g_idx=None):
        """Still describes these tensors (same objects, not written to since)?  `owner_g_idx`: the owner's g_idx buffer as it is now --
        the call was built for the owner's plan at that time, which a new or rewritten g_idx invalidates.  (The form of the
        single-module calls; the batched ones have their own arguments.)"""
        # _unchanged over the five, written out: this runs in front of every decode forward, and the loop is host time there
        # (profiles/decode_host/)
        k, v = self.keep, self.versions
        return (k[0] is qweight and k[1] is scales and k[2] is qzeros and k[3] is bias and k[4] is owner_g_idx
                and qweight._version == v[0] and scales._version == v[1] and (qzeros is None or qzeros._version == v[2])
                and (bias is None or bias._version == v[3]) and (owner_g_idx is None or owner_g_idx._version == v[4])
                and (self.ko is None or (self.perm_keep[0]._version, self.perm_keep[1]._version) == self.perm_versions))


class WoqGemmCall(_PreparedCall):
    """inc_woq_gemm with everything that does not change between calls resolved once (the decode path: the kernel is ~6 us,
    so the host side counts).  Built by MI355XWeightOnlyLinear for its packed buffers; per call only the activation pointer,
    the output, the stream and the (device, stream) workspace are looked up.  Holds references to the tensors whose addresses
    it caches; the owner rebuilds it when a buffer is replaced.

    With `k_order` (int32 [K]; act_order modules) `qweight` is the K-sorted packed weight and the call computes x[:, k_order] W^T:
    up to 64 rows through inc_woq_gemm_perm wherever the shape takes a streaming decode route (the gather happens inside the
    kernel: one launch), otherwise x2d.index_select(1, k_order) and the ordinary launch.  `owner_qweight` is the buffer the sorted
    copy was made from: current() is asked about that one.  `owner_g_idx`: the owner's g_idx buffer when its plan was chosen."""

    __slots__ = ("N", "K", "G", "gs", "bits", "qw", "sc", "qz", "gi", "need", "ko", "perm_keep", "perm_versions", "perm_ok")
    PERM_ROUTES = (9, 10, 11)  # GEMV16, STREAM_W4, STREAM_W8: the routes inc_woq_gemm_perm launches

    def __init__(self, qweight, scales, qzeros, bias, N, K, group_size, bits, dtype, g_idx=None, k_order=None, owner_qweight=None,
                 owner_g_idx=None):
        dt = self._compute_dt(dtype)
        if k_order is not None:
            _check_k_order(k_order, K)
            if g_idx is not None:
                raise ValueError("k_order goes with the K-sorted weight, whose groups are contiguous: no g_idx")
        dev = _dev(qweight, scales, qzeros, bias, g_idx, k_order, owner_qweight)
        self.ko = _ptr(k_order)
        self.perm_keep = (qweight, k_order)
        self.perm_versions = _versions(self.perm_keep)
        self.perm_ok = {}  # M -> inc_woq_gemm_perm takes it
        self._track((qweight if owner_qweight is None else owner_qweight, scales, qzeros, bias, owner_g_idx))
        self.hold = g_idx
        self._bind(dev, dtype, dt, bias)
        self.N, self.K, self.G, self.gs, self.bits = N, K, scales.shape[0], group_size, bits
        self.qw, self.sc, self.qz, self.gi = qweight.data_ptr(), scales.data_ptr(), qzeros.data_ptr(), _ptr(g_idx)
        self.need = {}

    def _perm_takes(self, M):
        """inc_woq_gemm_perm launches for M rows: the dispatcher's own plan for the shape (host only; y comes from torch.empty and
        is 16-byte aligned, as the planner is told)."""
        rc = lib.inc_woq_gemm_route(M, self.N, self.K, self.gs, self.bits, self.dt, 0, None, None, self.bi, None, 0, None, None, None,
                                    None, None, None)
        return rc in self.PERM_ROUTES

    def __call__(self, x2d):
        """x2d: contiguous [M, K] of the call's dtype on the call's device (the owner checks)."""
        M = x2d.shape[0]
        # the pointers between dtype and bias: (qweight, scales, qzeros, g_idx), or (k_order, qweight, scales, qzeros) for inc_woq_gemm_perm
        fn, name, a2, a3, a4, a5 = lib.inc_woq_gemm, "inc_woq_gemm", self.qw, self.sc, self.qz, self.gi
        if self.ko is not None:
            ok = self.perm_ok.get(M)
            if ok is None:
                ok = self.perm_ok[M] = self._perm_takes(M)
            if ok:  # the gather happens in the kernel
                fn, name, a2, a3, a4, a5 = lib.inc_woq_gemm_perm, "inc_woq_gemm_perm", self.ko, self.qw, self.sc, self.qz
            else:
                x2d = x2d.index_select(1, self.perm_keep[1])
        y = torch.empty((M, self.N), dtype=self.dtype, device=self.dev)
        need = self.need.get(M)
        if need is None:
            need = self.need[M] = lib.inc_woq_gemm_workspace_bytes(M, self.N, self.K)
        # _ws_lookup and _launch, written out: of all prepared routes these two (4 / 8 bits, plain and act_order) are the ones whose host
        # enqueue time the two extra Python frames moved by more than its spread between processes (profiles/decode_host/)
        idx = self.dev_index
        stream = _raw_stream(idx)
        wp, wn = None, 0
        if need > 0:
            buf = _ws_cache.get((idx, stream))
            if buf is None or buf.numel() < need:
                buf = _workspace(self.dev, need)
            wp, wn = buf.data_ptr(), buf.numel()
        if _cur_device() == idx:
            rc = fn(x2d.data_ptr(), self.dt, a2, a3, a4, a5, self.bi, y.data_ptr(), M, self.N, self.K, self.G,
                    self.gs, self.bits, wp, wn, stream)
        else:
            with torch.cuda.device(self.dev):
                rc = fn(x2d.data_ptr(), self.dt, a2, a3, a4, a5, self.bi, y.data_ptr(), M, self.N, self.K,
                        self.G, self.gs, self.bits, wp, wn, stream)
        if rc != 0:
            check(rc, name)
        return y


def sort_packed_k(qweight, order, K, bits):
    """The optimum-layout packed weight with its K axis reordered: field k of the result (k < K) is field order[k] of `qweight`.

    qweight [ceil(K / n_pack), N] int32 with n_pack = 32 // bits fields of `bits` bits per word from bit 0 (any width 1..8, K % n_pack
    need not be 0: 4096 % 10 = 6 at 3 bits); order [K] integer.  The fields are unpacked, the first K kept, index_select(0, order)
    applied, the tail padded with zero fields to whole words and packed again.  Pure torch on qweight's device: what
    MI355XWeightOnlyLinear does once per packed state for an act_order module (order = the stable argsort of g_idx), so that the groups
    of the sorted words are contiguous and inc_woq_gemv_anyw_perm / inc_woq_gemm_perm only gather the activations."""
    if not 1 <= bits <= 8:
        raise ValueError(f"sort_packed_k: bits={bits}; fields of 1 .. 8 bits")
    npk, mask = 32 // bits, (1 << bits) - 1
    rows = -(-K // npk)
    if qweight.dim() != 2 or qweight.shape[0] != rows or qweight.dtype is not torch.int32:
        raise ValueError(f"sort_packed_k: qweight must be int32 [{rows}, N], got {qweight.dtype} {list(qweight.shape)}")
    if order.dim() != 1 or order.shape[0] != K:
        raise ValueError(f"sort_packed_k: order must hold K = {K} entries, got {list(order.shape)}")
    dev, N = qweight.device, qweight.shape[1]
    shifts = (torch.arange(npk, device=dev, dtype=torch.int64) * bits).view(1, npk, 1)
    fields = ((qweight.to(torch.int64).unsqueeze(1) >> shifts) & mask).reshape(rows * npk, N)[:K]
    fields = fields.index_select(0, order.to(device=dev, dtype=torch.int64))
    if rows * npk != K:
        fields = torch.cat([fields, fields.new_zeros((rows * npk - K, N))])
    words = (fields.reshape(rows, npk, N) << shifts).sum(dim=1)  # disjoint fields, < 2^32
    words = torch.where(words >= 2**31, words - 2**32, words)
    return words.to(torch.int32).contiguous()


GEMV_ANYW_BITS = (1, 2, 3, 5, 6, 7)
GEMV_ANYW_MAX_M = 16


def gemv_anyw_takes(N, K, group_size, bits):
    """inc_woq_gemv_anyw takes a module of this shape (for 1 .. 16 rows of bf16 / fp16 x)?  Pure arithmetic, no library call."""
    gs = K if (group_size == -1 or group_size >= K) else group_size
    return (bits in GEMV_ANYW_BITS and K > 0 and K % 32 == 0 and K <= 1 << 30 and N >= 64 and N % 4 == 0 and N <= 1 << 18
            and (gs == K or (gs >= 32 and gs & (gs - 1) == 0)))


def _gemv_anyw_check_module(qweight, scales, qzeros, bias, N, K, group_size, bits):
    """The module side of woq_gemv_anyw's argument checks: ValueError before anything touches the device."""
    if bits not in GEMV_ANYW_BITS:
        raise ValueError(f"woq_gemv_anyw: bits={bits}; it serves 1, 2, 3, 5, 6 and 7 bits (4 and 8 bits are woq_gemm's)")
    if K <= 0 or K % 32 != 0 or K > 1 << 30:
        raise ValueError(f"woq_gemv_anyw: K={K} must be a positive multiple of 32 (at most 2^30)")
    if N < 64 or N % 4 != 0 or N > 1 << 18:
        raise ValueError(f"woq_gemv_anyw: N={N} must be a multiple of 4, at least 64 (at most 2^18)")
    gs = K if (group_size == -1 or group_size >= K) else group_size
    if gs != K and (gs < 32 or gs & (gs - 1) != 0):
        raise ValueError(f"woq_gemv_anyw: group_size={group_size} must be a power of two >= 32, or one group per row (-1 / >= K)")
    n_pack, G = 32 // bits, -(-K // gs)
    want = {"qweight": ((-(-K // n_pack), N), torch.int32), "scales": ((G, N), torch.float16), "qzeros": ((G, -(-N // n_pack)), torch.int32)}
    for name, t in (("qweight", qweight), ("scales", scales), ("qzeros", qzeros)):
        shape, dt = want[name]
        if tuple(t.shape) != shape or t.dtype is not dt:
            raise ValueError(f"woq_gemv_anyw: {name} must be {dt} {list(shape)}, got {t.dtype} {list(t.shape)}")
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError(f"woq_gemv_anyw: bias must be [{N}], got {list(bias.shape)}")
    for name, t in (("qweight", qweight), ("scales", scales), ("qzeros", qzeros), ("bias", bias)):
        if t is None:
            continue
        if t.device.type != "cuda":
            raise ValueError(f"woq_gemv_anyw: {name} is on {t.device}; tensors must be resident in HBM (device 'cuda' = HIP)")
        if t.device != qweight.device:
            raise ValueError(f"woq_gemv_anyw: tensors on different devices: {qweight.device} vs {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"woq_gemv_anyw: {name} must be contiguous")
    return G


def _gemv_anyw_check_x_shape(x2d, K):
    if x2d.dtype is not torch.bfloat16 and x2d.dtype is not torch.float16:
        raise ValueError(f"woq_gemv_anyw computes in bf16 or fp16, got {x2d.dtype}")
    if x2d.dim() != 2 or x2d.shape[1] != K:
        raise ValueError(f"woq_gemv_anyw: x must be [M, {K}], got {list(x2d.shape)}")
    if not 1 <= x2d.shape[0] <= GEMV_ANYW_MAX_M:
        raise ValueError(f"woq_gemv_anyw: M={x2d.shape[0]}; it serves 1 .. {GEMV_ANYW_MAX_M} rows")


def _gemv_anyw_check_x(x2d, K, dtype, dev):
    _gemv_anyw_check_x_shape(x2d, K)
    if x2d.dtype is not dtype:
        raise ValueError(f"woq_gemv_anyw: x is {x2d.dtype}, the call computes in {dtype}")
    if x2d.device != dev:
        raise ValueError(f"woq_gemv_anyw: x is on {x2d.device}, the weights on {dev}")
    if not x2d.is_contiguous():
        raise ValueError("woq_gemv_anyw: x must be contiguous")


def woq_gemv_anyw(x2d, qweight, scales, qzeros, bias, N, K, group_size, bits):
    """y[M,N] = x[M,K] @ recover(x.dtype)^T + bias for 1 <= M <= 16 rows and an optimum-layout module of 1, 2, 3, 5, 6 or 7 bits, in
    one launch that streams the packed words once (inc_woq_gemv_anyw; == INCWeightOnlyLinear.forward, modules.py:594-610).

    qweight [ceil(K / n_pack), N] int32, scales [G, N] fp16, qzeros [G, ceil(N / n_pack)] int32 (n_pack = 32 // bits), contiguous
    groups of a power of two >= 32 (or one per row; a ragged last group is fine), K % 32 == 0, N % 4 == 0, N >= 64, x bf16 / fp16.
    Everything else raises ValueError before any launch."""
    if bits not in GEMV_ANYW_BITS:
        raise ValueError(f"woq_gemv_anyw: bits={bits}; it serves 1, 2, 3, 5, 6 and 7 bits (4 and 8 bits are woq_gemm's)")
    _gemv_anyw_check_x_shape(x2d, K)
    return WoqGemvAnywCall(qweight, scales, qzeros, bias, N, K, group_size, bits, x2d.dtype)(x2d, checked=False)


class WoqGemvAnywCall(_PreparedCall):
    """inc_woq_gemv_anyw with the module side resolved once (the decode path of the odd widths, like WoqGemmCall): data pointers, the
    bias converted to the compute dtype, the K-slices per M.  Per call only x, y, the stream and the workspace are looked up.
    `current()` has WoqGemmCall's contract (same tensors, version counters unchanged).

    The workspace is the (device, stream) one the other calls use (its counters are zero between launches), asked for 16 rows from the
    first call on so that a change of M does not move it; when it grows, the outgrown buffer is kept (_workspace), so a captured graph
    that replays the call never meets a freed workspace.

    With `k_order` (int32 [K]; act_order modules) `qweight` is the K-sorted packed weight (sort_packed_k) and the call computes
    x[:, k_order] W^T through inc_woq_gemv_anyw_perm: the gather happens inside the kernel, one launch, and x need not be 16-byte
    aligned.  `owner_qweight` is the buffer the sorted copy was made from: current() is asked about that one (WoqGemmCall's contract).
    `gather_max_mn`: with more than that many outputs (M * N) the call gathers with x.index_select(1, k_order) in front of the plain
    kernel instead (two launches, the same bits: every 64-column strip repeats the in-kernel gather, so its cost grows with rows x
    columns while the torch gather is paid once; None = always inside the kernel).  See gathers()."""

    __slots__ = ("N", "K", "G", "gs", "bits", "qw", "sc", "qz", "need", "ko", "perm_keep", "perm_versions", "gather_max_mn")
    anyw = True
    MAX_M = GEMV_ANYW_MAX_M
    COMPUTES = (ValueError, "woq_gemv_anyw computes in bf16 or fp16, got {}")

    def __init__(self, qweight, scales, qzeros, bias, N, K, group_size, bits, dtype, k_order=None, owner_qweight=None,
                 gather_max_mn=None, owner_g_idx=None):
        dt = self._compute_dt(dtype)
        self.gather_max_mn = gather_max_mn
        self.G = _gemv_anyw_check_module(qweight, scales, qzeros, bias, N, K, group_size, bits)
        if qweight.data_ptr() % 16:
            raise ValueError("woq_gemv_anyw: qweight must be 16-byte aligned")
        if k_order is not None:
            _check_k_order(k_order, K)
            if k_order.device != qweight.device or not k_order.is_contiguous() or k_order.data_ptr() % 16:
                raise ValueError("woq_gemv_anyw: k_order must be contiguous, 16-byte aligned and on the weights' device")
        self.ko = _ptr(k_order)
        self.perm_keep = (qweight, k_order)
        self.perm_versions = _versions(self.perm_keep)
        self._track((qweight if owner_qweight is None else owner_qweight, scales, qzeros, bias, owner_g_idx))
        self._bind(qweight.device, dtype, dt, bias)
        self.N, self.K, self.gs, self.bits = N, K, group_size, bits
        self.qw, self.sc, self.qz = qweight.data_ptr(), scales.data_ptr(), qzeros.data_ptr()
        self.need = None

    def slices(self, M):
        """K-slices of the launch for M rows (inc_woq_gemv_anyw_slices: host only)."""
        return lib.inc_woq_gemv_anyw_slices(M, self.N, self.K, self.bits)

    def gathers(self, M):
        """M rows go through inc_woq_gemv_anyw_perm (one launch)?  Otherwise x.index_select + inc_woq_gemv_anyw: the same bits."""
        return (self.ko is not None and (self.gather_max_mn is None or M * self.N <= self.gather_max_mn)
                and M * self.K < 1 << 31)  # (x by 32-bit byte offsets)

    def __call__(self, x2d, checked=True):
        """x2d: contiguous [M, K], 1 <= M <= 16, of the call's dtype on the call's device (`checked`: the owner has made sure)."""
        if not checked:
            _gemv_anyw_check_x(x2d, self.K, self.dtype, self.dev)
        M = x2d.shape[0]
        ko = self.ko
        if ko is not None and not self.gathers(M):
            x2d, ko = x2d.index_select(1, self.perm_keep[1]), None
        if ko is None and x2d.data_ptr() % 16:
            x2d = x2d.clone()  # the plain kernel reads x in 16-byte pieces; a fresh allocation is aligned
        y = torch.empty((M, self.N), dtype=self.dtype, device=self.dev)
        need = self.need
        if need is None:
            need = self.need = lib.inc_woq_gemv_anyw_workspace_bytes(self.MAX_M, self.N, self.K, self.bits)
        wp, wn, stream = _ws_lookup(self.dev, self.dev_index, need)
        tail = (self.qw, self.sc, self.qz, self.bi, y.data_ptr(), M, self.N, self.K, self.G, self.gs, self.bits, wp, wn, stream)
        if ko is None:
            _launch(self.dev, self.dev_index, lib.inc_woq_gemv_anyw, "inc_woq_gemv_anyw", (x2d.data_ptr(), self.dt) + tail)
        else:  # the gather happens in the kernel
            _launch(self.dev, self.dev_index, lib.inc_woq_gemv_anyw_perm, "inc_woq_gemv_anyw_perm", (x2d.data_ptr(), self.dt, ko) + tail)
        return y


def woq_gemm_lut(x2d, qweight, table16, scales, qzeros, bias, N, K, group_size, scale_round):
    """y[M,N] = x[M,K] @ recover(x.dtype)^T + bias for 4-bit row-packed modules (NF4 / FP4 code books, integer modules with
    use_optimum_format=False, compression_dim = 1), fused (include/inc_mi355x.h: inc_woq_gemm_lut; reference modules.py:594-610).

    qweight [N, words] of any integer container, scales [N,G] fp32 / fp16 / bf16, qzeros [N, words] or None; table16: 16 floats on
    the host, indexed by the stored 4-bit field (see the header); scale_round: round (table - zp) * scale to the scale dtype first
    (the integer formats' rule) or not (code books)."""
    return WoqGemmLutCall(qweight, table16, scales, qzeros, bias, N, K, group_size, scale_round, x2d.dtype)(x2d)


class WoqGemmLutCall(_PreparedCall):
    """inc_woq_gemm_lut with the module side resolved once (the decode path, like WoqGemmCall): the bias converted to the compute
    dtype, the table as a host array, the row sizes in bytes; per call only x, y, the stream and the (device, stream) workspace.
    `current()` has WoqGemmCall's contract (same tensors, version counters unchanged; these modules have no g_idx)."""

    lut = True
    COMPUTES = (TypeError, "woq_gemm_lut computes in bf16 or fp16")

    def __init__(self, qweight, table16, scales, qzeros, bias, N, K, group_size, scale_round, dtype):
        import ctypes

        dev = _dev(qweight, scales, qzeros, bias)
        dt = self._compute_dt(dtype)
        if len(table16) != 16:
            raise ValueError("table16 holds the 16 values of a 4-bit field")
        self._track((qweight, scales, qzeros, bias, None))
        self._bind(dev, dtype, dt, bias)
        self.N, self.K, self.G, self.gs = N, K, scales.shape[1], group_size
        self.table = (ctypes.c_float * 16)(*[float(v) for v in table16])
        self.sdt, self.rnd = dtype_code(scales.dtype), int(bool(scale_round))
        self.qw, self.row_bytes = qweight.data_ptr(), qweight.shape[1] * qweight.element_size()
        self.qz, self.zrow_bytes = (None, 0) if qzeros is None else (qzeros.data_ptr(), qzeros.shape[1] * qzeros.element_size())
        self.sc = scales.data_ptr()
        self.need = {}

    def __call__(self, x2d):
        """x2d: contiguous [M, K] of the call's dtype on the call's device."""
        M = x2d.shape[0]
        if x2d.data_ptr() % 16:
            x2d = x2d.clone()  # the kernel reads x in 16-byte pieces; a fresh allocation is aligned
        y = torch.empty((M, self.N), dtype=self.dtype, device=self.dev)
        need = self.need.get(M)
        if need is None:
            need = self.need[M] = lib.inc_woq_gemm_lut_workspace_bytes(M, self.N, self.K)
        wp, wn, stream = _ws_lookup(self.dev, self.dev_index, need)
        _launch(self.dev, self.dev_index, lib.inc_woq_gemm_lut, "inc_woq_gemm_lut", (
            x2d.data_ptr(), self.dt, self.qw, self.row_bytes, self.table, self.sc, self.sdt, self.rnd, self.qz, self.zrow_bytes,
            self.bi, y.data_ptr(), M, self.N, self.K, self.G, self.gs, wp, wn, stream))
        return y


def _check_k_orders(k_orders, n, K):
    """k_orders of a batched call: None, or one int32 [K] tensor or None per part (WoqGemmCall's messages for each)."""
    if k_orders is None:
        return None
    k_orders = list(k_orders)
    if len(k_orders) != n:
        raise ValueError(f"k_orders must have one entry per part ({n}), got {len(k_orders)}")
    for ko in k_orders:
        if ko is not None:
            _check_k_order(ko, K)
    return k_orders if any(ko is not None for ko in k_orders) else None


class _BatchedCall(_PreparedCall):
    """The batched calls: `parts` = [(qweight, scales, qzeros, bias or None, N), ...] multiply the SAME activation.  `k_orders`
    (act_order members): one int32 [K] tensor or None per part; with any entry given, part i's qweight is its K-sorted words and its
    activations are gathered through k_orders[i] inside the kernel; a part without an order gets the identity, built once per call
    object."""

    def _bind_parts(self, parts, K, dtype, dt, k_orders):
        """-> the order tensor of every part (the identity where it has none), or None when no part has one."""
        dev = _dev(*[t for p in parts for t in p[:4]], *(k_orders or ()))
        self._bind(dev, dtype, dt)
        self._track(t for p in parts for t in p[:4])
        self.orders = k_orders  # as given (None entries included): what current() compares
        self.order_versions = None if k_orders is None else _versions(k_orders)
        used = None
        if k_orders is not None:
            ident = torch.arange(K, dtype=torch.int32, device=dev) if any(ko is None for ko in k_orders) else None
            used = [ident if ko is None else ko for ko in k_orders]
        self.hold = (parts, used)
        return used

    def _parts_current(self, parts, k_orders):
        """Still describes these parts (same tensors, not written to since), the order tensors included?"""
        if not _unchanged(self.keep, self.versions, [t for p in parts for t in p[:4]]):
            return False
        if k_orders is not None and all(ko is None for ko in k_orders):
            k_orders = None
        if self.orders is None or k_orders is None:
            return self.orders is None and k_orders is None
        return _unchanged(self.orders, self.order_versions, k_orders)


class WoqGemmGroupCall(_BatchedCall):
    """inc_woq_gemm_multi for modules that multiply the SAME activation (q / k / v; gate / up): ONE launch instead of one per module
    (a decode call of one module is ~2 us of weight streaming behind ~5 us of launch boundary and hand-off).  The state dict is
    untouched: the call holds the modules' packed buffers by reference and hands the library host arrays of their addresses.
    `parts` = [(qweight, scales, qzeros, bias or None, N), ...]; K, group_size, bits common.  __call__(x2d) -> [y_i [M, N_i]], or None
    when the library declines the batch (nothing launched: the owner then calls the modules one by one).

    `k_orders` (act_order members): one int32 [K] tensor or None per part.  With any entry given the call goes to
    inc_woq_gemm_multi_perm: part i's qweight is then its K-sorted words and its activations are gathered through k_orders[i] inside
    the kernel (y_i = x[:, k_orders[i]] W_i^T + b_i, bit-identical to the plain call on x.index_select(1, k_orders[i])); a part
    without an order gets the identity, built once per call object."""

    def __init__(self, parts, K, group_size, bits, dtype, k_orders=None):
        import ctypes

        dt = self._compute_dt(dtype)
        n = self.n = len(parts)
        used = self._bind_parts(parts, K, dtype, dt, _check_k_orders(k_orders, n, K))
        self.K, self.gs, self.bits = K, group_size, bits
        bias = [None if p[3] is None else (p[3] if p[3].dtype == dtype else p[3].to(dtype)) for p in parts]
        self.bias_conv = bias
        self.Ns = [int(p[4]) for p in parts]
        self.qw = (ctypes.c_void_p * n)(*[p[0].data_ptr() for p in parts])
        self.sc = (ctypes.c_void_p * n)(*[p[1].data_ptr() for p in parts])
        self.qz = (ctypes.c_void_p * n)(*[p[2].data_ptr() for p in parts])
        self.bi = (ctypes.c_void_p * n)(*[_ptr(b) for b in bias]) if any(b is not None for b in bias) else None
        self.Narr = (ctypes.c_int64 * n)(*self.Ns)
        self.yarr = (ctypes.c_void_p * n)()
        self.need = {}
        self.ko = None if used is None else (ctypes.c_void_p * n)(*[ko.data_ptr() for ko in used])

    def current(self, parts, k_orders=None):
        return self._parts_current(parts, k_orders)

    def _outputs(self, M):
        ys = [torch.empty((M, N), dtype=self.dtype, device=self.dev) for N in self.Ns]
        for i, y in enumerate(ys):
            self.yarr[i] = y.data_ptr()
        return ys

    def __call__(self, x2d):
        M = x2d.shape[0]
        need = self.need.get(M)
        if need is None:
            need = self.need[M] = lib.inc_woq_gemm_multi_workspace_bytes(self.n, M, self.Narr, self.K)
        ys = self._outputs(M)
        wp, wn, stream = _ws_lookup(self.dev, self.dev_index, need)
        tail = (self.qw, self.sc, self.qz, self.bi, self.yarr, M, self.Narr, self.K, self.gs, self.bits, wp, wn, stream)
        if self.ko is None:
            rc = _launch(self.dev, self.dev_index, lib.inc_woq_gemm_multi, "inc_woq_gemm_multi", (self.n, x2d.data_ptr(), self.dt) + tail, True)
        else:
            rc = _launch(self.dev, self.dev_index, lib.inc_woq_gemm_multi_perm, "inc_woq_gemm_multi_perm",
                         (self.n, x2d.data_ptr(), self.dt, self.ko) + tail, True)
        return None if rc == -2 else ys  # (INC_ERR_UNSUPPORTED: nothing was launched)


class WoqGemvAnywGroupCall(WoqGemmGroupCall):
    """inc_woq_gemv_anyw_multi: WoqGemmGroupCall for the members of ONE odd width (1, 2, 3, 5, 6, 7 bits) on up to 16 rows -- q / k / v or
    gate / up in one launch over the strips of all members.  `parts`, `k_orders`, current() and the return value (a list of outputs, or
    None where the library declines: nothing launched) are WoqGemmGroupCall's; with orders, part i's qweight is its K-sorted words
    (sort_packed_k) and a part without an order gets the identity.  Output i equals WoqGemvAnywCall on part i bit for bit.  The workspace
    is asked for 16 rows from the first call on (0 bytes where K fits one slice)."""

    MAX_M = GEMV_ANYW_MAX_M
    COMPUTES = WoqGemvAnywCall.COMPUTES

    def __init__(self, parts, K, group_size, bits, dtype, k_orders=None):
        self._compute_dt(dtype)
        for p in parts:
            _gemv_anyw_check_module(p[0], p[1], p[2], p[3], int(p[4]), K, group_size, bits)
        super().__init__(parts, K, group_size, bits, dtype, k_orders=k_orders)
        self.need = None

    def __call__(self, x2d):
        """x2d: contiguous [M, K] of the call's dtype on the call's device; more than 16 rows -> None."""
        M = x2d.shape[0]
        if M > self.MAX_M:
            return None
        if self.ko is None and x2d.data_ptr() % 16:
            x2d = x2d.clone()  # the plain kernel reads x in 16-byte pieces; a fresh allocation is aligned
        need = self.need
        if need is None:
            need = self.need = lib.inc_woq_gemv_anyw_multi_workspace_bytes(self.n, self.MAX_M, self.Narr, self.K, self.bits)
        ys = self._outputs(M)
        wp, wn, stream = _ws_lookup(self.dev, self.dev_index, need)
        rc = _launch(self.dev, self.dev_index, lib.inc_woq_gemv_anyw_multi, "inc_woq_gemv_anyw_multi", (
            self.n, x2d.data_ptr(), self.dt, self.ko, self.qw, self.sc, self.qz, self.bi, self.yarr, M, self.Narr, self.K, self.gs,
            self.bits, wp, wn, stream), True)
        return None if rc == -2 else ys  # (INC_ERR_UNSUPPORTED: nothing was launched)


class WoqGatedCall(_BatchedCall):
    """inc_woq_gemm_gated with the module side resolved once: h = silu(x Wg^T) * (x Wu^T) for the gate / up pair of a dense gated MLP in
    ONE launch, the product formed in fp32 from the two fp32 sums and rounded once (transformers' LlamaMLP.forward up to down_proj).
    `gate_part` / `up_part` = (qweight, scales, qzeros, None, N) as for WoqGemmGroupCall: no bias, equal N; K, group_size common, 4 bits.
    `k_orders` = (gate's, up's) int32 [K] tensors or None (act_order members: the parts' words are then the K-sorted ones and each member
    gathers x through its own order; a member without an order gets the identity).  __call__(x2d) -> h [M, N], or None when the library
    declines (more than MAX_M rows, a shape the batched launch does not take: nothing launched)."""

    MAX_M = 16  # rows the entry serves (include/inc_mi355x.h)

    def __init__(self, gate_part, up_part, K, group_size, bits, dtype, k_orders=None):
        dt = self._compute_dt(dtype)
        parts = [gate_part, up_part]
        k_orders = _check_k_orders(k_orders, 2, K)
        if gate_part[3] is not None or up_part[3] is not None:
            raise ValueError("the gated pair takes modules without a bias")
        if int(gate_part[4]) != int(up_part[4]):
            raise ValueError(f"gate and up must have the same N, got {int(gate_part[4])} and {int(up_part[4])}")
        used = self._bind_parts(parts, K, dtype, dt, k_orders)
        self.N, self.K, self.gs, self.bits = int(gate_part[4]), K, group_size, bits
        self.ptrs = tuple(t.data_ptr() for p in parts for t in p[:3])
        self.ko = (None, None) if used is None else tuple(ko.data_ptr() for ko in used)
        self.need = {}

    def current(self, gate_part, up_part, k_orders=None):
        return self._parts_current((gate_part, up_part), k_orders)

    def __call__(self, x2d):
        """x2d: contiguous [M, K] of the call's dtype on the call's device (the owner checks)."""
        M = x2d.shape[0]
        need = self.need.get(M)
        if need is None:
            need = self.need[M] = lib.inc_woq_gemm_gated_workspace_bytes(M, self.N, self.K)
        h = torch.empty((M, self.N), dtype=self.dtype, device=self.dev)
        wp, wn, stream = _ws_lookup(self.dev, self.dev_index, need)
        rc = _launch(self.dev, self.dev_index, lib.inc_woq_gemm_gated, "inc_woq_gemm_gated", (
            x2d.data_ptr(), self.dt, self.ko[0], self.ko[1], *self.ptrs, h.data_ptr(), M, self.N, self.K, self.gs, self.bits, 0, wp, wn,
            stream), True)
        return None if rc == -2 else h  # (INC_ERR_UNSUPPORTED: nothing was launched)


# ---------------------------------------------------------------------------------------------------
# K4e fused MoE experts (INT4, optimum layout stacked on the expert axis)
# ---------------------------------------------------------------------------------------------------
def _index_bytes(top_k_index):
    if top_k_index.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"top_k_index must be int64 or int32, got {top_k_index.dtype}")
    return top_k_index.element_size()


def moe_route(top_k_index, num_experts, route=None):
    """inc_moe_route: top_k_index [T, k] -> the int32 route buffer (offsets, sorted slot order, inverse map, tile table; see the header)."""
    top_k_index = top_k_index.contiguous()
    dev = _dev(top_k_index)
    T, k = top_k_index.shape
    nbytes = lib.inc_moe_route_bytes(T, k, num_experts)
    if route is None:
        route = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_moe_route(_ptr(top_k_index), _index_bytes(top_k_index), T, k, num_experts, _ptr(route), route.numel() * 4, _stream()),
              "inc_moe_route")
    return route


def woq_moe_gemm(mode, a, route, qweight, scales, qzeros, T, top_k, group_size, routing_weights=None, out=None, workspace=None):
    """inc_woq_moe_gemm.  mode 0: gate_up + SiLU product -> [T*k, N/2] of a.dtype; mode 1: down x routing weight -> fp32 [T*k, N];
    mode 2: plain -> fp32 [T*k, N] (rows in the route's sorted order).  qweight [E, K/8, N], scales [E, G, N] fp16, qzeros [E, G, N/8]."""
    dev = _dev(a, route, qweight, scales, qzeros, routing_weights)
    if a.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("woq_moe_gemm computes in bf16 or fp16")
    E, K8, N = qweight.shape
    K, G, S = K8 * 8, scales.shape[1], T * top_k
    if out is None:
        out = (torch.empty((S, N // 2), dtype=a.dtype, device=dev) if mode == 0 else torch.empty((S, N), dtype=torch.float32, device=dev))
    need = lib.inc_woq_moe_gemm_workspace_bytes(mode, T, top_k, E, N, K)
    if need > 0 and (workspace is None or workspace.numel() < need):
        workspace = torch.zeros(need, dtype=torch.uint8, device=dev)  # counters must start at zero
    wdt = dtype_code(routing_weights.dtype) if routing_weights is not None else INC_F32
    with torch.cuda.device(dev):
        check(lib.inc_woq_moe_gemm(mode, _ptr(a), dtype_code(a.dtype), _ptr(route), _ptr(qweight), _ptr(scales), _ptr(qzeros),
                                   _ptr(routing_weights), wdt, _ptr(out), T, top_k, E, N, K, G, group_size,
                                   _ptr(workspace) if need > 0 else None, workspace.numel() if need > 0 else 0, _stream()),
              "inc_woq_moe_gemm")
    return out


def gptq_hessian_accum_routed(H, rows, a, route, T, top_k, sorted_rows=False):
    """inc_gptq_hessian_accum_routed: the GPTQ Hessians of all experts of one fused module from one forward, in stream order.
    H [E, K, K] fp32, rows [E] int64 (rows folded so far, advanced by the call), route = moe_route(top_k_index [T, top_k], E).
    sorted_rows=False: a = x [T, K], expert e folds the rows x[order[p] // top_k] of its range (gate_up); True: a [T * top_k, K] in the
    route's sorted order (down).  Returns False (nothing launched) when the library declines the shape: the caller then loops over
    gptq_hessian_accum on host-sliced ranges."""
    if H.dim() != 3 or H.shape[1] != H.shape[2] or H.dtype != torch.float32:
        raise ValueError(f"H must be fp32 [E, K, K], got {tuple(H.shape)} {H.dtype}")
    E, K = H.shape[0], H.shape[1]
    if rows.dtype != torch.int64 or rows.shape != (E,):
        raise ValueError(f"rows must be int64 [{E}], got {tuple(rows.shape)} {rows.dtype}")
    if route.dtype != torch.int32 or route.dim() != 1:
        raise TypeError("route must be the int32 buffer moe_route returns")
    T, top_k = int(T), int(top_k)
    if T <= 0 or top_k <= 0:
        raise ValueError("T and top_k must be positive")
    want = (T * top_k, K) if sorted_rows else (T, K)
    if a.dim() != 2 or tuple(a.shape) != want:
        raise ValueError(f"a must be {list(want)} for sorted_rows={bool(sorted_rows)}, got {tuple(a.shape)}")
    code = dtype_code(a.dtype)
    if route.numel() * 4 < lib.inc_moe_route_bytes(T, top_k, E):
        raise ValueError("route is smaller than inc_moe_route_bytes(T, top_k, E)")
    dev = _dev(H, rows, a, route)
    with torch.cuda.device(dev):
        rc = lib.inc_gptq_hessian_accum_routed(_ptr(a), code, 1 if sorted_rows else 0, _ptr(route), T, top_k, E, K, _ptr(H), _ptr(rows),
                                               _stream())
    if rc == -2:  # INC_ERR_UNSUPPORTED: nothing was launched
        return False
    check(rc, "inc_gptq_hessian_accum_routed")
    return True


def moe_combine(y, route, T, top_k, num_experts, dtype, out=None):
    """inc_moe_combine: out[t] = sum_s y[pos(t, s)] in fp32, rounded once to `dtype`."""
    dev = _dev(y, route)
    H = y.shape[1]
    if out is None:
        out = torch.empty((T, H), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_moe_combine(_ptr(y), _ptr(route), _ptr(out), dtype_code(dtype), T, top_k, num_experts, H, _stream()), "inc_moe_combine")
    return out


class WoqMoeCall(_PreparedCall):
    """One fused experts forward (route -> gate_up -> down -> combine, four launches, no host wait) with the module side resolved once.
    The route buffer and the two intermediates are allocated per call (the caching allocator makes that free of device allocations, and
    inside a graph capture they come from the graph's pool).  Only the split-K workspace is kept: one zero-initialised buffer per call
    object that serves every call shape (its counters sit in a fixed region) and only grows.  A grown-out buffer is retired, never freed,
    because a captured graph may still write to it; growth at least doubles the size, so the retired buffers add up to less than the
    current one, which is below 2 x the largest need: what is held stays below 4 x the largest need.
    Calls that share the workspace run in stream order (one module, one stream).  `current()` has WoqGemmCall's contract for the six
    packed buffers."""

    def __init__(self, gate_up, down, E, H, I, group_size):
        self._track(tuple(gate_up) + tuple(down))
        self._bind(_dev(*self.keep))
        self.gu, self.dn = [t.data_ptr() for t in gate_up], [t.data_ptr() for t in down]
        self.E, self.H, self.I, self.gs = E, H, I, group_size
        self.Gh, self.Gi = gate_up[1].shape[1], down[1].shape[1]
        self.workspace = None
        self.retired = []  # grown-out workspaces, kept alive for graphs that captured them

    def current(self, gate_up, down):
        return _unchanged(self.keep, self.versions, tuple(gate_up) + tuple(down))

    def held_bytes(self):
        """Device memory this call keeps between calls (the workspace and the retired ones)."""
        return sum(t.numel() for t in ([self.workspace] if self.workspace is not None else []) + self.retired)

    def _workspace(self, T, k):
        need = max(lib.inc_woq_moe_gemm_workspace_bytes(0, T, k, self.E, 2 * self.I, self.H),
                   lib.inc_woq_moe_gemm_workspace_bytes(1, T, k, self.E, self.H, self.I))
        ws = self.workspace
        if need > 0 and (ws is None or ws.numel() < need):
            if ws is not None:
                self.retired.append(ws)
            size = max(need, 2 * ws.numel() if ws is not None else 0)
            ws = self.workspace = torch.zeros(size, dtype=torch.uint8, device=self.dev)  # counters must start at zero
        return ws

    def __call__(self, x2d, top_k_index, top_k_weights):
        """x2d [T, H] bf16 / fp16, top_k_index [T, k] int64 / int32, top_k_weights [T, k] fp32 / bf16 / fp16, all contiguous on the call's
        device -> [T, H] of x2d's dtype."""
        T, k = top_k_index.shape
        dt = dtype_code(x2d.dtype)
        E, H, I = self.E, self.H, self.I
        ws = self._workspace(T, k)
        wp, wn = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())
        route = torch.empty(lib.inc_moe_route_bytes(T, k, E) // 4, dtype=torch.int32, device=self.dev)
        h = torch.empty((T * k, I), dtype=x2d.dtype, device=self.dev)
        y = torch.empty((T * k, H), dtype=torch.float32, device=self.dev)
        out = torch.empty((T, H), dtype=x2d.dtype, device=self.dev)
        stream = _raw_stream(self.dev_index)
        with torch.cuda.device(self.dev):
            rc = lib.inc_moe_route(top_k_index.data_ptr(), top_k_index.element_size(), T, k, E, route.data_ptr(), route.numel() * 4, stream)
            if rc == 0:
                rc = lib.inc_woq_moe_gemm(0, x2d.data_ptr(), dt, route.data_ptr(), self.gu[0], self.gu[1], self.gu[2], None, INC_F32,
                                          h.data_ptr(), T, k, E, 2 * I, H, self.Gh, self.gs, wp, wn, stream)
            if rc == 0:
                rc = lib.inc_woq_moe_gemm(1, h.data_ptr(), dt, route.data_ptr(), self.dn[0], self.dn[1], self.dn[2], top_k_weights.data_ptr(),
                                          dtype_code(top_k_weights.dtype), y.data_ptr(), T, k, E, H, I, self.Gi, self.gs, wp, wn, stream)
            if rc == 0:
                rc = lib.inc_moe_combine(y.data_ptr(), route.data_ptr(), out.data_ptr(), dt, T, k, E, H, stream)
        if rc != 0:
            check(rc, "fused MoE experts forward")
        return out


# ---------------------------------------------------------------------------------------------------
# K7 group-wise RTN
# ---------------------------------------------------------------------------------------------------
def groupwise_quant(w, bits, group_size, scheme, quantile=1.0, full_range=False, return_int=False, inplace=True):
    """== quant_tensor (utility.py:272-436) for dtype "int".

    return_int=False: fake-quantises `w` (in place when `inplace`) and returns it.
    return_int=True : returns (int_weight int32 [N,K], scale fp32 [N,G], zp fp32 [N,G] or None); `w` is untouched.
    """
    dev = _dev(w)
    N, K = w.shape
    gs = K if (group_size == -1 or K < group_size) else group_size
    G = (K + gs - 1) // gs
    sym = scheme == "sym"
    scale = torch.empty((N, G), dtype=torch.float32, device=dev)
    zp = None if sym else torch.empty((N, G), dtype=torch.float32, device=dev)
    if return_int:
        iw = torch.empty((N, K), dtype=torch.int32, device=dev)
        qdq = None
    else:
        iw = None
        qdq = w if inplace else torch.empty_like(w)
    with torch.cuda.device(dev):
        check(
            lib.inc_groupwise_quant(
                _ptr(w), dtype_code(w.dtype), _ptr(qdq), _ptr(iw), _ptr(scale), _ptr(zp), N, K, gs, bits,
                INC_SCHEME_SYM if sym else INC_SCHEME_ASYM, float(quantile), int(bool(full_range)), _stream(),
            ),
            "inc_groupwise_quant",
        )
    if return_int:
        return iw, scale, zp
    return qdq


def codebook_quant(w, values, codes, group_size, quantile=1.0, return_int=False, inplace=True, scale=None):
    """== quantize_4bit through quant_tensor (utility.py:112-149, 246-265): NF4 / FP4 code-book quantisation per row group.

    values / codes: the ascending code book and the integers stored for its entries (FLOAT_MAPPING / INT_MAPPING).
    return_int=False: fake-quantises `w` (in place when `inplace`) and returns it; return_int=True: (int32 codes [N,K],
    scale [N,G] fp32, None) -- there is no zero point in these formats.  `scale` [N,G] (or broadcastable to it): the caller's
    scales, used instead of the rows' own max (quantize_4bit(..., scale=...), utility.py:127-128)."""
    import ctypes

    dev = _dev(w)
    assert w.dim() == 2
    N, K = w.shape
    gs = K if (group_size == -1 or K < group_size) else int(group_size)
    G = -(-K // gs)
    n = len(values)
    vals = (ctypes.c_float * n)(*[float(v) for v in values])
    cds = (ctypes.c_int32 * n)(*[int(c) for c in codes])
    scale_in = None
    if scale is not None:
        # anything the reference's `tensor.div_(scale)` broadcasts against the grouped weight [N * G, group_size] (utility.py:127-128): a
        # per-tensor scalar (0-dim or one element), one value per row [N] / [N,1], or the full [N,G] table.  The kernel divides in fp32
        # (the reference divides in the promoted dtype of weight and scale; equal for fp32 scales, one rounding apart for 16-bit ones)
        sc32 = scale.to(device=dev, dtype=torch.float32)
        if sc32.numel() == 1:
            sc32 = sc32.reshape(1, 1)
        elif sc32.dim() < 2:
            sc32 = sc32.reshape(-1, 1)
        else:
            sc32 = sc32.reshape(sc32.shape[0], -1)
        scale_in = torch.broadcast_to(sc32, (N, G)).contiguous()
    scale = torch.empty((N, G), dtype=torch.float32, device=dev)
    if return_int:
        iout = torch.empty((N, K), dtype=torch.int32, device=dev)
        qdq = None
    else:
        iout = None
        qdq = w if inplace else torch.empty_like(w)
    with torch.cuda.device(dev):
        check(lib.inc_codebook_quant_with_scale(_ptr(w), dtype_code(w.dtype), _ptr(qdq), _ptr(iout), _ptr(scale), N, K, gs, vals, cds, n,
                                                float(quantile), _ptr(scale_in), _stream()), "inc_codebook_quant_with_scale")
    if return_int:
        return iout, scale, None
    return qdq


_MSE_WS = {}


def mse_accumulate(a, b, out=None):
    """out += sum((a-b)^2): fp64 scalar tensor on device, fixed summation order (same input -> same bits)."""
    dev = _dev(a, b)
    assert a.dtype == b.dtype and a.numel() == b.numel()
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=dev)
    assert out.dtype == torch.float64
    ws = _MSE_WS.get(dev)
    if ws is None:  # per-workgroup partials; calls on one device are stream-ordered, so one buffer per device
        ws = _MSE_WS[dev] = torch.empty(int(lib.inc_mse_accumulate_workspace_bytes()) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_mse_accumulate(_ptr(a), _ptr(b), dtype_code(a.dtype), a.numel(), _ptr(out), _ptr(ws), _stream()), "inc_mse_accumulate")
    return out


# ---------------------------------------------------------------------------------------------------
# K5/K6 GPTQ
# ---------------------------------------------------------------------------------------------------
def gptq_hessian_accum(H, x2d, beta, alpha):
    """H <- beta*H + alpha * x^T x on the upper-triangular tiles (== GPTQ.add_batch, gptq.py:1111-1141)."""
    dev = _dev(H)
    if x2d.device.type != "cuda":
        raise RuntimeError("calibration activations must be resident in HBM")
    assert x2d.dim() == 2 and x2d.stride(1) == 1, "x must be [T,K] with unit inner stride"
    T, K = x2d.shape
    assert H.shape == (K, K) and H.dtype == torch.float32
    with torch.cuda.device(dev):
        check(
            lib.inc_gptq_hessian_accum(
                x2d.data_ptr(), dtype_code(x2d.dtype), T, K, x2d.stride(0), _ptr(H), float(beta), float(alpha), _stream()
            ),
            "inc_gptq_hessian_accum",
        )
    return H


# False: every tile of the batched Hessian launch is one workgroup (the last round of a launch then runs on a fraction of the CUs);
# a module attribute for A/B runs, not an environment switch
HESSIAN_TAIL_SPLIT = True
_hessian_ws_cache = {}


def _hessian_workspace(dev):
    """Scratch of the batched Hessian launch's split tail: one per (device, stream), never shared by concurrent launches."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _hessian_ws_cache.get(key)
    if buf is None:
        buf = _hessian_ws_cache[key] = torch.empty(lib.inc_gptq_hessian_accum_multi_workspace_bytes(), dtype=torch.uint8, device=dev)
    return buf


def gptq_hessian_accum_multi(items):
    """One launch for several Hessians of the same forward: items = [(H [K,K] fp32, x2d [T,K] 16-bit, beta, alpha), ...],
    all x2d with the same dtype and token count.  Returns False (nothing launched) when the library declines the batch
    (fp32 inputs, K < 256, more than 8 problems): the caller then uses gptq_hessian_accum per item."""
    import ctypes

    n = len(items)
    x0 = items[0][1]
    if n > 8 or x0.dtype not in (torch.bfloat16, torch.float16):
        return False
    dev = _dev(*[t for H, x, _, _ in items for t in (H, x)])
    T = x0.shape[0]
    for H, x, _, _ in items:
        assert H.dtype == torch.float32 and x.dim() == 2 and H.shape == (x.shape[1], x.shape[1])
        if x.dtype != x0.dtype or x.shape[0] != T:
            return False
    xs = (ctypes.c_void_p * n)(*[x.data_ptr() for _, x, _, _ in items])
    Hs = (ctypes.c_void_p * n)(*[H.data_ptr() for H, _, _, _ in items])
    Ks = (ctypes.c_int64 * n)(*[x.shape[1] for _, x, _, _ in items])
    ld = (ctypes.c_int64 * n)(*[x.stride(0) for _, x, _, _ in items])
    be = (ctypes.c_float * n)(*[float(b) for _, _, b, _ in items])
    al = (ctypes.c_float * n)(*[float(a) for _, _, _, a in items])
    ws = _hessian_workspace(dev) if HESSIAN_TAIL_SPLIT else None
    with torch.cuda.device(dev):
        rc = lib.inc_gptq_hessian_accum_multi(n, xs, dtype_code(x0.dtype), T, Ks, ld, Hs, be, al, _ptr(ws), 0 if ws is None else ws.numel(),
                                              _stream())
    if rc == -2:  # INC_ERR_UNSUPPORTED: nothing was launched
        return False
    check(rc, "inc_gptq_hessian_accum_multi")
    return True


def gptq_hessian_finalize(H, percdamp):
    """mirror + dead-column fix + damping (gptq.py:1186-1189, 1221-1227). Returns the uint8 dead mask [K]."""
    dev = _dev(H)
    K = H.shape[0]
    dead = torch.empty(K, dtype=torch.uint8, device=dev)
    ws = torch.empty(4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_gptq_hessian_finalize(_ptr(H), K, float(percdamp), _ptr(dead), _ptr(ws), _stream()), "inc_gptq_hessian_finalize")
    return dead


def gptq_prepare_weight(w, dead=None):
    """W.float() with dead columns zeroed (gptq.py:1176, 1189)."""
    w = w.contiguous()
    dev = _dev(w, dead)
    N, K = w.shape
    out = torch.empty((N, K), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_gptq_prepare_weight(_ptr(w), dtype_code(w.dtype), _ptr(out), _ptr(dead), N, K, _stream()), "inc_gptq_prepare_weight")
    return out


def gptq_find_params(w32, col0, group_size, ngroups, bits, sym, scale, zero, g0, mse=False, grid=100, maxshrink=0.8, norm=2.4):
    """Quantizer.find_params(weight=True) for `ngroups` groups starting at column `col0` (gptq.py:1501-1624); `mse`
    adds the shrink-grid search of :1567-1584."""
    dev = _dev(w32, scale, zero)
    N, K = w32.shape
    G = scale.shape[1]
    with torch.cuda.device(dev):
        if mse:
            check(
                lib.inc_gptq_find_params_mse(_ptr(w32), N, K, col0, group_size, ngroups, bits, int(bool(sym)), int(grid),
                                             float(maxshrink), float(norm), _ptr(scale), _ptr(zero), G, g0, _stream()),
                "inc_gptq_find_params_mse",
            )
        else:
            check(
                lib.inc_gptq_find_params(_ptr(w32), N, K, col0, group_size, ngroups, bits, int(bool(sym)), _ptr(scale), _ptr(zero), G, g0, _stream()),
                "inc_gptq_find_params",
            )


def gptq_quant_block(w32, hinv, scale, zero, codes, q_out, err, i1, count, group_size, bits):
    dev = _dev(w32, hinv, scale, zero, codes, q_out, err)
    N, K = w32.shape
    G = scale.shape[1]
    with torch.cuda.device(dev):
        check(
            lib.inc_gptq_quant_block(
                _ptr(w32), _ptr(hinv), _ptr(scale), _ptr(zero), _ptr(codes), _ptr(q_out),
                dtype_code(q_out.dtype) if q_out is not None else INC_F32, _ptr(err), N, K, G, i1, count,
                group_size, bits, _stream(),
            ),
            "inc_gptq_quant_block",
        )


def gptq_quant_block_params(w32, hinv, scale, zero, codes, q_out, err, i1, count, group_size, bits, sym):
    """`gptq_quant_block` that first computes the block's own group parameters (find_params fused into the launch; see
    include/inc_mi355x.h).  Returns False when the library has no such form for this block."""
    dev = _dev(w32, hinv, scale, zero, codes, q_out, err)
    N, K = w32.shape
    G = scale.shape[1]
    with torch.cuda.device(dev):
        rc = lib.inc_gptq_quant_block_params(
            _ptr(w32), _ptr(hinv), _ptr(scale), _ptr(zero), _ptr(codes), _ptr(q_out),
            dtype_code(q_out.dtype) if q_out is not None else INC_F32, _ptr(err), N, K, G, i1, count, group_size, bits,
            1 if sym else 0, _stream())
    if rc == -2:  # INC_ERR_UNSUPPORTED
        return False
    check(rc, "inc_gptq_quant_block_params")
    return True


def gptq_lazy_update(w32, hinv, err, i1, count):
    dev = _dev(w32, hinv, err)
    N, K = w32.shape
    with torch.cuda.device(dev):
        check(lib.inc_gptq_lazy_update(_ptr(w32), _ptr(hinv), _ptr(err), N, K, i1, count, _stream()), "inc_gptq_lazy_update")


def gptq_lazy_update_cols(w32, hinv, err, i1, count, col_begin, col_end):
    """`gptq_lazy_update` for the trailing columns [col_begin, col_end) only (see include/inc_mi355x.h); launches on the
    CURRENT stream.  Returns False when the library has no column-range form for this block shape."""
    dev = _dev(w32, hinv, err)
    N, K = w32.shape
    with torch.cuda.device(dev):
        rc = lib.inc_gptq_lazy_update_cols(_ptr(w32), _ptr(hinv), _ptr(err), N, K, i1, count, col_begin, col_end, _stream())
    if rc == -2:  # INC_ERR_UNSUPPORTED
        return False
    check(rc, "inc_gptq_lazy_update_cols")
    return True


def probe_hbm_triad(a, b, c, s):
    """a <- b + s * c (fp32, same shape): the stream triad behind bench.py's `ceilings` (include/inc_mi355x.h)."""
    dev = _dev(a, b, c)
    with torch.cuda.device(dev):
        check(lib.inc_probe_hbm_triad(_ptr(a), _ptr(b), _ptr(c), float(s), a.numel(), _stream()), "inc_probe_hbm_triad")


def probe_hbm_copy(dst, src, variant=0):
    """dst <- src (same byte count, 16-byte aligned): the chip's copy ceiling for bench.py; `variant` see inc_probe_hbm_copy."""
    dev = _dev(dst, src)
    nbytes = src.numel() * src.element_size()
    assert nbytes == dst.numel() * dst.element_size() and nbytes % 16 == 0
    with torch.cuda.device(dev):
        check(lib.inc_probe_hbm_copy(_ptr(dst), _ptr(src), nbytes, int(variant), _stream()), "inc_probe_hbm_copy")
    return dst


def probe_mfma_bf16(src, sink, blocks, iters):
    """Bare bf16 MFMA loop (bench.py `ceilings`); returns the flops of the launch."""
    import ctypes

    dev = _dev(src, sink)
    assert src.numel() * src.element_size() >= 65536 and sink.numel() >= blocks * 256
    flops = ctypes.c_double(0.0)
    with torch.cuda.device(dev):
        check(lib.inc_probe_mfma_bf16(_ptr(src), _ptr(sink), int(blocks), int(iters), ctypes.byref(flops), _stream()), "inc_probe_mfma_bf16")
    return flops.value


# ---------------------------------------------------------------------------------------------------
# forward elementwise chains of a Llama block (csrc/fwd_elementwise.hip): bit-identical to eager, or declined
# ---------------------------------------------------------------------------------------------------
def _fwd_call(fn, name, args):
    """check(rc) -- except INC_ERR_UNSUPPORTED (-2: nothing was launched), which is False: the caller runs the eager ops."""
    rc = fn(*args)
    if rc == -2:
        return False
    check(rc, name)
    return True


def fwd_silu_mul(gate, up):
    """`silu(gate) * up` with eager's two roundings in one pass (inc_fwd_silu_mul); None where the library declines."""
    dev = _dev(gate, up)
    if gate.shape != up.shape or gate.dtype != up.dtype or gate.numel() == 0:
        return None
    out = torch.empty_like(gate)
    with torch.cuda.device(dev):
        ok = _fwd_call(lib.inc_fwd_silu_mul, "inc_fwd_silu_mul", (_ptr(gate), _ptr(up), _ptr(out), gate.numel(), dtype_code(gate.dtype), _stream()))
    return out if ok else None


def fwd_rmsnorm(x, weight, eps):
    """LlamaRMSNorm.forward on contiguous x [..., cols] in one pass (inc_fwd_rmsnorm); None where the library declines (shapes whose
    mean torch sums in an order the kernel does not reproduce)."""
    dev = _dev(x, weight)
    cols = x.shape[-1]
    if x.dtype != weight.dtype or weight.shape != (cols,) or x.numel() == 0:
        return None
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        ok = _fwd_call(lib.inc_fwd_rmsnorm, "inc_fwd_rmsnorm",
                       (_ptr(x), _ptr(weight), _ptr(out), x.numel() // cols, cols, float(eps), dtype_code(x.dtype), _stream()))
    return out if ok else None


def fwd_rope(q, k, cos, sin, q_out_strides, k_out_strides):
    """apply_rotary_pos_emb(q, k, cos, sin) for q [B, Hq, T, D], k [B, Hk, T, D] addressed by their strides (last stride 1) and contiguous
    cos / sin [1 or B, T, D], in one launch (inc_fwd_rope).  The outputs get the given strides (the ones eager's results have); None where
    the library declines."""
    import ctypes

    for t in (q, k, cos, sin):
        if t.device.type != "cuda" or t.device != q.device or t.dtype != q.dtype:
            return None
    if q.dim() != 4 or k.dim() != 4 or cos.dim() != 3 or cos.shape != sin.shape or not cos.is_contiguous() or not sin.is_contiguous():
        return None
    B, Hq, T, D = q.shape
    if k.shape[0] != B or k.shape[2] != T or k.shape[3] != D or cos.shape[1:] != (T, D) or cos.shape[0] not in (1, B):
        return None
    if q.numel() == 0 or k.numel() == 0 or q.stride(3) != 1 or k.stride(3) != 1 or q_out_strides[3] != 1 or k_out_strides[3] != 1:
        return None
    q_out = torch.empty_strided(q.shape, q_out_strides, dtype=q.dtype, device=q.device)
    k_out = torch.empty_strided(k.shape, k_out_strides, dtype=k.dtype, device=k.device)
    strides = (ctypes.c_int64 * 12)(*q.stride()[:3], *k.stride()[:3], *q_out_strides[:3], *k_out_strides[:3])
    with torch.cuda.device(q.device):
        ok = _fwd_call(lib.inc_fwd_rope, "inc_fwd_rope",
                       (_ptr(q), _ptr(k), _ptr(cos), _ptr(sin), _ptr(q_out), _ptr(k_out), B, Hq, k.shape[1], T, D, strides, cos.shape[0],
                        dtype_code(q.dtype), _stream()))
    return (q_out, k_out) if ok else None


def probe_round16(x, dtype):
    """fp32 `x` (contiguous) rounded to `dtype` (bf16 / fp16) by the rounding helper of the forward kernels (inc_probe_round16): what
    tests compare with torch's own `x.to(dtype)` bit for bit."""
    dev = _dev(x)
    assert x.dtype == torch.float32 and dtype in (torch.bfloat16, torch.float16)
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    with torch.cuda.device(dev):
        check(lib.inc_probe_round16(_ptr(x), _ptr(out), x.numel(), dtype_code(dtype), _stream()), "inc_probe_round16")
    return out


_HIP_RT = None


def cu_masked_stream(device, mask_words):
    """A HIP stream restricted to the compute units whose bits are set (hipExtStreamCreateWithCUMask), as a torch stream; None when
    the runtime refuses.  On the MI355X the 256 bits are 8 words of 32: word w = CU number w of every shader engine (measured with
    inc_probe_mfma_bf16, scripts/cumask_probe.py: seven words set = 224 CUs, one CU per shader engine left free)."""
    global _HIP_RT
    import ctypes

    try:
        if _HIP_RT is None:
            _HIP_RT = ctypes.CDLL("libamdhip64.so")
        st = ctypes.c_void_p()
        arr = (ctypes.c_uint32 * len(mask_words))(*mask_words)
        with torch.cuda.device(device):
            if _HIP_RT.hipExtStreamCreateWithCUMask(ctypes.byref(st), len(mask_words), arr) != 0 or not st.value:
                return None
            return torch.cuda.ExternalStream(st.value, device=device)
    except Exception:  # pragma: no cover - a runtime without the extension
        return None


def trace_marker(marker_id, device=None):
    """Phase boundary for kernel-trace timelines: an empty launch with Grid_Size_X = 64 * marker_id on the current stream."""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        check(lib.inc_trace_marker(int(marker_id), _stream()), "inc_trace_marker")


GPTQ_DYNAMIC_GROUPS, GPTQ_MSE, GPTQ_NO_LOOKAHEAD, GPTQ_NO_FUSED_PARAMS = 1, 2, 4, 8


def gptq_quantize_layer(w32, hinv, scale, zero, loop_scale, loop_zero, codes, q_out, err_ws, group_size, kernel_group_size, block_size,
                        bits, sym, flags, aux_stream=None):
    """The whole blocked column loop of GPTQ.fasterquant (gptq.py:1250-1304) as ONE C-ABI call (include/inc_mi355x.h:
    inc_gptq_quantize_layer): issued on the CURRENT stream, the bulk of the lazy updates on `aux_stream` (a torch stream) when
    given.  `err_ws` is fp32 [2, N, 128]; `loop_scale` / `loop_zero` may be None (= scale / zero)."""
    dev = _dev(w32, hinv, scale, zero, codes, q_out, err_ws)
    N, K = w32.shape
    assert err_ws.dtype == torch.float32 and err_ws.numel() >= 2 * N * 128
    with torch.cuda.device(dev):
        check(
            lib.inc_gptq_quantize_layer(
                _ptr(w32), _ptr(hinv), _ptr(scale), _ptr(zero), scale.shape[1], _ptr(loop_scale), _ptr(loop_zero),
                loop_scale.shape[1] if loop_scale is not None else scale.shape[1], _ptr(codes), _ptr(q_out),
                dtype_code(q_out.dtype) if q_out is not None else INC_F32, _ptr(err_ws), N, K, int(group_size), int(kernel_group_size),
                int(block_size), int(bits), 1 if sym else 0, int(flags), _stream(),
                aux_stream.cuda_stream if aux_stream is not None else None,
            ),
            "inc_gptq_quantize_layer",
        )


def chol_diag_block(A_view, Linv_view, info, tag):
    """In-place Cholesky of one <=128x128 diagonal block (a strided view into a larger fp32 matrix) + inverse of its
    factor into `Linv_view` (also a strided view).  See include/inc_mi355x.h: inc_chol_diag_block."""
    dev = A_view.device
    if dev.type != "cuda" or Linv_view.device != dev:
        raise RuntimeError("chol_diag_block needs HBM-resident views")
    n = A_view.shape[0]
    assert A_view.shape == (n, n) and Linv_view.shape == (n, n) and A_view.stride(1) == 1 and Linv_view.stride(1) == 1
    assert A_view.dtype == torch.float32 and Linv_view.dtype == torch.float32
    with torch.cuda.device(dev):
        check(
            lib.inc_chol_diag_block(A_view.data_ptr(), A_view.stride(0), n, Linv_view.data_ptr(), Linv_view.stride(0),
                                    _ptr(info), int(tag), _stream()),
            "inc_chol_diag_block",
        )


def gptq_inverse_factor(H, aux_stream=None, flags=0):
    """Upper Cholesky factor U of H^-1 for the damped SPD fp32 Hessian H [K,K] (gptq.py:1228-1231) as ONE C-ABI call
    (include/inc_mi355x.h: inc_gptq_inverse_factor).  Returns (U, info): `info` is a device int32 that stays 0 unless H
    is not positive definite (no host synchronisation here)."""
    dev = _dev(H)
    K = H.shape[0]
    assert H.shape == (K, K) and H.dtype == torch.float32 and H.is_contiguous()
    U = torch.empty((K, K), dtype=torch.float32, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = int(lib.inc_gptq_inverse_factor_workspace_bytes(K, int(flags)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    # (no record_stream for `aux_stream`: the call returns with the current stream ordered behind everything it issued on the second
    # one, so the caching allocator's stream-ordered reuse of H / U / the workspace is already safe -- and record_stream would make
    # every call hipMalloc a fresh workspace: 2.2 GB at K = 11008, 14.8 GB at K = 28672 with the split products' planes; the
    # caching allocator keeps one per stream that factorises, so the driver's concurrent factor streams each hold theirs)
    aux = aux_stream.cuda_stream if aux_stream is not None else None
    with torch.cuda.device(dev):
        check(lib.inc_gptq_inverse_factor(_ptr(H), K, _ptr(U), _ptr(ws), wsb, _ptr(info), int(flags), _stream(), aux), "inc_gptq_inverse_factor")
    return U, info


# ---------------------------------------------------------------------------------------------------
# K8 AWQ statistics
# ---------------------------------------------------------------------------------------------------
def awq_act_abs_sum(x2d, out):
    dev = _dev(x2d, out)
    T, K = x2d.shape
    with torch.cuda.device(dev):
        check(lib.inc_awq_act_abs_sum(_ptr(x2d), dtype_code(x2d.dtype), T, K, _ptr(out), _stream()), "inc_awq_act_abs_sum")
    return out


def awq_weight_scale(w, group_size):
    """== _get_weight_scale (awq.py:131-147): mean over rows of |w|/groupmax|w| -> [K] in w.dtype."""
    w = w.contiguous()
    dev = _dev(w)
    N, K = w.shape
    out = torch.zeros(K, dtype=torch.float32, device=dev)
    nbytes = lib.inc_awq_weight_scale_workspace_bytes(N, K, group_size)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(
            lib.inc_awq_weight_scale(_ptr(w), dtype_code(w.dtype), N, K, group_size, _ptr(out), _ptr(ws), nbytes, _stream()),
            "inc_awq_weight_scale",
        )
    return (out / N).to(w.dtype)


# ---------------------------------------------------------------------------------------------------
# K10-K14 SmoothQuant W8A8 (reference neural_compressor/torch/algorithms/smooth_quant/utility.py)
# ---------------------------------------------------------------------------------------------------
FLT_MAX = 3.4028234663852886e38


def sq_new_minmax(K, device):
    """(min, max) running buffers for sq_channel_minmax."""
    return (torch.full((K,), FLT_MAX, dtype=torch.float32, device=device),
            torch.full((K,), -FLT_MAX, dtype=torch.float32, device=device))


def sq_channel_minmax(x2d, mn, mx):
    """== Calibration._save_input_pc_hook (utility.py:858-883): running per-channel min / max of x [T, K]."""
    dev = _dev(x2d, mn, mx)
    if x2d.stride(-1) != 1:
        x2d = x2d.contiguous()
    T, K = x2d.shape
    with torch.cuda.device(dev):
        check(lib.inc_sq_channel_minmax(_ptr(x2d), dtype_code(x2d.dtype), T, K, x2d.stride(0), _ptr(mn), _ptr(mx), _stream()),
              "inc_sq_channel_minmax")
    return mn, mx


def sq_weight_col_absmax(w, out=None):
    """max_n |w[n,k]| accumulated into `out` (fp32 [K], zero-initialised): the weight side of cal_scale (:617-618)."""
    w = w.contiguous()
    dev = _dev(w, out)
    N, K = w.shape
    if out is None:
        out = torch.zeros(K, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_sq_weight_col_absmax(_ptr(w), dtype_code(w.dtype), N, K, _ptr(out), _stream()), "inc_sq_weight_col_absmax")
    return out


def sq_cal_scale(amax_x, amax_w, alpha, weight_max_lb=1e-5):
    """== cal_scale (utility.py:605-626) from the two abs-max vectors."""
    amax_x = amax_x.to(torch.float32).contiguous()
    amax_w = amax_w.to(torch.float32).contiguous()
    dev = _dev(amax_x, amax_w)
    K = amax_x.numel()
    scale = torch.empty(K, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_sq_cal_scale(_ptr(amax_x), _ptr(amax_w), K, float(alpha), float(weight_max_lb), _ptr(scale), _stream()),
              "inc_sq_cal_scale")
    return scale


def sq_quant_weight(w, smooth=None, Kp=None):
    """== quant_dequant_w_v1 (utility.py:652-695, Linear, sym int8) of w * smooth -> (qw int8 [N,Kp], scale [N], rowsum [N])."""
    w = w.contiguous()
    smooth = None if smooth is None else smooth.to(torch.float32).contiguous()
    dev = _dev(w, smooth)
    N, K = w.shape
    Kp = K if Kp is None else int(Kp)
    qw = torch.empty((N, Kp), dtype=torch.int8, device=dev)
    w_scale = torch.empty(N, dtype=torch.float32, device=dev)
    rowsum = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_sq_quant_weight(_ptr(w), dtype_code(w.dtype), N, K, Kp, _ptr(smooth), _ptr(qw), _ptr(w_scale), _ptr(rowsum),
                                      _stream()), "inc_sq_quant_weight")
    return qw, w_scale, rowsum


def sq_quant_act(x2d, in_scale, sx, zp, Kp=None):
    """clamp(rint(x * in_scale / sx + zp), 0, 255) - 128 as int8 [M, Kp] (SQLinearWrapper.forward + quant_dequant_x_v1)."""
    x2d = x2d.contiguous()
    dev = _dev(x2d, in_scale)
    M, K = x2d.shape
    Kp = K if Kp is None else int(Kp)
    out = torch.empty((M, Kp), dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_sq_quant_act(_ptr(x2d), dtype_code(x2d.dtype), M, K, Kp, _ptr(in_scale), float(sx), float(zp), _ptr(out),
                                   _stream()), "inc_sq_quant_act")
    return out


def sq_quant_act_token(x2d, in_scale, Kp=None):
    """Dynamic per-token symmetric int8: s[m] = max(max_k |x * in_scale| / 127, eps), q = clamp(rint(x * in_scale / s),
    -127, 127) -> (xq int8 [M, Kp], row_scale fp32 [M])."""
    x2d = x2d.contiguous()
    in_scale = None if in_scale is None else in_scale.to(torch.float32).contiguous()
    dev = _dev(x2d, in_scale)
    M, K = x2d.shape
    Kp = K if Kp is None else int(Kp)
    xq = torch.empty((M, Kp), dtype=torch.int8, device=dev)
    row_scale = torch.empty(M, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_sq_quant_act_token(_ptr(x2d), dtype_code(x2d.dtype), M, K, Kp, _ptr(in_scale), _ptr(xq), _ptr(row_scale), _stream()),
              "inc_sq_quant_act_token")
    return xq, row_scale


def w8a8_gemm(xq, wq, alpha, corr, bias, out_dtype, row_scale=None):
    """y = alpha[n] * (xq @ wq^T + corr[n]) + bias[n], int32 accumulate on the matrix cores (K14).  With `row_scale` (fp32 [M], the
    per-token cell): y = (row_scale[m] * alpha[n]) * (xq @ wq^T) + bias[n], alpha = w_scale and no corr."""
    dev = _dev(xq, wq, alpha, corr, bias, row_scale)
    M, K = xq.shape
    N = wq.shape[0]
    assert wq.shape[1] == K and xq.dtype == torch.int8 and wq.dtype == torch.int8
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    y = torch.empty((M, N), dtype=out_dtype, device=dev)
    nbytes = lib.inc_w8a8_gemm_workspace_bytes(M, N, K)
    ws = _workspace_i8(dev, nbytes) if nbytes > 0 else None
    if row_scale is not None:
        assert corr is None and row_scale.dtype == torch.float32 and row_scale.numel() == M and row_scale.is_contiguous()
        with torch.cuda.device(dev):
            check(lib.inc_w8a8_gemm_rowscale(_ptr(xq), _ptr(wq), _ptr(row_scale), _ptr(alpha), _ptr(bias), _ptr(y), dtype_code(out_dtype),
                                             M, N, K, _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "inc_w8a8_gemm_rowscale")
        return y
    with torch.cuda.device(dev):
        check(lib.inc_w8a8_gemm(_ptr(xq), _ptr(wq), _ptr(alpha), _ptr(corr), _ptr(bias), _ptr(y), dtype_code(out_dtype), M, N, K,
                                _ptr(ws), 0 if ws is None else ws.numel(), _stream()), "inc_w8a8_gemm")
    return y


_ws_i8_cache = {}


def _workspace_i8(dev, nbytes):
    """The int32 slabs of the W8A8 GEMM's K-split tail tiles, one buffer per (device, stream).  The kernels keep no state in it
    (every slab element that is read was written by the same call), so its contents never matter; separate from the 4-bit
    GEMM's workspace, whose first 16 KiB hold arrival counters that must stay zero between calls."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _ws_i8_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.zeros(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _ws_i8_cache[key] = buf
    return buf


# ---------------------------------------------------------------------------------------------------
# K15/K16 OCP microscaling: MXFP8 / MXFP4 on the block-scaled matrix instruction (include/inc_mi355x.h has the specification)
# ---------------------------------------------------------------------------------------------------
MX_FP8_E4M3, MX_FP4_E2M1 = 0, 4  # the instruction's own format codes
MX_KTILE = 128


def mx_padded_k(K):
    """K rounded up to the MX GEMM's K-tile."""
    return (int(K) + MX_KTILE - 1) // MX_KTILE * MX_KTILE


def mx_quant(x2d, fmt, Kp=None):
    """The MX row quantiser: x [M,K] bf16 / fp16 / fp32 -> (codes uint8 [M,Kp] (fp8) or [M,Kp/2] (fp4), scales uint8 [M,Kp/32])."""
    x2d = x2d.contiguous()
    dev = _dev(x2d)
    M, K = x2d.shape
    Kp = mx_padded_k(K) if Kp is None else int(Kp)
    codes = torch.empty((M, Kp if fmt == MX_FP8_E4M3 else Kp // 2), dtype=torch.uint8, device=dev)
    scales = torch.empty((M, Kp // 32), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_mx_quant(_ptr(x2d), dtype_code(x2d.dtype), M, K, Kp, int(fmt), _ptr(codes), _ptr(scales), _stream()), "inc_mx_quant")
    return codes, scales


def _mx_check_operands(xq, xs, xfmt, wq, ws, wfmt):
    """The shapes the MX products take -> Kp."""
    Kp = xs.shape[1] * 32
    assert ws.shape[1] * 32 == Kp and xq.dtype == torch.uint8 and wq.dtype == torch.uint8
    assert xq.shape[1] == (Kp if xfmt == MX_FP8_E4M3 else Kp // 2) and wq.shape[1] == (Kp if wfmt == MX_FP8_E4M3 else Kp // 2)
    assert xq.is_contiguous() and xs.is_contiguous() and wq.is_contiguous() and ws.is_contiguous()
    return Kp


def mx_gemm(xq, xs, xfmt, wq, ws, wfmt, bias, out_dtype):
    """y[m,n] = sum_blocks 2^(xs + ws - 254) * sum_{k in block} x_k * w_k + bias[n] on v_mfma_scale_f32_32x32x64_f8f6f4 (K16)."""
    dev = _dev(xq, xs, wq, ws, bias)
    M, N = xq.shape[0], wq.shape[0]
    Kp = _mx_check_operands(xq, xs, xfmt, wq, ws, wfmt)
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    y = torch.empty((M, N), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_mx_gemm(_ptr(xq), _ptr(xs), int(xfmt), _ptr(wq), _ptr(ws), int(wfmt), _ptr(bias), _ptr(y), dtype_code(out_dtype),
                              M, N, Kp, _stream()), "inc_mx_gemm")
    return y


MX_GEMV_MAX_M = 16      # INC_MX_GEMV_MAX_M: rows of x the decode route takes
MX_GEMV_MAX_MEMBERS = 8


def mx_gemv(xq, xs, xfmt, wq, ws, wfmt, bias, out_dtype):
    """mx_gemm's product for up to MX_GEMV_MAX_M rows of x on v_mfma_scale_f32_16x16x128_f8f6f4 (K16b, inc_mx_gemv): one workgroup per
    16 weight rows, K split over its waves, no workspace."""
    dev = _dev(xq, xs, wq, ws, bias)
    M, N = xq.shape[0], wq.shape[0]
    Kp = _mx_check_operands(xq, xs, xfmt, wq, ws, wfmt)
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    y = torch.empty((M, N), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_mx_gemv(_ptr(xq), _ptr(xs), int(xfmt), _ptr(wq), _ptr(ws), int(wfmt), _ptr(bias), _ptr(y), dtype_code(out_dtype),
                              M, N, Kp, _stream()), "inc_mx_gemv")
    return y


def mx_gemv_multi(xq, xs, xfmt, wqs, wss, wfmt, biases, out_dtype):
    """[mx_gemv(xq, xs, xfmt, wq_i, ws_i, wfmt, bias_i, out_dtype) for i] for 2 .. MX_GEMV_MAX_MEMBERS weight matrices in ONE launch
    (inc_mx_gemv_multi); every output is the single call's bit for bit.  `biases`: a list with None for a member without one."""
    import ctypes

    n = len(wqs)
    biases = [None if b is None else (b if b.dtype == out_dtype else b.to(out_dtype)) for b in biases]
    dev = _dev(xq, xs, *wqs, *wss, *biases)
    M = xq.shape[0]
    Kp = xs.shape[1] * 32
    for wq, ws in zip(wqs, wss):
        assert _mx_check_operands(xq, xs, xfmt, wq, ws, wfmt) == Kp
    ys = [torch.empty((M, wq.shape[0]), dtype=out_dtype, device=dev) for wq in wqs]
    arr = lambda ts: (ctypes.c_void_p * n)(*[_ptr(t) for t in ts])  # noqa: E731
    Ns = (ctypes.c_int64 * n)(*[wq.shape[0] for wq in wqs])
    with torch.cuda.device(dev):
        check(lib.inc_mx_gemv_multi(n, _ptr(xq), _ptr(xs), int(xfmt), arr(wqs), arr(wss), int(wfmt), arr(biases), arr(ys),
                                    dtype_code(out_dtype), M, Ns, Kp, _stream()), "inc_mx_gemv_multi")
    return ys


def _moe_gemm_out(mode, out, out_dtype, S, N, dev, routing_weights, name):
    """(out, its dtype, the routing weights' dtype code) of a routed GEMM wrapper `name` (mx_moe_gemm, mx_moe_gemm_glu, fp8_moe_gemm):
    mode 0 writes [S, N/2] of out's dtype or `out_dtype` (bf16 / fp16), modes 1 and 2 fp32 [S, N]; `out` is allocated when None."""
    if mode == 0:
        odt = out.dtype if out is not None else out_dtype
        if odt not in (torch.bfloat16, torch.float16):
            raise TypeError(f"{name} mode 0 writes bf16 or fp16: pass out_dtype")
    else:
        odt = torch.float32
    if out is None:
        out = torch.empty((S, N // 2 if mode == 0 else N), dtype=odt, device=dev)
    wdt = dtype_code(routing_weights.dtype) if routing_weights is not None else INC_F32
    return out, odt, wdt


def _mx_moe_check_operands(mode, aq, as_, afmt, wq, ws, wfmt, T, top_k):
    """The operand checks of mx_moe_gemm and mx_moe_gemm_glu -> (E, N, Kp, S)."""
    E, N = wq.shape[0], wq.shape[1]
    Kp, S = ws.shape[2] * 32, T * top_k
    assert aq.dtype == torch.uint8 and as_.dtype == torch.uint8 and wq.dtype == torch.uint8 and ws.dtype == torch.uint8
    assert aq.shape[0] == (S if mode == 1 else T) and as_.shape == (aq.shape[0], Kp // 32) and ws.shape[:2] == (E, N)
    assert aq.shape[1] == (Kp if afmt == MX_FP8_E4M3 else Kp // 2) and wq.shape[2] == (Kp if wfmt == MX_FP8_E4M3 else Kp // 2)
    assert aq.is_contiguous() and as_.is_contiguous() and wq.is_contiguous() and ws.is_contiguous()
    return E, N, Kp, S


def mx_moe_gemm(mode, aq, as_, afmt, route, wq, ws, wfmt, T, top_k, routing_weights=None, out=None, out_dtype=None):
    """inc_mx_moe_gemm (K16e): mx_gemm's product per expert over the rows of the route's sorted order.  wq [E, N, Kp or Kp/2],
    ws [E, N, Kp/32] (slice e = mx_quant of expert e's matrix).  mode 0: gate_up + SiLU product -> [T*k, N/2] of `out_dtype` (bf16 /
    fp16) from aq [T, ...]; mode 1: down x routing weight -> fp32 [T*k, N] from aq [T*k, ...] in sorted order; mode 2: plain -> fp32
    [T*k, N] from aq [T, ...].  Rows past the route's valid positions are not written."""
    dev = _dev(aq, as_, route, wq, ws, routing_weights)
    E, N, Kp, S = _mx_moe_check_operands(mode, aq, as_, afmt, wq, ws, wfmt, T, top_k)
    out, odt, wdt = _moe_gemm_out(mode, out, out_dtype, S, N, dev, routing_weights, "mx_moe_gemm")
    with torch.cuda.device(dev):
        check(lib.inc_mx_moe_gemm(mode, _ptr(aq), _ptr(as_), int(afmt), _ptr(route), _ptr(wq), _ptr(ws), int(wfmt), _ptr(routing_weights),
                                  wdt, _ptr(out), dtype_code(odt), T, top_k, E, N, Kp, _stream()), "inc_mx_moe_gemm")
    return out


def mx_moe_gemm_glu(mode, aq, as_, afmt, route, wq, ws, wfmt, T, top_k, bias=None, alpha=1.702, limit=7.0, routing_weights=None, out=None,
                    out_dtype=None):
    """inc_mx_moe_gemm_glu: mx_moe_gemm with a per-expert fp32 bias [E, N] (None: no add) in every mode and, in mode 0, the clamped
    SwiGLU of the GPT-OSS experts instead of the SiLU product: g = min(g, limit), u = clamp(u, -limit, limit), (u + 1) * g *
    sigmoid(alpha * g), on gate rows 0..I-1 and up rows I..2I-1 of wq / ws / bias.  Shapes, dtypes and modes as mx_moe_gemm."""
    dev = _dev(aq, as_, route, wq, ws, routing_weights, bias)
    E, N, Kp, S = _mx_moe_check_operands(mode, aq, as_, afmt, wq, ws, wfmt, T, top_k)
    assert bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (E, N) and bias.is_contiguous())
    out, odt, wdt = _moe_gemm_out(mode, out, out_dtype, S, N, dev, routing_weights, "mx_moe_gemm_glu")
    with torch.cuda.device(dev):
        check(lib.inc_mx_moe_gemm_glu(mode, _ptr(aq), _ptr(as_), int(afmt), _ptr(route), _ptr(wq), _ptr(ws), int(wfmt), _ptr(bias),
                                      float(alpha), float(limit), _ptr(routing_weights), wdt, _ptr(out), dtype_code(odt), T, top_k, E, N,
                                      Kp, _stream()), "inc_mx_moe_gemm_glu")
    return out


# ---------------------------------------------------------------------------------------------------
# K17 FP8 per-token / per-channel: e4m3 codes with one fp32 scale per row (include/inc_mi355x.h has the specification)
# ---------------------------------------------------------------------------------------------------
FP8_GEMV_MAX_M = MX_GEMV_MAX_M


def fp8_quant_rows(x2d, in_scale=None, Kp=None):
    """The per-row e4m3 quantiser (inc_fp8_quant_rows): x [M,K] bf16 / fp16 / fp32 -> (codes uint8 [M,Kp], row_scale fp32 [M]) with
    row_scale = max(max_k |x * in_scale| / 448, 2^-60) and codes = e4m3(x * in_scale / row_scale).  Activation rows and weight rows alike."""
    x2d = x2d.contiguous()
    in_scale = None if in_scale is None else in_scale.to(torch.float32).contiguous()
    dev = _dev(x2d, in_scale)
    M, K = x2d.shape
    Kp = mx_padded_k(K) if Kp is None else int(Kp)
    codes = torch.empty((M, Kp), dtype=torch.uint8, device=dev)
    row_scale = torch.empty(M, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_fp8_quant_rows(_ptr(x2d), dtype_code(x2d.dtype), M, K, Kp, _ptr(in_scale), _ptr(codes), _ptr(row_scale), _stream()),
              "inc_fp8_quant_rows")
    return codes, row_scale


def _fp8_product(fn, name, xq, row_scale, wq, alpha, bias, out_dtype):
    dev = _dev(xq, row_scale, wq, alpha, bias)
    (M, Kp), N = xq.shape, wq.shape[0]
    assert wq.shape[1] == Kp and xq.dtype == torch.uint8 and wq.dtype == torch.uint8
    assert row_scale.dtype == torch.float32 and row_scale.numel() == M and alpha.dtype == torch.float32 and alpha.numel() == N
    if bias is not None and bias.dtype != out_dtype:
        bias = bias.to(out_dtype)
    y = torch.empty((M, N), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(fn(_ptr(xq), _ptr(row_scale), _ptr(wq), _ptr(alpha), _ptr(bias), _ptr(y), dtype_code(out_dtype), M, N, Kp, _stream()), name)
    return y


def fp8_gemm(xq, row_scale, wq, alpha, bias, out_dtype):
    """y[m,n] = (row_scale[m] * alpha[n]) * sum_k x_k * w_k + bias[n] over e4m3 codes on v_mfma_f32_32x32x64_f8f6f4 (inc_fp8_gemm)."""
    return _fp8_product(lib.inc_fp8_gemm, "inc_fp8_gemm", xq, row_scale, wq, alpha, bias, out_dtype)


def fp8_gemv(xq, row_scale, wq, alpha, bias, out_dtype):
    """fp8_gemm's product for up to FP8_GEMV_MAX_M rows of x on v_mfma_f32_16x16x128_f8f6f4 (inc_fp8_gemv): one workgroup per 16 weight
    rows, K split over its waves, no workspace."""
    return _fp8_product(lib.inc_fp8_gemv, "inc_fp8_gemv", xq, row_scale, wq, alpha, bias, out_dtype)


FP8_GEMV_MAX_MEMBERS = 8


def _fp8_check_member(xq, wq, alpha):
    assert wq.dtype == torch.uint8 and wq.shape[1] == xq.shape[1] and wq.is_contiguous()
    assert alpha.dtype == torch.float32 and alpha.numel() == wq.shape[0] and alpha.is_contiguous()


def fp8_gemv_multi(xq, row_scale, wqs, alphas, biases, out_dtype, outs=None):
    """[fp8_gemv(xq, row_scale, wq_i, alpha_i, bias_i, out_dtype) for i] for 2 .. FP8_GEMV_MAX_MEMBERS weight matrices in ONE launch
    (inc_fp8_gemv_multi); every output is the single call's bit for bit.  `biases`: a list with None for a member without one.
    `outs`: contiguous [M, N_i] tensors of out_dtype to write into (allocated when None)."""
    import ctypes

    n = len(wqs)
    biases = [None if b is None else (b if b.dtype == out_dtype else b.to(out_dtype)) for b in biases]
    dev = _dev(xq, row_scale, *wqs, *alphas, *biases)
    M = xq.shape[0]
    Kp = xq.shape[1]
    assert xq.dtype == torch.uint8 and xq.is_contiguous() and row_scale.dtype == torch.float32 and row_scale.numel() == M
    for wq, alpha in zip(wqs, alphas):
        _fp8_check_member(xq, wq, alpha)
    if outs is None:
        ys = [torch.empty((M, wq.shape[0]), dtype=out_dtype, device=dev) for wq in wqs]
    else:
        ys = list(outs)
        assert len(ys) == n and all(y.shape == (M, wq.shape[0]) and y.dtype == out_dtype and y.is_contiguous() for y, wq in zip(ys, wqs))
    arr = lambda ts: (ctypes.c_void_p * n)(*[_ptr(t) for t in ts])  # noqa: E731
    Ns = (ctypes.c_int64 * n)(*[wq.shape[0] for wq in wqs])
    with torch.cuda.device(dev):
        check(lib.inc_fp8_gemv_multi(n, _ptr(xq), _ptr(row_scale), arr(wqs), arr(alphas), arr(biases), arr(ys), dtype_code(out_dtype),
                                     M, Ns, Kp, _stream()), "inc_fp8_gemv_multi")
    return ys


def fp8_gemv_gated(xq, row_scale, gate_wq, gate_alpha, gate_bias, up_wq, up_alpha, up_bias, out_dtype):
    """silu(g) * u of a gated MLP for up to FP8_GEMV_MAX_M rows in ONE launch (inc_fp8_gemv_gated): g and u are fp8_gemv's values on
    the gate / up weight before their rounding, the product is formed in fp32 and rounded once to `out_dtype` (bf16 / fp16)."""
    dev = _dev(xq, row_scale, gate_wq, gate_alpha, gate_bias, up_wq, up_alpha, up_bias)
    (M, Kp), N = xq.shape, gate_wq.shape[0]
    assert xq.dtype == torch.uint8 and xq.is_contiguous() and row_scale.dtype == torch.float32 and row_scale.numel() == M
    assert up_wq.shape == gate_wq.shape
    _fp8_check_member(xq, gate_wq, gate_alpha)
    _fp8_check_member(xq, up_wq, up_alpha)
    gate_bias, up_bias = [None if b is None else (b if b.dtype == out_dtype else b.to(out_dtype)) for b in (gate_bias, up_bias)]
    h = torch.empty((M, N), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.inc_fp8_gemv_gated(_ptr(xq), _ptr(row_scale), _ptr(gate_wq), _ptr(gate_alpha), _ptr(gate_bias), _ptr(up_wq),
                                     _ptr(up_alpha), _ptr(up_bias), _ptr(h), dtype_code(out_dtype), M, N, Kp, _stream()),
              "inc_fp8_gemv_gated")
    return h


def fp8_moe_gemm(mode, aq, a_scale, route, wq, alpha, T, top_k, routing_weights=None, out=None, out_dtype=None):
    """inc_fp8_moe_gemm (K17e): fp8_gemm's product per expert over the rows of the route's sorted order.  wq [E, N, Kp], alpha fp32
    [E, N] (slice e = fp8_quant_rows of expert e's matrix).  mode 0: gate_up + SiLU product -> [T*k, N/2] of `out_dtype` (bf16 / fp16)
    from aq [T, Kp], a_scale [T]; mode 1: down x routing weight -> fp32 [T*k, N] from aq [T*k, Kp], a_scale [T*k] in sorted order;
    mode 2: plain -> fp32 [T*k, N] from aq [T, Kp].  Rows past the route's valid positions are not written."""
    dev = _dev(aq, a_scale, route, wq, alpha, routing_weights)
    E, N, Kp = wq.shape
    S = T * top_k
    assert aq.dtype == torch.uint8 and wq.dtype == torch.uint8 and a_scale.dtype == torch.float32 and alpha.dtype == torch.float32
    assert aq.shape == ((S if mode == 1 else T), Kp) and a_scale.numel() == aq.shape[0] and alpha.shape == (E, N)
    assert aq.is_contiguous() and a_scale.is_contiguous() and wq.is_contiguous() and alpha.is_contiguous()
    out, odt, wdt = _moe_gemm_out(mode, out, out_dtype, S, N, dev, routing_weights, "fp8_moe_gemm")
    with torch.cuda.device(dev):
        check(lib.inc_fp8_moe_gemm(mode, _ptr(aq), _ptr(a_scale), _ptr(route), _ptr(wq), _ptr(alpha), _ptr(routing_weights), wdt,
                                   _ptr(out), dtype_code(odt), T, top_k, E, N, Kp, _stream()), "inc_fp8_moe_gemm")
    return out
