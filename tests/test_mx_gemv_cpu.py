"""CPU: the surface of the MX decode route -- the two entry points exist, are bound, and reject what they do not take before any
HIP call (so this runs without a device); the module's switch and the group function are where the README says."""

import ctypes

from tests import mx_cases as C


def _host_pointer():
    """A 16-byte aligned address inside a host buffer: every call below returns before anything is read through it."""
    buf = (ctypes.c_uint8 * 4096)()
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_entry_points_are_bound_and_the_abi_version_stays():
    from neural_compressor_amd import _lib

    assert "inc_mx_gemv" in _lib.SIGNATURES and "inc_mx_gemv_multi" in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "inc_mx_gemv") and hasattr(lib, "inc_mx_gemv_multi")
    assert _lib.ABI_VERSION == 12 and _lib.lib.inc_abi_version() == 12


def test_gemv_rejects_what_it_does_not_take_without_a_device():
    from neural_compressor_amd import _lib

    L = _lib.lib
    keep, p = _host_pointer()
    bf16, f32 = _lib.INC_BF16, _lib.INC_F32
    assert L.inc_mx_gemv(p, None, C.FP8, p, p, C.FP8, None, p, bf16, 1, 1, 128, None) == -1           # a NULL operand
    assert L.inc_mx_gemv(p, p, C.FP8, None, p, C.FP8, None, p, bf16, 1, 1, 128, None) == -1
    assert L.inc_mx_gemv(p, p, C.FP8, p, p, C.FP8, None, None, bf16, 1, 1, 128, None) == -1
    assert L.inc_mx_gemv(p, p, C.FP8, p, p, C.FP8, None, p, bf16, 0, 1, 128, None) == -1              # M, N < 1
    assert L.inc_mx_gemv(p, p, C.FP8, p, p, C.FP8, None, p, bf16, 1, 0, 128, None) == -1
    assert L.inc_mx_gemv(p, p, C.FP8, p, p, C.FP8, None, p, bf16, 17, 1, 128, None) == -2             # more than 16 rows
    assert L.inc_mx_gemv(p, p, C.FP4, p, p, C.FP8, None, p, bf16, 1, 1, 128, None) == -2              # fp4 activations x fp8 weights
    assert L.inc_mx_gemv(p, p, C.FP8, p, p, C.FP8, None, p, bf16, 1, 1, 96, None) == -2               # Kp % 128 != 0
    assert L.inc_mx_gemv(p, p, C.FP8, p, p, C.FP8, None, p, f32, 1, 1, 128, None) == -2               # an fp32 y
    del keep


def test_gemv_multi_rejects_what_it_does_not_take_without_a_device():
    from neural_compressor_amd import _lib

    L = _lib.lib
    keep, p = _host_pointer()
    bf16 = _lib.INC_BF16

    def call(n, M=1, Kp=128, xfmt=C.FP8, ydtype=bf16, null_member=False):
        ptrs = (ctypes.c_void_p * max(n, 1))(*[p] * max(n, 1))
        wq = (ctypes.c_void_p * max(n, 1))(*[None if null_member and i == n - 1 else p for i in range(max(n, 1))])
        Ns = (ctypes.c_int64 * max(n, 1))(*[1] * max(n, 1))
        return L.inc_mx_gemv_multi(n, p, p, xfmt, wq, ptrs, C.FP8, None, ptrs, ydtype, M, Ns, Kp, None)

    assert call(1) == -2 and call(9) == -2 and call(0) == -2                                            # n outside 2 .. 8
    assert call(2, M=17) == -2 and call(3, Kp=96) == -2 and call(8, xfmt=C.FP4) == -2 and call(2, ydtype=_lib.INC_F32) == -2
    assert call(3, null_member=True) == -1
    assert L.inc_mx_gemv_multi(2, p, p, C.FP8, None, None, C.FP8, None, None, bf16, 1, None, 128, None) == -1
    del keep


def test_module_switch_and_group_function_are_public():
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms import mx_quant
    from neural_compressor_amd.torch.algorithms.mx_quant import MXLinear, mx_linear_group

    assert ops.MX_GEMV_MAX_M == 16
    assert isinstance(MXLinear.DECODE_GEMV, bool) and 1 <= MXLinear.DECODE_MAX_M <= ops.MX_GEMV_MAX_M
    assert callable(mx_linear_group) and "mx_linear_group" in mx_quant.__all__
    assert callable(ops.mx_gemv) and callable(ops.mx_gemv_multi)
