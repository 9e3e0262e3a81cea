"""CPU: the block-scaled FP8 cell without a GPU -- the config surface and the argument validation of the four entry points (it runs
before any HIP call)."""

import pytest


def test_config_takes_the_block_pair_and_nothing_mixed():
    from neural_compressor_amd.torch.quantization import FP8Config

    c = FP8Config(act_granularity="per_group", w_granularity="per_block")
    assert (c.fp8_config, c.act_granularity, c.w_granularity) == ("E4M3", "per_group", "per_block")
    d = FP8Config()
    assert (d.act_granularity, d.w_granularity, d.dynamic_quantization, d.moe_experts) == ("per_token", "per_channel", True, False)
    for act, w, names in (("per_token", "per_block", "w_granularity"), ("per_group", "per_channel", "act_granularity"),
                          ("per_group", "per_tensor", "act_granularity.*w_granularity")):
        with pytest.raises(NotImplementedError, match="FP8 on MI355X: .*" + names):
            FP8Config(act_granularity=act, w_granularity=w)


def test_entry_points_validate_their_arguments():
    """NULL, sizes < 1 and misaligned pointers are INC_ERR_BAD_ARG (-1), what is not built INC_ERR_UNSUPPORTED (-2); the fake pointers
    are never dereferenced."""
    from neural_compressor_amd import _lib

    L, p = _lib.lib, 4096
    BF16, F16, F32 = _lib.INC_BF16, _lib.INC_F16, _lib.INC_F32
    for fn in (L.inc_fp8_quant_groups, L.inc_fp8_quant_blocks):  # (x, dtype, rows, K, Kp, codes, scales, stream)
        for hole in (0, 5, 6):
            args = [p, BF16, 1, 128, 128, p, p]
            args[hole] = None
            assert fn(*args, None) == -1
        assert fn(p, BF16, 0, 128, 128, p, p, None) == -1 and fn(p, BF16, 1, 0, 128, p, p, None) == -1
        assert fn(p, BF16, 1, 129, 128, p, p, None) == -1                                          # Kp < K
        assert fn(p, BF16, 1, 128, 128, p + 8, p, None) == -1 and fn(p, BF16, 1, 128, 128, p, p + 2, None) == -1
        assert fn(p, BF16, 1, 100, 192, p, p, None) == -2 and fn(p, 77, 1, 128, 128, p, p, None) == -2
    for fn in (L.inc_fp8_block_gemm, L.inc_fp8_block_gemv):      # (xq, xs, wq, ws, bias, y, ydtype, M, N, Kp, stream)
        for hole in (0, 1, 2, 3, 5):
            args = [p, p, p, p, None, p]
            args[hole] = None
            assert fn(*args, BF16, 1, 4, 128, None) == -1
        for M, N, Kp in ((0, 4, 128), (1, 0, 128), (1, 4, 0), (1, 4, -128)):
            assert fn(p, p, p, p, None, p, BF16, M, N, Kp, None) == -1
        assert fn(p, p, p, p, None, p, BF16, 1, 4, 192, None) == -2 and fn(p, p, p, p, None, p, F32, 1, 4, 128, None) == -2
        assert fn(p + 8, p, p, p, None, p, F16, 1, 4, 128, None) == -1 and fn(p, p, p + 8, p, None, p, F16, 1, 4, 128, None) == -1
        assert fn(p, p + 2, p, p, None, p, F16, 1, 4, 128, None) == -1 and fn(p, p, p, p + 2, None, p, F16, 1, 4, 128, None) == -1
    assert L.inc_fp8_block_gemv(p, p, p, p, None, p, BF16, 17, 4, 128, None) == -2
