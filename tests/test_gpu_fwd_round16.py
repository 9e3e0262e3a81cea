"""The fp32 -> 16-bit rounding helper of csrc/fwd_elementwise.hip (inc_probe_round16) against torch's own conversion on the same
device, on bit patterns.  bf16: EVERY fp32 bit pattern -- all NaNs (torch writes 0x7FC0 for each, the hardware conversion alone would
not), the infinities, both zeros, every denormal and every tie.  fp16: a fixed sample of 2^24 patterns plus the special values."""

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24


def _patterns(hip, start):
    """fp32 values with the bit patterns start .. start + 2^24 - 1."""
    return (torch.arange(CHUNK, dtype=torch.int64, device=hip) + start).to(torch.int32).view(torch.float32)


def _differences(x, dtype):
    from neural_compressor_amd import ops

    got = ops.probe_round16(x, dtype)
    return int((got.view(torch.int16) != x.to(dtype).view(torch.int16)).sum())


def test_bf16_every_fp32_bit_pattern(hip):
    wrong = 0
    for c in range(256):
        # chunk c holds the patterns whose top byte is c (as an unsigned number): wrap into int32's range
        start = c * CHUNK
        wrong += _differences(_patterns(hip, start if start < (1 << 31) else start - (1 << 32)), torch.bfloat16)
    assert wrong == 0


SPECIALS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
            0x00000001, 0x807FFFFF, 0x00800000,          # fp32 denormals and the smallest normal
            0x33000000, 0x33000001, 0x33800000,          # around half of fp16's smallest denormal (2^-25: a tie to zero), 2^-24
            0x387FC000, 0x387FE000, 0x38800000,          # fp16 denormal / normal border
            0x477FE000, 0x477FEFFF, 0x477FF000, 0x47800000,  # fp16 max, the last value below the tie, the tie that overflows, 2^16
            0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001]  # ties to even (down, up) and their neighbours


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sample_and_special_values(hip, dtype):
    g = torch.Generator(device="cpu").manual_seed(16)
    sample = torch.randint(-(1 << 31), 1 << 31, (CHUNK,), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([s if s < (1 << 31) else s - (1 << 32) for s in SPECIALS], dtype=torch.int64).to(torch.int32)
    x = torch.cat([sample, special]).to(hip).view(torch.float32)  # 2^24 + 27 values: the n % 8 tail of the kernel runs too
    assert x.numel() % 8 != 0
    assert _differences(x, dtype) == 0
    # every piece with a NaN in any of its eight places, a NaN-free piece in front and behind
    piece = torch.arange(1, 9, dtype=torch.float32)
    rows = [piece.clone()]
    for i in range(8):
        for nan in (0x7F800001, 0xFFC12345):
            p = piece.clone().view(torch.int32)
            p[i] = nan if nan < (1 << 31) else nan - (1 << 32)
            rows.append(p.view(torch.float32))
    rows.append(piece.clone())
    assert _differences(torch.cat(rows).to(hip), dtype) == 0
