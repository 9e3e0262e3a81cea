"""MXFP6 (e2m3 / e3m2) for the oracle of tests/mx_cases.py: the two format rows, registered at import so that quant_mx, code_table,
dequant_mx, chain_bound and random_operands serve fp6 unchanged, and the storage of inc_mx_quant_fp6 in plain torch.  No GPU code."""

import torch

from tests import mx_cases as C

E2M3, E3M2 = 2, 3                    # the instruction's format codes (INC_MX_FP6_E2M3, INC_MX_FP6_E3M2)
C._F[E2M3] = dict(emax=2, mb=3, emin=0, bias=1, sat=7.5, sign=0x20)
C._F[E3M2] = dict(emax=4, mb=2, emin=-2, bias=3, sat=28.0, sign=0x20)
C._VALUE_CODE[E2M3] = {0: 0x00, 1: 0x08, 2: 0x10, 3: 0x14}
C._VALUE_CODE[E3M2] = {0: 0x00, 1: 0x0C, 2: 0x10, 3: 0x12}
FMT_NAMES = {C.FP8: "fp8_e4m3", E2M3: "fp6_e2m3", E3M2: "fp6_e3m2", C.FP4: "fp4"}
PAIRS = [(E2M3, E2M3), (E3M2, E3M2), (C.FP8, E2M3), (E2M3, C.FP4)]      # (activation, weight)
PAIR_IDS = ["a6w6_e2m3", "a6w6_e3m2", "a8w6", "a6w4"]


def pack_fp6(codes):
    """[M, Kp] codes < 64 -> [M, Kp * 3/4]: element j of a row in bits 6j .. 6j+5 of the row's little-endian bit string (so block b
    is the 24 bytes at 24 b)."""
    assert codes.shape[1] % 4 == 0 and int(codes.max()) < 64
    c = codes.to(torch.int32).view(codes.shape[0], -1, 4)
    word = c[:, :, 0] | (c[:, :, 1] << 6) | (c[:, :, 2] << 12) | (c[:, :, 3] << 18)
    return torch.stack([word & 0xFF, (word >> 8) & 0xFF, word >> 16], dim=2).to(torch.uint8).reshape(codes.shape[0], -1)


def unpack_fp6(packed):
    b = packed.to(torch.int32).view(packed.shape[0], -1, 3)
    word = b[:, :, 0] | (b[:, :, 1] << 8) | (b[:, :, 2] << 16)
    return torch.stack([(word >> (6 * i)) & 0x3F for i in range(4)], dim=2).to(torch.uint8).reshape(packed.shape[0], -1)


def stored(codes, fmt):
    return pack_fp6(codes) if fmt in (E2M3, E3M2) else C.stored(codes, fmt)
