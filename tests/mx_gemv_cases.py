"""The cases of tests/test_gpu_mx_gemv.py (the decode route of the MX cell: inc_mx_gemv, inc_mx_gemv_multi).  No GPU code.

The oracle is tests/mx_cases.py: the scale rules, the value codes, the exact-sum condition and the bound of an fp32 chain.  Operands are
built here because `exact_operands` there is keyed to its own case list: integers in {0, +-1, +-2, +-3} with scale bytes 125 .. 129, so
every product is a multiple of 2^-4 of at most 144 and, while every partial sum stays below 2^18, every sum is exact in fp32 in any
order -- the result then has ONE right answer, whatever the split of K over the waves.  For Kp <= 1664 the condition holds for any
such operands (144 * 1664 + 8 < 2^18); the cases past that size hold it for the operands built here (their absolute mass is about
7 Kp), and it is asserted for every case and both scale rules when this file is imported.
"""

from collections import namedtuple

import torch

from tests import mx_cases as C

# the kernel as built: one workgroup per strip of STRIP weight rows, WAVES waves that take the K-tiles w, w + WAVES, ..., UNROLL tiles
# of a wave per round of its main loop and a remainder of 1 .. UNROLL - 1 tiles behind it
STRIP, WAVES, UNROLL = 16, 8, 4

VCase = namedtuple("VCase", "name M N Kp y_misaligned")
VCASES = [
    VCase("m1_n1_k1tile", 1, 1, 128, False),            # one row, fewer K-tiles than waves
    VCase("m1_n16_k2tiles", 1, 16, 256, False),         # exactly one strip
    VCase("m1_n17_k8tiles", 1, 17, 1024, False),        # a strip holding one row; one K-tile per wave
    VCase("m2_n15_k5tiles", 2, 15, 640, True),          # 2-byte stores, odd tile count
    VCase("m3_n33_k9tiles", 3, 33, 1152, False),        # more K-tiles than waves: a second tile for one wave only
    VCase("m15_n260_k13tiles", 15, 260, 1664, False),   # M one short of the instruction's 16, N % 4 == 0
    VCase("m16_n64_k3tiles", 16, 64, 384, False),       # full M
    VCase("m16_n515_k8tiles", 16, 515, 1024, False),    # odd N, many strips
    VCase("m5_n1030_k2tiles", 5, 1030, 256, False),     # more workgroups than K work
    # the edges of the kernel as built (WAVES = 8, UNROLL = 4): WAVES - 1 tiles; 3 tiles for every wave (the largest remainder, no
    # main-loop round); one main-loop round for wave 0 only, for two waves, for every wave + one tile more for wave 0; two rounds
    VCase("m4_n20_k7tiles", 4, 20, 896, False),
    VCase("m3_n18_k24tiles", 3, 18, 3072, False),
    VCase("m16_n19_k25tiles", 16, 19, 3200, False),
    VCase("m2_n16_k26tiles", 2, 16, 3328, True),
    VCase("m7_n36_k33tiles", 7, 36, 4224, False),
    VCase("m1_n17_k57tiles", 1, 17, 7296, False),
]
VCASE_IDS = [c.name for c in VCASES]

_exact = {}


def exact_operands(c, rule):
    """values x [M,Kp], w [N,Kp] (int), scale bytes xs [M,Kp/32], ws [N,Kp/32] under C.SCALE_RULES[rule], bias [N] (multiples of 2^-4 up
    to 8) and the exact float64 result without / with bias (the keys of C.exact_operands).  Built once per (case, rule)."""
    key = (c.name, rule)
    if key not in _exact:
        g = torch.Generator().manual_seed(4100 + VCASES.index(c))
        x = torch.randint(-3, 4, (c.M, c.Kp), generator=g)
        w = torch.randint(-3, 4, (c.N, c.Kp), generator=g)
        fx, fw = C.SCALE_RULES[rule]
        nb = c.Kp // 32
        b = torch.arange(nb)[None, :]
        xs = fx(torch.arange(c.M)[:, None], b).to(torch.uint8)
        ws = fw(torch.arange(c.N)[:, None], b).to(torch.uint8)
        bias = torch.randint(-128, 129, (c.N,), generator=g).double() / 16
        xd = (x.double().view(c.M, nb, 32) * torch.ldexp(torch.ones(c.M, nb, dtype=torch.float64), xs.int() - 127)[:, :, None]).view(c.M, c.Kp)
        wd = (w.double().view(c.N, nb, 32) * torch.ldexp(torch.ones(c.N, nb, dtype=torch.float64), ws.int() - 127)[:, :, None]).view(c.N, c.Kp)
        y = xd @ wd.T
        mass = xd.abs() @ wd.abs().T                   # bounds every partial sum of every output, in any order
        _exact[key] = dict(x=x, w=w, xs=xs, ws=ws, bias=bias, y=y, yb=y + bias[None, :], mass=mass, xd=xd, wd=wd)
    return _exact[key]


for _c in VCASES:
    assert _c.Kp % C.KTILE == 0 and 1 <= _c.M <= 16
    for _rule in C.SCALE_RULES:
        C.assert_exact_condition(exact_operands(_c, _rule))
