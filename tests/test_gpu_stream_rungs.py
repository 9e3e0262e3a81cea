"""-m gpu: the streaming GEMV's three entry points take the same kernel rung.

inc_woq_gemm, inc_woq_gemm_perm and inc_woq_gemm_multi launch the streaming kernel through ONE ladder over (dtype, group lookup, steps
per wave, row blocks, bits) in csrc/gemm_stream.hip; the gathered and the batched form are documented as bit-identical to the plain
one.  For every STREAM_W4 / STREAM_W8 case of tests/gemm_route_cases.py (plus `stream4_8step` widened to two strips), in both dtypes:
  (a) ops.woq_gemm;
  (b) ops.woq_gemm_perm with the identity k_order                                   == (a), bit for bit, on every case;
  (c) the batched launch (ops.WoqGemmGroupCall) of the layer split by columns, concatenated == (a) on every case the library batches.
The library declines a batch only for 8-bit words above 16 rows, and a layer of one strip (N = 64) cannot be split: exactly those cases
go without (c), and the ones that ran cover every 4-bit (row blocks, steps) rung in the group-lookup forms the table has, and the 8-bit
rung with one row block.  No tolerance anywhere: torch.equal.
"""

import pytest
import torch

from tests import gemm_route_cases as R

pytestmark = pytest.mark.gpu

_8STEP = next(c for c in R.CASES if c.name == "stream4_8step")
WIDE_8STEP = _8STEP._replace(name="stream4_8step_n128", N=128)
BASE = [c for c in R.CASES if c.route in ("STREAM_W4", "STREAM_W8")] + [WIDE_8STEP]


def test_widened_8step_case_keeps_its_rung():
    """Host-only query: two strips instead of one still leave fewer than 512 workgroups at 4 steps per wave -> 8 steps."""
    from neural_compressor_amd import ops

    for dtype in (torch.bfloat16, torch.float16):
        got = ops.woq_gemm_route(WIDE_8STEP.M, WIDE_8STEP.N, WIDE_8STEP.K, WIDE_8STEP.group_size, 4, dtype)
        assert (got["route"], got["steps"], got["row_blocks"], got["splitk"]) == ("STREAM_W4", 8, 1, _8STEP.splitk)


def _halves(N):
    """Column split of the batched launch: at 128 (128 + 72, 128 + 136, 128 + 872), the two-strip layer at 64 + 64."""
    cut = 128 if N > 128 else 64
    return (0, cut), (cut, N)


def _one_group_per_4_steps(c):
    """The launcher's group-lookup form (g_shift == -1 or >= 7): one group for the whole of K, or a power of two >= 128."""
    gs = c.group_size
    return gs >= c.K or (gs >= 128 and gs & (gs - 1) == 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_plain_perm_and_multi_take_the_same_rung(hip, dtype):
    from neural_compressor_amd import ops

    ran = []
    for c in BASE:
        what = f"{c.name} {str(dtype)[6:]}"
        got = ops.woq_gemm_route(c.M, c.N, c.K, c.group_size, c.bits, dtype)
        assert (got["route"], got["row_blocks"], got["steps"]) == (c.route, c.row_blocks, c.steps), what
        L = R.make_layer(c.N, c.K, c.group_size, c.bits)
        qw, sc, qz = (torch.from_numpy(L[k]).to(hip) for k in ("qweight", "scales", "qzeros"))
        x, bias = R.make_x(c.M, c.K, dtype).to(hip), R.make_bias(c.N, dtype).to(hip)
        ya = ops.woq_gemm(x, qw, sc, qz, bias, c.N, c.K, c.group_size, c.bits)
        identity = torch.arange(c.K, dtype=torch.int32, device=hip)
        yb = ops.woq_gemm_perm(x, identity, qw, sc, qz, bias, c.N, c.K, c.group_size, c.bits)
        assert torch.equal(ya, yb), f"{what}: inc_woq_gemm_perm with the identity order != inc_woq_gemm"
        if c.N == 64:
            continue  # one strip: nothing to split
        npk = 32 // c.bits
        parts = [(qw[:, a:b].contiguous(), sc[:, a:b].contiguous(), qz[:, a // npk:b // npk].contiguous(), bias[a:b].contiguous(), b - a)
                 for a, b in _halves(c.N)]
        ys = ops.WoqGemmGroupCall(parts, c.K, c.group_size, c.bits, dtype)(x)
        assert (ys is None) == (c.bits == 8 and c.M > 16), f"{what}: the library {'declined' if ys is None else 'took'} the batch"
        if ys is not None:
            assert torch.equal(torch.cat(ys, dim=1), ya), f"{what}: inc_woq_gemm_multi on the column halves != inc_woq_gemm"
            ran.append(c)
    torch.cuda.synchronize()

    def forms(cases, rung):
        return {_one_group_per_4_steps(c) for c in cases if c.bits == 4 and (c.row_blocks, c.steps) == rung}

    for rung in ((1, 4), (2, 4), (4, 4), (1, 8)):
        assert forms(ran, rung) and forms(ran, rung) == forms(BASE, rung), f"4-bit rung {rung}: group-lookup forms batched {forms(ran, rung)}"
    assert any(c.bits == 8 and c.row_blocks == 1 for c in ran)
    assert {c.name for c in BASE} - {c.name for c in ran} == {c.name for c in BASE if c.N == 64 or (c.bits == 8 and c.M > 16)}
