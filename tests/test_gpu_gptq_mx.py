"""GPTQ on the MX grid (inc_gptq_quantize_layer_mx, GPTQConfig(dtype="mx_fp4" | "mx_fp8_e4m3")) against the torch restatement of
tests/gptq_mx_cases.py, and through the public interface."""

import pytest
import torch

from tests import gptq_mx_cases as C

pytestmark = pytest.mark.gpu
FMTS = ("fp4", "fp8_e4m3")


def _solve(hip, N, K, fmt, lookahead=False):
    """-> (qweight, w_scale, Q, Err1 of the first block) of case(N, K) on the GPU, on the CPU."""
    from neural_compressor_amd import ops

    W, _, Hinv = C.case(N, K)
    Q = torch.empty((N, K), dtype=torch.float32, device=hip)
    err_ws = torch.zeros((2, N, 128), dtype=torch.float32, device=hip)
    side = torch.cuda.Stream(device=hip) if lookahead else None
    wq, ws = ops.gptq_quantize_layer_mx(W.to(hip), Hinv.to(hip), Q, err_ws, C.FMT[fmt]["code"],
                                        flags=0 if lookahead else ops.GPTQ_NO_LOOKAHEAD, aux_stream=side)
    torch.cuda.synchronize()
    return wq.cpu(), ws.cpu(), Q.cpu(), err_ws[0].cpu()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,K", [(16, 128), (70, 128), (48, 96)])
def test_single_block_is_the_fp32_restatement_bit_for_bit(hip, fmt, N, K):
    """One chain launch, no lazy update: every operation is an elementwise fp32 op in the restatement's order, so the packed codes, the
    scale bytes, Q and Err1 are its bits.  N = 70: a ragged last wave and workgroup.  K = 96: count = 96, and the padding columns
    96 .. 127 leave as zero codes under byte 0 (C.pack pads with zeros)."""
    codes, bytes_, Q, err = C.reference(N, K, fmt, torch.float32)
    wq, ws, Qg, errg = _solve(hip, N, K, fmt)
    eq, es = C.pack(codes, bytes_, fmt)
    assert torch.equal(wq, eq) and torch.equal(ws, es)
    assert torch.equal(Qg.view(torch.int32), Q.view(torch.int32)) and torch.equal(errg.view(torch.int32), err.view(torch.int32))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,K", [(48, 320), (48, 384), (80, 512)])
def test_multi_block_against_the_fp64_restatement(hip, fmt, N, K):
    """K = 320: a tail of 64; 384: the smallest K at which the look-ahead engages; 512: two look-ahead rounds.
    (a) the two-stream form is bit-identical to INC_GPTQ_NO_LOOKAHEAD; (b) codes and scale bytes agree with the fp64 restatement on
    >= 0.999 of the elements (the integer loop's bar in tests/test_gpu_parity.py; the fp32 restatement shows no mismatch at all on
    these inputs); (c) the layer objective of the GPU's Q is at most round-to-nearest's and within 1 % of the fp64 restatement's --
    the fp32 restatement's objective equals the fp64 one's to six digits here, and a flip of at most 0.1 % of the elements at rounding
    ties, all the lazy update's MFMA summation order can cause, moves the objective by a few times that fraction."""
    W, H, _ = C.case(N, K)
    codes, bytes_, Q64, _ = C.reference(N, K, fmt, torch.float64)
    wq, ws, Q, _ = _solve(hip, N, K, fmt, lookahead=True)
    wq1, ws1, Q1, _ = _solve(hip, N, K, fmt, lookahead=False)
    assert torch.equal(wq, wq1) and torch.equal(ws, ws1) and torch.equal(Q.view(torch.int32), Q1.view(torch.int32))
    code_match = float((C.unpack(wq, fmt, K) == codes).float().mean())
    byte_match = float((ws[:, : K // 32].to(torch.int64) == bytes_).float().mean())
    obj, obj64, obj_rtn = C.objective(W, Q, H), C.objective(W, Q64, H), C.objective(W, C.rtn_mx(W, fmt), H)
    print(f"{fmt} {N}x{K}: codes {code_match:.6f} bytes {byte_match:.6f} objective gpu/fp64 {obj / obj64:.6f} gpu/rtn {obj / obj_rtn:.4f}")
    assert code_match >= 0.999 and byte_match >= 0.999
    assert obj <= obj_rtn and obj <= 1.01 * obj64


@pytest.mark.parametrize("fmt", FMTS)
def test_public_interface_packs_the_solved_weights(hip, fmt, tmp_path, monkeypatch):
    """prepare / calibrate / convert on a two-block Llama: every selected Linear (stacked q/k/v and gate/up solves included) is an
    MXWeightOnlyLinear whose recover() is the Q its block's second forward ran with, bit for bit; lm_head stays float; save / load
    give the state dict back; and every solve's objective on the model's own (damped) Hessian, H = (U^T U)^-1 of the factor U the
    solve ran with, is at most round-to-nearest's.  The objective stands in for a comparison of logits: on this random tiny model
    the logits' mean squared error against the float model is not robustly below round-to-nearest's (gptq / rtn over three seeds:
    0.94, 1.10, 0.44 for fp4; 0.89, 0.81, 0.48 for fp8_e4m3)."""
    from neural_compressor_amd import ops
    from neural_compressor_amd.torch.algorithms.mx_quant import save_load
    from neural_compressor_amd.torch.algorithms.mx_quant.mx_quant import MXWeightOnlyLinear
    from neural_compressor_amd.torch.algorithms.weight_only.gptq import RAWGPTQuantizer
    from neural_compressor_amd.torch.quantization import GPTQConfig, convert, prepare
    from tests.model_zoo import calib_ids, tiny_llama

    solved, pack_one = [], RAWGPTQuantizer._mx_module

    def recording(self, layer, cfg, mx_codes, mx_scales):
        new = pack_one(self, layer, cfg, mx_codes, mx_scales)
        solved.append((layer.weight.data.clone(), new))  # the weight the pack step sees is the block forward's Q
        return new

    monkeypatch.setattr(RAWGPTQuantizer, "_mx_module", recording)
    solves, column_loop = [], ops.gptq_quantize_layer_mx

    def recording_loop(w32, hinv, q_out, *args, **kwargs):
        solves.append((w32.clone(), hinv, q_out))  # the loop consumes w32
        return column_loop(w32, hinv, q_out, *args, **kwargs)

    monkeypatch.setattr(ops, "gptq_quantize_layer_mx", recording_loop)
    ids = calib_ids(n=8, seq=32)
    m = prepare(tiny_llama(), GPTQConfig(dtype="mx_" + fmt, block_size=128))
    for x in ids:
        m(x)
    m = convert(m)
    linears = {n: mod for n, mod in m.named_modules() if isinstance(mod, (torch.nn.Linear, MXWeightOnlyLinear))}
    assert len(solved) == 14 and type(linears.pop("lm_head")) is torch.nn.Linear
    assert all(type(mod) is MXWeightOnlyLinear and mod.w_dtype == fmt for mod in linears.values())
    for Q, mod in solved:
        assert torch.equal(mod.recover(torch.float32), Q)
    m.save(str(tmp_path))
    back = save_load.load(str(tmp_path), tiny_llama(), device="cuda")
    state, state_back = m.state_dict(), back.state_dict()
    assert state.keys() == state_back.keys() and all(torch.equal(state[k], state_back[k]) for k in state)
    assert len(solves) == 8  # per block: q/k/v stacked, o_proj, gate/up stacked, down_proj
    for W, U, Q in solves:
        def objective(q):  # tr(D H D^T) = |D U^-1|^2 for H = (U^T U)^-1
            return float(torch.linalg.solve_triangular(U.double().cpu(), W.double().cpu() - q.double().cpu(), upper=True, left=False).square().sum())

        assert objective(Q) <= objective(C.rtn_mx(W.cpu(), fmt))
