"""CPU record of the GPTQ-on-MX restatement (tests/gptq_mx_cases.py): the encoders against torch's own casts, then per format and
shape the fp32 restatement against the fp64 one (code / byte mismatches, objective ratio) and GPTQ / RTN on the objective.
usage: python scripts/gptq_mx_cpu_numerics.py > profiles/mx/gptq_mx_cpu_numerics.log"""
import os
import sys

import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import gptq_mx_cases as C
# sanity of the encoders
x = torch.randn(64, 64) * 0.02
q8 = C.rtn_mx(x, "fp8_e4m3"); b = C.mx_bytes(x.view(64,2,32), "fp8_e4m3")[...,None]
s = torch.ldexp(torch.ones(()), b-127)
ref8 = ((x.view(64,2,32)/s).clamp(-448,448).to(torch.float8_e4m3fn).float()*s).view(64,64)
print("e4m3 rtn == torch float8 cast:", torch.equal(q8, ref8))
GRID = torch.tensor([0,0.5,1,1.5,2,3,4,6.])
b = C.mx_bytes(x.view(64,2,32), "fp4")[...,None]; s = torch.ldexp(torch.ones(()), b-127)
v = (x.view(64,2,32)/s); a=v.abs().clamp(max=6)
near = GRID[(a[...,None]-GRID).abs().argmin(-1)]
print("e2m1 rtn max diff vs nearest grid (ties aside):", float((C.rtn_mx(x,"fp4").view(64,2,32)/s - near*torch.sign(v)).abs().max()))
for fmt in ("fp4", "fp8_e4m3"):
    for (N, K) in [(16,128),(70,128),(48,96),(48,320),(48,384),(80,512)]:
        W, H, Hinv = C.case(N, K)
        c32, b32, Q32, _ = C.reference(N, K, fmt, torch.float32)
        c64, b64, Q64, _ = C.reference(N, K, fmt, torch.float64)
        o32, o64, ortn = C.objective(W, Q32, H), C.objective(W, Q64, H), C.objective(W, C.rtn_mx(W, fmt), H)
        print(fmt, N, K, "code mismatch %.6f byte mismatch %.6f obj32/obj64 %.6f gptq64/rtn %.4f" % (float((c32!=c64).float().mean()), float((b32!=b64).float().mean()), o32/o64, o64/ortn))
