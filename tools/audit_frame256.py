#!/usr/bin/env python3
"""Per-kernel resource and instruction counts of .hip files (test infrastructure, run by hand): compile a change and its parent, diff
the two tables.  A refactor that only moves code must leave every column but the last unchanged.

Each file is compiled device-only to assembly (no GPU needed).  Per kernel: vgpr_count, agpr_count, sgpr_count, private segment size,
SGPR / VGPR spill counts and static LDS size from the kernel's metadata, then the number of instructions whose mnemonic starts with
v_mfma, ds_read / ds_write, global_load / global_store / buffer_, s_barrier, s_waitcnt.

usage: tools/audit_frame256.py [-DNAME ...] file.hip [file.hip ...] > table.txt
"""
import os, re, subprocess, sys, tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(root, "neural_compressor_amd", "csrc")
defs = [a for a in sys.argv[1:] if a.startswith("-D")]
files = [a for a in sys.argv[1:] if not a.startswith("-")]
META = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
        ("sspill", ".sgpr_spill_count"), ("vspill", ".vgpr_spill_count"), ("lds", ".group_segment_fixed_size"))
COUNT = (("mfma", ("v_mfma",)), ("lds_op", ("ds_read", "ds_write")), ("vmem", ("global_load", "global_store", "buffer_")),
         ("barrier", ("s_barrier",)), ("waitcnt", ("s_waitcnt",)))
print("kernel " + " ".join(n for n, _ in META + COUNT))
for f in files:
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-w", "--cuda-device-only", "-S",
                               "-I" + csrc, os.path.abspath(f), "-o", out] + defs)
        asm = open(out).read()
    meta = {}
    for block in asm[asm.find("amdhsa.kernels:"):].split("  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(m.group(1)) if (m := re.search(re.escape(k) + r":\s+(\d+)", block)) else 0 for _, k in META}
    print(f"# {os.path.basename(f)}")
    for name in sorted(meta):
        i = asm.find("\n" + name + ":")
        body = asm[i:asm.find(".Lfunc_end", i)]
        ins = [l.split()[0] for l in body.split("\n") if l.strip() and not l.strip().startswith((";", ".", "#")) and not l.strip().endswith(":")]
        print(name + " " + " ".join(str(meta[name][k]) for _, k in META) + " " + " ".join(str(sum(x.startswith(p) for x in ins)) for _, p in COUNT))
