#!/usr/bin/env python3
"""Count the FP64 operations a kernel executes per pass, from its gfx950 ISA (straight-line kernels only: every
instruction of the node loop runs once per pass).  Used for bench.py's EXEC_FLOPS_PER_NODE_HEX.

    python tools/count_fp64.py [source.hip | listing.s] [kernel-name-substring] [lanes per node]
"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ninpol_amd", "csrc", "kernels_gls_hex8mf.hip")
kern = sys.argv[2] if len(sys.argv) > 2 else "nin_gls_hex8w2_kernelILb0"
lanes_per_node = int(sys.argv[3]) if len(sys.argv) > 3 else 4
asm = "/tmp/_count_fp64.s"
sys.path.insert(0, ROOT)
from ninpol_amd.build import UNITS
extra = next((x for f, _, x in UNITS if f == os.path.basename(src)), [])
if src.endswith(".s"):      # an assembly listing kept from another build (the parent's, for a before / after record)
    asm = src
else:
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"] + extra +
                          ["-I", os.path.dirname(src), src, "-o", asm], stderr=subprocess.DEVNULL)
lines = open(asm).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + kern + r"\w*:", l))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))


def count(first, last):
    c = collections.Counter()
    for l in lines[first:last]:
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        c[t.split()[0]] += 1
    return c


def classes(c):
    return (sum(v for k, v in c.items() if k.startswith(("v_fma_f64", "v_fmac_f64"))),
            sum(v for k, v in c.items() if k.startswith(("v_mul_f64", "v_add_f64"))),
            sum(v for k, v in c.items() if k.startswith(("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64", "v_div_", "v_ldexp_f64", "v_frexp", "v_rndne_f64"))),
            sum(v for k, v in c.items() if k.startswith(("v_cvt_f64", "v_cvt_i32_f64"))))


ops = count(start, end)
total = sum(ops.values())
fma, oth, spc, cvt = classes(ops)
print(f"{kern}: {total} instructions in the kernel body (one pass of the node loop + prologue)")
print(f"  FP64 fma {fma}, mul/add {oth}, special {spc}; per lane-pass {2 * fma + oth} flop; per node ({lanes_per_node} lanes) "
      f"{lanes_per_node * (2 * fma + oth)} flop")
for k, v in ops.most_common(25):
    print(f"  {v:6d} {k}")
# Functions the kernel CALLS (noinline: face_tau_t / face_tau_tab_t) are bodies of their own and not in the figures above
# (nor were they in the records of rounds 3 - 5).  One callee, called once per s_swappc_b64 of the straight-line pass:
callees = sorted({m.group(1) for l in lines[start:end] for m in [re.search(r"s_add_u32 .*, (\w+)@rel32@lo", l)] if m and any(l.startswith("\t.type\t" + m.group(1) + ",@function") for l in lines)})
calls = ops["s_swappc_b64"]
if len(callees) == 1 and calls:
    cs = next(i for i, l in enumerate(lines) if l.startswith(callees[0] + ":"))
    ce = next(i for i in range(cs, len(lines)) if lines[i].startswith(".Lfunc_end"))
    cops = count(cs, ce)
    cf, co, csp, ccv = classes(cops)
    ct = sum(cops.values())
    print(f"callee {callees[0]}: {ct} instructions, FP64 fma {cf}, mul/add {co}, special {csp}, conversions {ccv}; called {calls} times a pass")
    print(f"  per pass with the calls: {total + calls * ct} instructions, FP64 fma {fma + calls * cf}, mul/add {oth + calls * co}, "
          f"special {spc + calls * csp}, conversions {cvt + calls * ccv} (all FP64-pipe: {fma + oth + spc + cvt + calls * (cf + co + csp + ccv)}); "
          f"per node ({lanes_per_node} lanes) {lanes_per_node * (2 * (fma + calls * cf) + oth + calls * co)} flop")
elif callees:
    print(f"calls {callees}: not counted")
