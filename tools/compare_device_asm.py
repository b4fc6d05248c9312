#!/usr/bin/env python3
"""Is the device code of two source trees the same?  python tools/compare_device_asm.py OTHER_CSRC [unit.hip ...]

Compiles every kernel unit (kernels_*.hip, grid_update.hip, grid_device.hip; or the ones named) of ninpol_amd/csrc and of OTHER_CSRC
(another checkout's csrc directory) to device-only gfx950 assembly with the unit's own flags from build.UNITS, the way count_fp64.py
does, and compares the instruction streams kernel by kernel after stripping comments, the compiler ident, file-path lines and the
compilation-unit id (a hash of the source path).  The metadata block at the end of a unit (every kernel's register and scratch
figures) is compared as an entry of its own, "(metadata)".
One line per unit; exit status 1 if any differs.  No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ninpol_amd.build import CSRC, UNITS


def kernels(csrc, unit, extra, tmp):
    """{symbol: [instruction lines]} of one unit's device assembly (the text before the first symbol under '')."""
    asm = os.path.join(tmp, unit + ".s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"] + extra +
                          ["-I", csrc, os.path.join(csrc, unit), "-o", asm], stderr=subprocess.DEVNULL)
    out, name = {"": []}, ""
    for line in open(asm):
        line = re.sub(r"\s*(;|//).*", "", line.rstrip())
        if not line.strip() or re.match(r"\s*\.(ident|file)\b", line) or csrc in line or "__hip_cuid_" in line:
            continue
        m = re.match(r"^(_Z\w+):", line)
        if m or line.strip() == ".amdgpu_metadata":        # (the unit's metadata follows the last kernel: its own entry, not that kernel's)
            name = m.group(1) if m else "(metadata)"
            out[name] = []
        out[name].append(line)
    return out


def main():
    other = os.path.abspath(sys.argv[1])
    units = sys.argv[2:] or [u for u, cc, _ in UNITS if cc == "hipcc" and (u.startswith(("kernels_", "grid_update", "grid_device")))]
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for unit in units:
            extra = next(x for u, _, x in UNITS if u == unit)
            a, b = kernels(CSRC, unit, extra, ta), kernels(other, unit, extra, tb)
            diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
            bad += bool(diff)
            print(f"{unit}: {sum(k.startswith('_Z') for k in a)} symbols, {sum(map(len, a.values()))} lines: " +
                  ("identical" if not diff else "DIFFERENT in " + ", ".join(k or "(preamble)" for k in diff)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
