"""An incremental interpolate(): what HostMatrix.update() costs against the full call.  python tools/time_hostmatrix.py [hex216 ...]
                                                                                     [--fractions 0.001 0.01 0.1 1.0]

Per mesh (the 216^3 hexahedron mesh by default; ALH K), GLS, for every dirty fraction f: the cells inside a box at the middle of the mesh
that holds f of it get new K rows from the device (update_permeability(cells=), waited for before the clock starts), then
  M.update()                 the dirty rows recomputed, counted, packed, transferred and patched into the scipy matrix
  Interpolator.interpolate() every row, the whole matrix over PCIe: the call this replaces, unchanged code, same session
interleaved, host clock around calls that end in a device synchronise (both are host-synchronous), WARMUP steps first, medians over REPS.
f = 1.0 goes through the same path (every cell scattered: every node marked), not through the full run update() falls back to when
the whole table is replaced; that one is timed as `full fallback`.
The split of update() comes from the library's own laps (NIN_TIMING=1: nin_weights_dirty_device's HIP events and nin_hostmatrix_*'s host
clock, every lap waiting for its work -- so their sum is above the unsplit median): REPS more steps in the same session, medians."""
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import mesh as M

CASES = {"hex216": lambda: M.hex_mesh(216, jitter=0.15), "hex64": lambda: M.hex_mesh(64, jitter=0.15), "hex24": lambda: M.hex_mesh(24, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "del20": lambda: M.delaunay_tet_mesh(20, seed=0)}
WARMUP, REPS = 3, 11
LAPS = ("dirty launch", "count + pack", "D2H", "host patch")


def box_cells(mesh, fraction):
    """the cells whose centroid lies in a box around the middle of the mesh that holds `fraction` of its volume"""
    cen = M.cell_centroids(mesh)
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    half = 0.5 * (hi - lo) * fraction ** (1.0 / 3.0) * (1.0 + 1e-9)
    mid = 0.5 * (lo + hi)
    return np.flatnonzero(np.all(np.abs(cen - mid) <= half, axis=1)).astype(np.int64)


def host_ms(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    return (time.perf_counter() - t0) * 1e3, out


def split_of(run, n):
    """medians of the laps the library prints under NIN_TIMING=1 (stderr is read back through a file)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["NIN_TIMING"] = "1"
        try:
            for i in range(n):
                run(i)
            torch.cuda.synchronize()
        finally:
            del os.environ["NIN_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read()
    out = {}
    for name in LAPS:
        v = [float(x) for x in re.findall(r"\[nin_hostmatrix\] " + re.escape(name) + r"\s+(\S+) ms", text)]
        out[name] = float(np.median(v)) if len(v) == n else float("nan")
    return out


def main():
    args = sys.argv[1:]
    fractions = [0.001, 0.01, 0.1, 1.0]
    if "--fractions" in args:
        j = args.index("--fractions") + 1
        fractions = []
        while j < len(args) and not args[j].startswith("--") and args[j] not in CASES:
            fractions.append(float(args[j]))
            j += 1
        args = args[:args.index("--fractions")] + args[j:]
    names = [a for a in args if not a.startswith("--")] or ["hex216"]
    if not torch.cuda.is_available():
        raise SystemExit("time_hostmatrix.py needs a GPU")
    torch.cuda.init()
    med = lambda a: float(np.median(a))
    for name in names:
        m = CASES[name]()
        M.attach_fields(m, "u", perm="ALH")
        I = ninpol_amd.Interpolator(grid_build="device")
        I.load_mesh(mesh_obj=m)
        g = I.grid
        P, E = int(g.n_points), int(g.n_elems)
        plan = I.device_plan("u", "gls")
        t_first, Mx = host_ms(lambda: plan.host_matrix())
        nnz = int(Mx.W.indptr[-1])
        print(f"{name}: P={P} E={E} nnz={nnz} ({nnz * 12 / 1e9:.3f} GB of indices + data); host_matrix() (first full run, allocations included) "
              f"{t_first:.1f} ms", flush=True)
        v2i = I.variable_to_index["cells"]
        K0 = np.array(I.cells_data[v2i["permeability"]][:E * 9]).reshape(E, 9)
        k_full = [torch.from_numpy(K0).cuda(), torch.from_numpy(1.5 * K0).cuda()]
        inpoel = np.array(g.inpoel)
        for f in fractions:
            cells = box_cells(m, f)
            if len(cells) == 0:
                print(f"{name}: fraction {f:g}: the box holds no cell centroid of this mesh: skipped", flush=True)
                continue
            ids = torch.from_numpy(cells).cuda()
            k_box = [k_full[0][ids].contiguous(), k_full[1][ids].contiguous()]
            scatter = lambda i: I.update_permeability(k_box[i & 1], cells=ids)
            n = 0
            for i in range(WARMUP):
                scatter(i)
                n = Mx.update()
                I.interpolate("u", "gls")
            t_upd, t_full, changed = [], [], 0
            for i in range(REPS):   # interleaved: one incremental step, one full call
                scatter(i)
                t_upd.append(host_ms(Mx.update)[0])
                changed += bool(Mx.structure_changed)
                t_full.append(host_ms(lambda: I.interpolate("u", "gls"))[0])
            laps = split_of(lambda i: (scatter(i), torch.cuda.synchronize(), Mx.update()), REPS)
            dirty = np.arange(P) if len(cells) == E else np.unique(inpoel[cells].reshape(-1))
            rows_bytes = int(np.diff(Mx.W.indptr)[dirty[dirty >= 0]].sum()) * 12 + n * 24      # entries; node, count, offset, neumann_ws per row
            print(f"{name}: fraction {f:g}: {len(cells)} cells, {n} dirty rows of {P} ({100.0 * n / P:.2f} %), {rows_bytes / 1e6:.2f} MB over PCIe "
                  f"against {(nnz * 12 + P * 12) / 1e6:.1f} MB: M.update() median {med(t_upd):.3f} ms (min {min(t_upd):.3f}, max {max(t_upd):.3f}); "
                  f"interpolate() median {med(t_full):.3f} ms (min {min(t_full):.3f}, max {max(t_full):.3f}) over {REPS}; "
                  f"interpolate / update = {med(t_full) / med(t_upd):.2f}; structure changed in {changed} steps", flush=True)
            print(f"{name}: fraction {f:g}: split of update(), medians over {REPS}, each lap waiting for its work: " +
                  ", ".join(f"{k} {laps[k]:.3f} ms" for k in LAPS), flush=True)
        # the fallback: the whole table replaced, every node dirty
        t_fb = []
        for i in range(WARMUP + REPS):
            I.update_permeability(k_full[i & 1])
            t_fb.append(host_ms(Mx.update)[0])
        print(f"{name}: full fallback (whole-array update, every node dirty): M.update() median {med(t_fb[WARMUP:]):.3f} ms over {REPS}", flush=True)
        Mx.release()
        I.release_scratch()
        del Mx, plan, I


if __name__ == "__main__":
    main()
