"""Changing Neumann flags: what a changed boundary condition costs by the host route and by the device route.
python tools/time_update_flags.py [hex216 ...] [--counts 1000 10000 100000 1000000]

Per mesh (the 216^3 hexahedron mesh by default), GLS, Neumann plane z = 0:
  (a)  the host route, as before update_neumann_flags(): the flag row edited in place, then DevicePlan.refresh() -- pack, blocking copy of
       the flag bytes -- and a full launch(), host clock around calls that end in a device synchronise, median of HOST_REPS;
  (b)  the whole-array update alone (nin_fields_set_flags_device), HIP events around every call, WARMUP calls first, median of REPS: a
       float64 source at a 16-byte aligned address and at an odd multiple of 8, and a bool source; the two arrays alternate, so every
       call flips the flags of the changed nodes (writes) -- and, for scale, calls that rewrite equal values (no writes at all); with
       the bytes the pass must read (8 or 1 in, + 1 flag byte per node) against the 6.29 TB/s copy rate DESIGN uses;
  (c)  the local step: update_neumann_flags(nodes=ids) for the m nodes lowest in z, whose flags flip every call -- the z = 0 face first
       (Neumann boundary nodes that turn Dirichlet and back), then the layers of interior nodes above it (flagged and unflagged: their GLS
       row moves through neumann_ws) -- + launch_dirty, HIP events around the pair, against refresh() + launch(), for every m of --counts
       that the mesh holds; launch_dirty waits for the stream once (it reads the lists' sizes back), so its events span that wait.
No time is asserted anywhere."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import mesh as M

CASES = {"hex216": lambda: M.hex_mesh(216, jitter=0.15), "hex64": lambda: M.hex_mesh(64, jitter=0.15), "hex16": lambda: M.hex_mesh(16, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "del20": lambda: M.delaunay_tet_mesh(20, seed=0)}
WARMUP, REPS, HOST_REPS = 5, 30, 5
COPY_RATE = 6.29e12


def events_ms(run, stream, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        run()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def odd_view(t):
    """the same values at an address that is an odd multiple of 8 bytes"""
    buf = torch.empty(t.numel() + 3, dtype=t.dtype, device=t.device)
    start = 1 if buf.data_ptr() % 16 == 0 else 2
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def main():
    args = sys.argv[1:]
    counts = [1000, 10000, 100000, 1000000]
    if "--counts" in args:
        j = args.index("--counts") + 1
        counts = []
        while j < len(args) and args[j].isdigit():
            counts.append(int(args[j]))
            j += 1
        args = args[:args.index("--counts")] + args[j:]
    names = [a for a in args if not a.startswith("--")] or ["hex216"]
    if not torch.cuda.is_available():
        raise SystemExit("time_update_flags.py needs a GPU")
    torch.cuda.init()
    st = torch.cuda.current_stream()
    med = lambda a: float(np.median(a))
    for name in names:
        m = CASES[name]()
        M.attach_fields(m, "u", perm="ALH", neumann_plane=(2, 0.0))
        I = ninpol_amd.Interpolator(grid_build="device")
        I.load_mesh(mesh_obj=m)
        g = I.grid
        P = int(g.n_points)
        plan = I.device_plan("u", "gls")
        w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda")
        nws = torch.empty(P, dtype=torch.float64, device="cuda")
        step = lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        row = I.points_data[I.variable_to_index["points"]["neumann_flag_u"]][:P]
        f0 = np.array(row)
        boundary = np.flatnonzero(np.asarray(g.boundary_points) != 0)
        X = np.asarray(m.points, dtype=np.float64)
        face = np.argsort(X[:, 2], kind="stable").astype(np.int64)   # lowest z first: the Neumann face, then the interior layers above it
        print(f"{name}: P={P}, {len(boundary)} boundary nodes, {int(np.count_nonzero(f0))} flagged; the flags are {P * 8 / 1e9:.3f} GB of float64", flush=True)
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        print(f"{name}: GLS weights step alone: median {med(events_ms(step, st, REPS)):.3f} ms", flush=True)

        # (a) the host route
        some = face[:min(len(face), 1000)]
        edit, host = [], []
        for i in range(HOST_REPS):
            t0 = time.perf_counter()
            row[some] = 1.0 - row[some]
            t1 = time.perf_counter()
            plan.refresh()
            step()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            edit.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        row[:] = f0
        plan.refresh()
        t_host = med(host)
        print(f"{name}: (a) host route, refresh() + launch + synchronise: median {t_host:.2f} ms (min {min(host):.2f}, max {max(host):.2f}) over "
              f"{HOST_REPS}; the in-place edit of {len(some)} flags before it: median {med(edit):.3f} ms", flush=True)

        # (b) the whole-array update alone
        f1 = f0.copy()
        f1[some] = 1.0 - f1[some]
        pair = [torch.from_numpy(f1).cuda(), torch.from_numpy(f0).cuda()]
        for label, src, nbytes in (("float64, aligned", pair, 9 * P), ("float64, odd offset", [odd_view(t) for t in pair], 9 * P),
                                   ("bool", [t != 0 for t in pair], 2 * P)):
            for flips in (True, False):
                upd = (lambda i: I.update_neumann_flags("u", src[i & 1])) if flips else (lambda i: I.update_neumann_flags("u", src[1]))
                for i in range(WARMUP + 1):
                    upd(i)
                torch.cuda.synchronize()
                ms = [events_ms(lambda: upd(i), st, 1)[0] for i in range(REPS)]
                upd(1)
                print(f"{name}: (b) whole-array update, {label}, {'flipping ' + str(len(some)) + ' flags' if flips else 'equal values'}: median "
                      f"{med(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}) over {REPS}; {nbytes / 1e9:.3f} GB read -> "
                      f"{nbytes / (med(ms) * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (med(ms) * 1e-3) / COPY_RATE:.0f} % of the 6.29 TB/s copy rate", flush=True)

        # (c) the local step against the full relaunch
        step()
        g.clear_dirty(st.cuda_stream)
        for mcount in counts:
            if mcount > len(face):
                print(f"{name}: (c) {mcount} nodes: the mesh holds only {len(face)} nodes: skipped", flush=True)
                continue
            ids_h = face[:mcount]
            ids = torch.from_numpy(np.ascontiguousarray(ids_h)).cuda()
            vals = [torch.from_numpy(1.0 - f0[ids_h]).cuda(), torch.from_numpy(f0[ids_h]).cuda()]
            scatter = lambda i: I.update_neumann_flags("u", vals[i & 1], nodes=ids)
            dirty = lambda: plan.launch_dirty(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
            n = 0
            for i in range(WARMUP + 1):
                scatter(i)
                n = dirty()
            torch.cuda.synchronize()
            t_local, t_scatter, t_dirty = [], [], []
            for i in range(REPS):
                t_local.append(events_ms(lambda: (scatter(i), dirty()), st, 1)[0])
            for i in range(REPS):
                t_scatter.append(events_ms(lambda: scatter(i), st, 1)[0])
                t_dirty.append(events_ms(dirty, st, 1)[0])
            print(f"{name}: (c) {mcount} nodes ({100.0 * mcount / P:.3f} % of the mesh), {n} rows recomputed: update_neumann_flags(nodes=) + launch_dirty "
                  f"median {med(t_local):.3f} ms (min {min(t_local):.3f}, max {max(t_local):.3f}) = scatter {med(t_scatter):.4f} + launch_dirty "
                  f"{med(t_dirty):.3f} over {REPS}; refresh() + launch() / local step = {t_host / med(t_local):.1f}", flush=True)
        I.release_scratch()
        del plan, I


if __name__ == "__main__":
    main()
