"""Moving meshes: what Interpolator.update_points costs, and what it replaces.  python tools/time_update.py [hex216 del54 ...]

Per mesh (a 216^3 hexahedron mesh and an unstructured Delaunay tetrahedron mesh by default):
  load   what a caller paid before: load_mesh(grid_build="device") of the moved mesh + the first interpolate()'s plan build
         (nin_grid_to_device), host clock around calls that end in a device synchronise, once;
  (a)    the device-pointer update (nin_grid_update_points_device): HIP events around every call, WARMUP calls first, the median of
         REPS calls; with the bytes the kernels must move at least (connectivity in, coordinates in once, records out) against the
         6.29 TB/s copy rate DESIGN uses;
  (b)    the host-pointer update end to end (upload + kernels + synchronise), host clock, median of REPS;
  (c)    a GLS weights step before and after an update, interleaved in the same process: medians and their difference.
--profile: only WARMUP + REPS device-pointer updates (for a rocprofv3 run around this script)."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import mesh as M

CASES = {"hex216": lambda: M.hex_mesh(216, jitter=0.15), "hex64": lambda: M.hex_mesh(64, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "del20": lambda: M.delaunay_tet_mesh(20, seed=0)}
WARMUP, REPS = 5, 30
COPY_RATE = 6.29e12


def moved(X, a):
    Y = X.copy()
    Y[:, 0] += a * (0.05 * X[:, 1] + 0.01 * np.sin(2.0 * np.pi * X[:, 1]))
    Y[:, 1] += a * (0.03 * X[:, 0] + 0.01 * np.sin(2.0 * np.pi * X[:, 0]))
    Y[:, 2] += a * X[:, 2] * (0.04 * X[:, 0] + 0.01 * np.sin(2.0 * np.pi * X[:, 1]))
    return np.ascontiguousarray(Y)


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


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    profile_only = "--profile" in sys.argv
    if not torch.cuda.is_available():
        raise SystemExit("time_update.py needs a GPU")
    torch.cuda.init()
    st = torch.cuda.current_stream()
    for name in names:
        m = CASES[name]()
        M.attach_fields(m, "u", perm="ALH")
        X0 = np.ascontiguousarray(np.asarray(m.points, dtype=np.float64))
        X1, X2 = moved(X0, 1.0), moved(X0, 0.5)
        t0 = time.perf_counter()
        I = ninpol_amd.Interpolator(grid_build="device")
        I.load_mesh(mesh_obj=m)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        t0 = time.perf_counter()
        I.grid.to_device(I.device)       # what the first interpolate() does first: adopt the arrays, build the GLS launch plan
        torch.cuda.synchronize()
        t_plan = time.perf_counter() - t0
        g = I.grid
        P, E, F = int(g.n_points), int(g.n_elems), int(g.n_faces)
        print(f"{name}: P={P} E={E} F={F}; load_mesh(grid_build='device') {t_load * 1e3:.1f} ms (mesh tables and field packing included) + "
              f"plan build {t_plan * 1e3:.1f} ms", flush=True)
        plan = I.device_plan("u", "gls")
        w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda")
        nws = torch.empty(P, dtype=torch.float64, device="cuda")
        step = lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        x1, x2 = torch.from_numpy(X1).cuda(), torch.from_numpy(X2).cuda()
        upd = [lambda: I.update_points(x1), lambda: I.update_points(x2)]
        if profile_only:
            for i in range(WARMUP + REPS):
                upd[i & 1]()
            torch.cuda.synchronize()
            continue
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        before = events_ms(step, st, REPS)
        for i in range(WARMUP):          # the first call also puts the connectivity copies in place
            upd[i & 1]()
        torch.cuda.synchronize()
        ms = [events_ms(upd[i & 1], st, 1)[0] for i in range(REPS)]
        # the least the three pieces can move: coordinates in and out, [E][8] + [E] + [F][4] indices in, 24 E + (24 + 12 + 8) F out
        nbytes = 48 * P + 33 * E + 16 * F + 24 * E + 44 * F
        med = float(np.median(ms))
        print(f"{name}: (a) update_points(device tensor): median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) over {REPS} calls; "
              f"{nbytes / 1e9:.3f} GB least traffic -> {nbytes / (med * 1e-3) / 1e12:.2f} TB/s = "
              f"{100 * nbytes / (med * 1e-3) / COPY_RATE:.0f} % of the 6.29 TB/s copy rate", flush=True)
        # (c) interleaved: step, update, step, update, ...
        after, mid = [], []
        for i in range(REPS):
            mid += events_ms(step, st, 1)
            upd[i & 1]()
            after += events_ms(step, st, 1)
        b, a, c = float(np.median(before)), float(np.median(after)), float(np.median(mid))
        print(f"{name}: (c) GLS weights step: {b:.3f} ms before any update; interleaved with updates {c:.3f} / {a:.3f} ms "
              f"(step before / after each update): after - before = {a - b:+.3f} ms ({100 * (a - b) / b:+.1f} %); "
              f"update / step = {med / a:.2f}", flush=True)
        hs = []
        for i in range(REPS):
            t0 = time.perf_counter()
            I.update_points((X1, X2)[i & 1])
            hs.append((time.perf_counter() - t0) * 1e3)
        print(f"{name}: (b) update_points(host array), end to end: median {float(np.median(hs)):.2f} ms (min {min(hs):.2f})", flush=True)
        I.release_scratch()
        del plan, I


if __name__ == "__main__":
    main()
