"""Moving meshes: what Interpolator.update_points costs, and what it replaces.  python tools/time_update.py [hex216 del54 ...]

Per mesh (a 216^3 hexahedron mesh and an unstructured Delaunay tetrahedron mesh by default):
  load   what a caller paid before: load_mesh(grid_build="device") of the moved mesh + the first interpolate()'s plan build
         (nin_grid_to_device), host clock around calls that end in a device synchronise, once;
  (a)    the device-pointer update (nin_grid_update_points_device): HIP events around every call, WARMUP calls first, the median of
         REPS calls; with the bytes the kernels must move at least (connectivity in, coordinates in once, records out) against the
         6.29 TB/s copy rate DESIGN uses;
  (b)    the host-pointer update end to end (upload + kernels + synchronise), host clock, median of REPS;
  (c)    a GLS weights step before and after an update, interleaved in the same process: medians and their difference.
--profile: only WARMUP + REPS device-pointer updates (for a rocprofv3 run around this script).
--local FRACTION [FRACTION ...]: instead of (a) .. (c), the LOCAL step against the full step, calls interleaved in one session, for two
  sets of moved nodes that each hold that fraction of the mesh's nodes: a contiguous slab under the top of the mesh (a free-surface
  layer) and a random subset.  update_points(rows, nodes=ids) + launch_dirty against update_points(X) + launch, HIP events around each
  pair, WARMUP local steps first, medians (with minimum and maximum) of REPS; and the scatter and the dirty launch alone.
  launch_dirty waits for the stream once (it reads the lists' sizes back), so its events span that wait."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import mesh as M

CASES = {"hex216": lambda: M.hex_mesh(216, jitter=0.15), "hex64": lambda: M.hex_mesh(64, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "del20": lambda: M.delaunay_tet_mesh(20, seed=0),
         "kuhn40": lambda: M.tet_mesh(40, jitter=0.1), "kuhn12": lambda: M.tet_mesh(12, jitter=0.1)}
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


def moved_sets(X, fraction, seed=0):
    """{label: node ids}: `fraction` of the nodes as the slab of highest z (a free-surface layer: contiguous in space) and as a random
    subset"""
    P = len(X)
    m = max(int(round(fraction * P)), 1)
    slab = np.argsort(X[:, 2], kind="stable")[P - m:]
    return {"slab": np.sort(slab).astype(np.int64), "random": np.sort(np.random.default_rng(seed).choice(P, size=m, replace=False)).astype(np.int64)}


def local_leg(name, I, plan, st, X, fractions):
    g = I.grid
    P = int(g.n_points)
    w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda")
    nws = torch.empty(P, dtype=torch.float64, device="cuda")
    x_full = [torch.from_numpy(X[0]).cuda(), torch.from_numpy(X[1]).cuda()]
    step = lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
    dirty = lambda: plan.launch_dirty(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
    full = lambda i: (I.update_points(x_full[i & 1]), step())
    med = lambda a: float(np.median(a))
    for f in fractions:
        for label, nodes in moved_sets(X[0], f).items():
            ids = torch.from_numpy(nodes).cuda()
            rows = [x_full[0][ids].contiguous(), x_full[1][ids].contiguous()]
            scatter = lambda i: I.update_points(rows[i & 1], nodes=ids)
            full(0)
            g.clear_dirty(st.cuda_stream)   # w holds a full result of X[0] as of now
            n = 0
            for i in range(WARMUP):
                scatter(i + 1)
                n = dirty()
            torch.cuda.synchronize()
            t_local, t_full, t_scatter, t_dirty = [], [], [], []
            for i in range(REPS):   # interleaved: one local step, one full step
                t_local.append(events_ms(lambda: (scatter(i), dirty()), st, 1)[0])
                t_full.append(events_ms(lambda: full(i), st, 1)[0])
                g.clear_dirty(st.cuda_stream)   # (the full update marked everything; w is not looked at)
                t_scatter.append(events_ms(lambda: scatter(i + 1), st, 1)[0])
                t_dirty.append(events_ms(dirty, st, 1)[0])
            print(f"{name}: --local {f:g} {label}: {len(nodes)} nodes ({100.0 * len(nodes) / P:.2f} %), {n} dirty nodes of {P}: "
                  f"local step median {med(t_local):.3f} ms (min {min(t_local):.3f}, max {max(t_local):.3f}) = scatter {med(t_scatter):.3f} + "
                  f"launch_dirty {med(t_dirty):.3f}; full step median {med(t_full):.3f} ms (min {min(t_full):.3f}, max {max(t_full):.3f}) "
                  f"over {REPS}; full / local = {med(t_full) / med(t_local):.2f}", flush=True)


def main():
    args = sys.argv[1:]
    fractions = []
    if "--local" in args:
        j = args.index("--local") + 1
        while j < len(args) and not args[j].startswith("--") and args[j] not in CASES:
            fractions.append(float(args[j]))
            j += 1
        if not fractions:
            raise SystemExit("--local needs at least one fraction, e.g. --local 0.001 0.01 0.1")
        args = args[:args.index("--local")] + args[j:]
    names = [a for a in args if not a.startswith("--")] or ["hex216", "del54"]
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
        if fractions:
            local_leg(name, I, plan, st, (X1, X2), fractions)
            I.release_scratch()
            del plan, I
            continue
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
