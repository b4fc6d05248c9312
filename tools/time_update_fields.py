"""Changing permeability: what a changed K costs by the host route and by the device route.  python tools/time_update_fields.py [hex216 ...]

Per mesh (the 216^3 hexahedron mesh by default), GLS:
  (a)  the host route of a changed K: the table edited in place (numpy, timed on its own), then DevicePlan.refresh() -- hash of the
       tables, upload, flags -- and launch, host clock around calls that end in a device synchronise, median of HOST_REPS;
  (b)  the device route: Interpolator.update_permeability(K_dev) + launch on one stream, HIP events, median of REPS;
  (c)  the update alone (nin_fields_set_permeability_device), HIP events around every call, WARMUP calls first, median of REPS, for
       K at a 16-byte aligned address and at an odd multiple of 8, with and without `scale`; with the bytes the update must move
       (72 in + 80 out per cell, + 8 with a scale) against the 6.29 TB/s copy rate DESIGN uses;
  and the launch alone, for scale.
--profile: only WARMUP + REPS device updates (for a rocprofv3 run around this script).
--local FRACTION [FRACTION ...]: instead of (a) .. (c), the LOCAL step against the full step, calls interleaved in one session: the cells
  inside a box at the middle of the mesh that holds that fraction of it; update_permeability(K_box, cells=box) + launch_dirty against
  update_permeability(K) + launch, HIP events around each pair, median of REPS; and the scatter alone.  launch_dirty waits for the
  stream once (it reads the lists' sizes back), so its events span that wait.  The split of the dirty launch into compaction +
  read-back, descriptor kernels and weight kernels comes from the library's own HIP events around the three phases (NIN_TIMING=1 makes
  nin_weights_dirty_device print them on stderr): REPS more local steps in the same session, median of each."""
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


def box_cells(mesh, fraction):
    """the cells whose centroid lies in a box around the middle of the mesh that holds `fraction` of its volume"""
    cen = M.cell_centroids(mesh)
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    half = 0.5 * (hi - lo) * fraction ** (1.0 / 3.0)
    mid = 0.5 * (lo + hi)
    return np.flatnonzero(np.all(np.abs(cen - mid) <= half, axis=1)).astype(np.int64)


def dirty_split(run, n):
    """medians of the three phases nin_weights_dirty_device reports under NIN_TIMING=1 (stderr is read back through a file)"""
    import re
    import tempfile
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
        rows = [tuple(map(float, m.groups())) for m in
                re.finditer(r"\[nin_dirty\] nodes \d+ compact\+readback (\S+) descriptors (\S+) weights (\S+) ms", tmp.read())]
    if len(rows) != n:   # (a launch with an empty set, or one that found everything dirty, reports no phases)
        return [float("nan")] * 3
    return [float(np.median([r[k] for r in rows])) for k in range(3)]


def local_leg(name, mesh, I, plan, step, st, fractions, profile_only):
    g = I.grid
    E = int(g.n_elems)
    v2i = I.variable_to_index["cells"]
    K0 = np.array(I.cells_data[v2i["permeability"]][:E * 9]).reshape(E, 9)
    k_full = [torch.from_numpy(K0).cuda(), torch.from_numpy(1.5 * K0).cuda()]
    w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda")
    nws = torch.empty(int(g.n_points), dtype=torch.float64, device="cuda")
    full = lambda i: (I.update_permeability(k_full[i & 1]), step())
    for f in fractions:
        cells = box_cells(mesh, f)
        if len(cells) == 0:
            print(f"{name}: --local {f:g}: the box holds no cell centroid of this mesh: skipped", flush=True)
            continue
        ids = torch.from_numpy(cells).cuda()
        k_box = [k_full[0][ids].contiguous(), k_full[1][ids].contiguous()]
        scatter = lambda i: I.update_permeability(k_box[i & 1], cells=ids)
        dirty = lambda: plan.launch_dirty(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        full(0)
        plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        g.clear_dirty(st.cuda_stream)
        n = 0
        for i in range(WARMUP):
            scatter(i)
            n = dirty()
        torch.cuda.synchronize()
        if profile_only:
            for i in range(REPS):
                scatter(i)
                dirty()
            torch.cuda.synchronize()
            continue
        t_local, t_full, t_scatter, t_dirty = [], [], [], []
        for i in range(REPS):   # interleaved: one local step, one full step
            t_local.append(events_ms(lambda: (scatter(i), dirty()), st, 1)[0])
            t_full.append(events_ms(lambda: full(i), st, 1)[0])
            g.clear_dirty(st.cuda_stream)   # (the full update marked everything; w is not looked at)
            t_scatter.append(events_ms(lambda: scatter(i), st, 1)[0])
            t_dirty.append(events_ms(dirty, st, 1)[0])
        med = lambda a: float(np.median(a))
        split = dirty_split(lambda i: (scatter(i), dirty()), REPS)
        print(f"{name}: --local {f:g}: {len(cells)} cells ({100.0 * len(cells) / E:.2f} %), {n} dirty nodes of {int(g.n_points)}: "
              f"local step median {med(t_local):.3f} ms (min {min(t_local):.3f}, max {max(t_local):.3f}) = scatter {med(t_scatter):.3f} + "
              f"launch_dirty {med(t_dirty):.3f}; full step median {med(t_full):.3f} ms (min {min(t_full):.3f}, max {max(t_full):.3f}) over {REPS}; "
              f"full / local = {med(t_full) / med(t_local):.2f}", flush=True)
        print(f"{name}: --local {f:g}: split of the local step, medians over {REPS}: scatter {med(t_scatter):.3f} ms, compaction + read-back "
              f"{split[0]:.3f} ms, descriptor kernels {split[1]:.3f} ms, weight kernels {split[2]:.3f} ms", flush=True)


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
    names = [a for a in args if not a.startswith("--")] or ["hex216"]
    profile_only = "--profile" in sys.argv
    if not torch.cuda.is_available():
        raise SystemExit("time_update_fields.py needs a GPU")
    torch.cuda.init()
    st = torch.cuda.current_stream()
    for name in names:
        m = CASES[name]()
        M.attach_fields(m, "u", perm="ALH")
        I = ninpol_amd.Interpolator(grid_build="device")
        I.load_mesh(mesh_obj=m)
        g = I.grid
        P, E = int(g.n_points), int(g.n_elems)
        plan = I.device_plan("u", "gls")
        w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda")
        nws = torch.empty(P, dtype=torch.float64, device="cuda")
        step = lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        v2i = I.variable_to_index["cells"]
        perm_row = I.cells_data[v2i["permeability"]][:E * 9]
        dmag_row = I.cells_data[v2i["diff_mag"]][:E]
        K0 = np.array(perm_row).reshape(E, 9)
        rng = np.random.default_rng(0)
        scale_h = rng.uniform(0.1, 10.0, E)
        k_dev = [torch.from_numpy(K0).cuda(), torch.from_numpy(1.5 * K0).cuda()]
        s_dev = torch.from_numpy(scale_h).cuda()
        print(f"{name}: P={P} E={E}; K is {E * 72 / 1e9:.3f} GB", flush=True)
        upd = lambda i, K=k_dev, s=None: I.update_permeability(K[i & 1], scale=s)
        if fractions:
            local_leg(name, m, I, plan, step, st, fractions, profile_only)
            I.release_scratch()
            del plan, I
            continue
        if profile_only:
            for i in range(WARMUP + REPS):
                upd(i)
            torch.cuda.synchronize()
            continue
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        t_step = float(np.median(events_ms(step, st, REPS)))
        print(f"{name}: GLS weights step alone: median {t_step:.3f} ms", flush=True)

        # (a) the host route
        edit, host = [], []
        for i in range(HOST_REPS):
            f = 1.0 + 0.01 * (i + 1)
            t0 = time.perf_counter()
            np.multiply(K0.reshape(-1), f, out=perm_row)
            dmag_row[:] = I.compute_diffusion_magnitude(perm_row.reshape(E, 9))
            t1 = time.perf_counter()
            plan.refresh()
            step()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            edit.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
        t_host = float(np.median(host))
        print(f"{name}: (a) host route, refresh() + launch + synchronise: median {t_host:.2f} ms (min {min(host):.2f}, max {max(host):.2f}) "
              f"over {HOST_REPS}; the in-place edit of the table + diff_mag before it: median {float(np.median(edit)):.2f} ms", flush=True)

        # (b) the device route
        for i in range(WARMUP):
            upd(i)
            step()
        torch.cuda.synchronize()
        both = [events_ms(lambda: (upd(i), step()), st, 1)[0] for i in range(REPS)]
        t_dev = float(np.median(both))
        print(f"{name}: (b) device route, update_permeability(K_dev) + launch: median {t_dev:.3f} ms (min {min(both):.3f}, max {max(both):.3f}) "
              f"over {REPS}; host route / device route = {t_host / t_dev:.1f}", flush=True)

        # (c) the update alone
        k_odd = [odd_view(k_dev[0]), odd_view(k_dev[1])]
        s_odd = odd_view(s_dev)
        for label, K, s in (("aligned", k_dev, None), ("aligned, scaled", k_dev, s_dev), ("odd offset", k_odd, None),
                            ("odd offset, scaled", k_odd, s_odd)):
            nbytes = (152 + (8 if s is not None else 0)) * E
            for i in range(WARMUP):
                upd(i, K, s)
            torch.cuda.synchronize()
            ms = [events_ms(lambda: upd(i, K, s), st, 1)[0] for i in range(REPS)]
            med = float(np.median(ms))
            print(f"{name}: (c) update alone, {label}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) over "
                  f"{REPS}; {nbytes / 1e9:.3f} GB -> {nbytes / (med * 1e-3) / 1e12:.2f} TB/s = "
                  f"{100 * nbytes / (med * 1e-3) / COPY_RATE:.0f} % of the 6.29 TB/s copy rate", flush=True)
        I.release_scratch()
        del plan, I


if __name__ == "__main__":
    main()
