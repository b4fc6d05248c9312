"""Changing permeability: what a changed K costs by the host route and by the device route.  python tools/time_update_fields.py [hex216 ...]

Per mesh (the 216^3 hexahedron mesh by default), GLS:
  (a)  the host route of a changed K: the table edited in place (numpy, timed on its own), then DevicePlan.refresh() -- hash of the
       tables, upload, flags -- and launch, host clock around calls that end in a device synchronise, median of HOST_REPS;
  (b)  the device route: Interpolator.update_permeability(K_dev) + launch on one stream, HIP events, median of REPS;
  (c)  the update alone (nin_fields_set_permeability_device), HIP events around every call, WARMUP calls first, median of REPS, for
       K at a 16-byte aligned address and at an odd multiple of 8, with and without `scale`; with the bytes the update must move
       (72 in + 80 out per cell, + 8 with a scale) against the 6.29 TB/s copy rate DESIGN uses;
  and the launch alone, for scale.
--profile: only WARMUP + REPS device updates (for a rocprofv3 run around this script)."""
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
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216"]
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
