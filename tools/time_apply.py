"""W . u on the device (DevicePlan.apply: weights + row-block apply) per mesh and method: python tools/time_apply.py del54 [mixed10m ...]

Then, on the weights of one plan.launch(add_neumann=True): W . u alone (nin_spmv_device) and its adjoint W^T . v
(nin_spmv_transpose_device), device events around REPS launches after WARMUP, with the achieved rate against 8 TB/s for the
algorithmic bytes  forward: 4(P+1) + 12 nnz + 8 E k + 8 P k   transpose: 4(E+1) + 16 nnz + 8 P k + 8 E k."""
import sys, os
sys.path.insert(0, os.getcwd())
import numpy as np, torch
import ninpol_amd
from ninpol_amd import mesh as M
cases = {"tet40": lambda: M.tet_mesh(40, jitter=0.1), "mixed10m": lambda: M.mixed_mesh(200, 120, 120, jitter=0.1), "hex216": lambda: M.hex_mesh(216, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "delr40": lambda: M.delaunay_tet_mesh(40, seed=0, lattice="random")}
WARMUP, REPS = 3, 20
for name in sys.argv[1:] or ["del54"]:
    m = cases[name](); M.attach_fields(m, "u", perm="ALH")
    I = ninpol_amd.Interpolator(grid_build="device"); I.load_mesh(mesh_obj=m)
    st = torch.cuda.current_stream()
    for meth in os.environ.get("NIN_METHODS", "idw,ls").split(","):
        plan = I.device_plan("u", meth)
        for k in (1, 4):
            u = torch.rand(k, I.grid.n_elems, dtype=torch.float64, device="cuda"); v = torch.empty(k, I.grid.n_points, dtype=torch.float64, device="cuda")
            nws = torch.empty(I.grid.n_points, dtype=torch.float64, device="cuda")
            plan.launch_apply(u.data_ptr(), k, v.data_ptr(), nws.data_ptr(), st.cuda_stream); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(5): plan.launch_apply(u.data_ptr(), k, v.data_ptr(), nws.data_ptr(), st.cuda_stream)
            b.record(st); torch.cuda.synchronize()
            print(f"{name}: P={I.grid.n_points} MX={I.grid.MX_ELEMENTS_PER_POINT} {meth} apply, {k} field(s): {a.elapsed_time(b) / 5:.3f} ms (weights + W.u)", flush=True)
        # the spmv pair on the same weights (the first transpose call builds the cell-major index: part of the warm-up)
        w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda"); nws = torch.empty(I.grid.n_points, dtype=torch.float64, device="cuda")
        plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream, add_neumann=True)
        P, E, nnz = I.grid.n_points, I.grid.n_elems, plan.nnz
        for k in (1, 4):
            u = torch.rand(k, E, dtype=torch.float64, device="cuda"); v = torch.rand(k, P, dtype=torch.float64, device="cuda")
            y = torch.empty(k, P, dtype=torch.float64, device="cuda"); x = torch.empty(k, E, dtype=torch.float64, device="cuda")
            legs = (("W.u  ", lambda: plan.launch_spmv(w.data_ptr(), u.data_ptr(), k, y.data_ptr(), st.cuda_stream),
                     4 * (P + 1) + 12 * nnz + 8 * E * k + 8 * P * k),
                    ("W^T.v", lambda: plan.launch_spmv_transpose(w.data_ptr(), v.data_ptr(), k, x.data_ptr(), st.cuda_stream),
                     4 * (E + 1) + 16 * nnz + 8 * P * k + 8 * E * k))
            for label, run, nbytes in legs:
                for _ in range(WARMUP): run()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(REPS): run()
                b.record(st); torch.cuda.synchronize()
                ms = a.elapsed_time(b) / REPS
                print(f"{name}: {meth} {label} {k} field(s): {ms:.3f} ms, {nbytes / 1e9:.3f} GB algorithmic, "
                      f"{nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / 8e12:.0f} % of 8 TB/s", flush=True)
