"""The kept corner-gradient operator (DevicePlan.gradient_operator) beside the call it replaces
(DevicePlan.launch_corner_gradients), same mesh, same session.  python tools/time_gradop.py [hex216 del54 ...]

Per mesh, the cases and the timing of tools/time_adjoint.py (HIP events, WARMUP calls first, median of REPS): the bytes held, the
factorisation, and for n = 1 and 4 fields the apply, the transposed apply and launch_corner_gradients; ms, the achieved GB/s of each
product against the size of the operator's buffer, the ratio of the per-call solve to the apply, and the break-even number of calls
factorise / (per-call solve - apply).  The spread (min .. max of the REPS) of the per-call solve is printed beside its median."""
import ctypes
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import _lib
from ninpol_amd import mesh as M
from time_adjoint import CASES, REPS, WARMUP, events_ms, median_ms


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    if not torch.cuda.is_available():
        raise SystemExit("time_gradop.py needs a GPU")
    torch.cuda.init()
    st = torch.cuda.current_stream()
    for name in names:
        m = CASES[name]()
        M.attach_fields(m, "u", perm="ALH", neumann_plane=(2, 0.0))
        I = ninpol_amd.Interpolator(grid_build="device")
        I.load_mesh(mesh_obj=m)
        g = I.grid
        P, E = int(g.n_points), int(g.n_elems)
        plan = I.device_plan("u", "gls")
        n_bytes = ctypes.c_int64(0)
        _lib.check(_lib.load().nin_gls_gradop_bytes(g._h, ctypes.byref(n_bytes)))
        print(f"{name}: P={P} E={E} nnz_esup={plan.nnz}; adjoint bins {g.gls_adjoint_plan()}; the operator takes {n_bytes.value} bytes = "
              f"{n_bytes.value / 1e9:.3f} GB", flush=True)
        op = plan.gradient_operator(st.cuda_stream)
        torch.cuda.synchronize()
        t_fac = median_ms(lambda: op.factorize(st.cuda_stream), st)
        print(f"{name}: factorise {t_fac:.3f} ms = {t_fac * 1e6 / P:.1f} ns/node; held {op.nbytes} bytes (operator {8 * op.n_values})", flush=True)
        for k in (1, 4):
            u = torch.rand((k, E), dtype=torch.float64, device="cuda") - 0.5
            grad = torch.empty((k, plan.nnz, 3), dtype=torch.float64, device="cuda")
            t_app = median_ms(lambda: op.launch_apply(u.data_ptr(), grad.data_ptr(), k, stream=st.cuda_stream), st)
            assert torch.isfinite(grad).all()
            gbar = torch.rand((k, plan.nnz, 3), dtype=torch.float64, device="cuda") - 0.5
            ubar = torch.empty((k, E), dtype=torch.float64, device="cuda")
            t_tr = median_ms(lambda: op.launch_apply_transpose(gbar.data_ptr(), ubar.data_ptr(), k, st.cuda_stream), st)
            assert torch.isfinite(ubar).all()
            del gbar, ubar
            run = lambda: plan.launch_corner_gradients(u.data_ptr(), grad.data_ptr(), k, stream=st.cuda_stream)      # noqa: E731
            for _ in range(WARMUP):
                run()
            torch.cuda.synchronize()
            t = events_ms(run, st, REPS)
            t_cg = float(np.median(t))
            gbs = lambda ms: 8 * op.n_values / (ms * 1e-3) / 1e9      # noqa: E731
            even = t_fac / (t_cg - t_app) if t_cg > t_app else float("inf")
            print(f"{name}: n = {k}: apply {t_app:.3f} ms = {gbs(t_app):.0f} GB/s; transposed apply {t_tr:.3f} ms = {gbs(t_tr):.0f} GB/s; "
                  f"launch_corner_gradients {t_cg:.3f} ms (min {min(t):.3f} .. max {max(t):.3f}); per-call solve / apply = {t_cg / t_app:.1f}, "
                  f"/ transposed apply = {t_cg / t_tr:.1f}; break-even after {even:.2f} calls", flush=True)
            del u, grad
        op.release()
        I.release_scratch()
        del op, plan, I


if __name__ == "__main__":
    main()
