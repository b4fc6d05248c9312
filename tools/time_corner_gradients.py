"""The GLS corner gradients (DevicePlan.launch_corner_gradients) beside the tangent in the permeability with the same
number of right-hand sides (DevicePlan.launch_weights_tangent: the nearest existing workload -- one factorisation per node, one extra
solve per direction), same mesh, same session.  python tools/time_corner_gradients.py [hex216 del54 ...]

Per mesh, the cases and the timing of tools/time_adjoint.py (HIP events, WARMUP calls first, median of REPS): the forward launch, then
for n = 1 and 4 the tangent, the gradients alone, the gradients with every optional output (node values, fluxes, nodal mean), and the
gradients' bins one by one (NIN_GLS_ADJ_ONLY); ms, ns per node, the ratio to the tangent, each field beyond the first."""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import ninpol_amd
from ninpol_amd import mesh as M
from time_adjoint import CASES, median_ms


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    if not torch.cuda.is_available():
        raise SystemExit("time_corner_gradients.py needs a GPU")
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
        w = torch.empty(plan.nnz, dtype=torch.float64, device="cuda")
        nws = torch.empty(P, dtype=torch.float64, device="cuda")
        bins = g.gls_adjoint_plan()
        print(f"{name}: P={P} E={E} nnz_esup={plan.nnz}; adjoint bins {bins}", flush=True)
        t_fwd = median_ms(lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream), st)
        print(f"{name}: forward launch {t_fwd:.3f} ms = {t_fwd * 1e6 / P:.1f} ns/node", flush=True)
        del w, nws
        t_tan, t_grd = {}, {}
        for k in (1, 4):
            dK = torch.rand((k, E, 9), dtype=torch.float64, device="cuda") - 0.5
            dw = torch.empty((k, plan.nnz), dtype=torch.float64, device="cuda")
            dn = torch.empty((k, P), dtype=torch.float64, device="cuda")
            t_tan[k] = median_ms(lambda: plan.launch_weights_tangent(dK.data_ptr(), dw.data_ptr(), k, 0, dn.data_ptr(), st.cuda_stream), st)
            assert torch.isfinite(dw).all()
            del dK, dw, dn
            u = torch.rand((k, E), dtype=torch.float64, device="cuda") - 0.5
            grad = torch.empty((k, plan.nnz, 3), dtype=torch.float64, device="cuda")
            t_grd[k] = median_ms(lambda: plan.launch_corner_gradients(u.data_ptr(), grad.data_ptr(), k, stream=st.cuda_stream), st)
            assert torch.isfinite(grad).all()
            vals = torch.empty((k, P), dtype=torch.float64, device="cuda")
            flux = torch.empty((k, plan.nnz, 3), dtype=torch.float64, device="cuda")
            ng = torch.empty((k, P, 3), dtype=torch.float64, device="cuda")
            t_all = median_ms(lambda: plan.launch_corner_gradients(u.data_ptr(), grad.data_ptr(), k, vals.data_ptr(), flux.data_ptr(), ng.data_ptr(),
                                                                   st.cuda_stream), st)
            assert torch.isfinite(flux).all() and torch.isfinite(ng).all() and torch.isfinite(vals).all()
            print(f"{name}: n = {k}: tangent {t_tan[k]:.3f} ms = {t_tan[k] * 1e6 / P:.1f} ns/node; gradients {t_grd[k]:.3f} ms = "
                  f"{t_grd[k] * 1e6 / P:.1f} ns/node; / tangent = {t_grd[k] / t_tan[k]:.2f}; / forward = {t_grd[k] / t_fwd:.1f}; with node values, "
                  f"fluxes and nodal mean {t_all:.3f} ms", flush=True)
            if k == 1:
                try:
                    for b, (label, count) in enumerate(bins.items()):
                        if count == 0:
                            continue
                        os.environ["NIN_GLS_ADJ_ONLY"] = str(b)
                        t = median_ms(lambda: plan.launch_corner_gradients(u.data_ptr(), grad.data_ptr(), 1, stream=st.cuda_stream), st)
                        print(f"{name}: gradients, bin {label}: {count} nodes, {t:.3f} ms = {t * 1e6 / count:.1f} ns/node", flush=True)
                finally:
                    del os.environ["NIN_GLS_ADJ_ONLY"]
            del u, grad, vals, flux, ng
        print(f"{name}: beyond the first: each direction of the tangent {(t_tan[4] - t_tan[1]) / 3:.3f} ms, each field of the gradients "
              f"{(t_grd[4] - t_grd[1]) / 3:.3f} ms = {(t_grd[4] - t_grd[1]) / 3 * 1e6 / P:.1f} ns/node", flush=True)
        I.release_scratch()
        del plan, I


if __name__ == "__main__":
    main()
