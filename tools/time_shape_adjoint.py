"""The GLS adjoint in the node coordinates (dL/d points) beside the K adjoint (dL/dK) and the forward launch: same mesh, same session.
python tools/time_shape_adjoint.py [hex216 del54 ...]

Per mesh: the bins of the adjoint kernel (Grid.gls_adjoint_plan), then HIP events around
  the forward launch (DevicePlan.launch),
  the K backward (DevicePlan.launch_weights_backward: the four bins' kernels + its gather),
  the coordinate backward (DevicePlan.launch_weights_backward_points: the four bins' kernels in their coordinate mode + the three
  gathers of csrc/kernels_gls_shape.hip),
  the three gathers alone (NIN_GLS_ADJ_ONLY with no bin, which the library reads at every call),
WARMUP calls first, median of REPS each; ms and ns per node.  The K adjoint's buffers are given back before the coordinate adjoint
makes its own (at 216^3 hexahedra: 6.4 GB and 10.7 GB).

--tangent: instead, the tangent in the node coordinates (DevicePlan.launch_weights_tangent_points) with n_tangents = 1
and 4 beside the forward launch, the coordinate backward and the K tangent (n_tangents = 1 and 4) of the same session."""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import ninpol_amd
from ninpol_amd import mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_adjoint import CASES, median_ms  # noqa: E402


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    if not torch.cuda.is_available():
        raise SystemExit("time_shape_adjoint.py needs a GPU")
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
        ghat = torch.rand(plan.nnz, dtype=torch.float64, device="cuda") - 0.5
        forward = lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        print(f"{name}: P={P} E={E} F={int(g.n_faces)} nnz_esup={plan.nnz} nnz_fsup={g._scalar('nnz_fsup')}; adjoint bins {g.gls_adjoint_plan()}",
              flush=True)
        t_fwd = median_ms(forward, st)
        if "--tangent" in sys.argv:
            gpts = torch.empty((P, 3), dtype=torch.float64, device="cuda")
            t_x = median_ms(lambda: plan.launch_weights_backward_points(ghat.data_ptr(), gpts.data_ptr(), stream=st.cuda_stream), st)
            assert torch.isfinite(gpts).all()
            del gpts
            I.release_scratch()                            # the coordinate adjoint's buffers go: the tangents make none of them
            t = {}
            for n in (1, 4):
                dw = torch.empty((n, plan.nnz), dtype=torch.float64, device="cuda")
                dK = torch.rand((n, E, 9), dtype=torch.float64, device="cuda") - 0.5
                t["K", n] = median_ms(lambda: plan.launch_weights_tangent(dK.data_ptr(), dw.data_ptr(), n, stream=st.cuda_stream), st)
                assert torch.isfinite(dw).all()
                del dK
                dX = torch.rand((n, P, 3), dtype=torch.float64, device="cuda") - 0.5
                t["X", n] = median_ms(lambda: plan.launch_weights_tangent_points(dX.data_ptr(), dw.data_ptr(), n, stream=st.cuda_stream), st)
                assert torch.isfinite(dw).all()
                del dX, dw
            assert g._scalar("gls_shape_contrib_bytes") == 0 and g._scalar("gls_adjoint_contrib_bytes") == 0
            print(f"{name}: buffers of the coordinate tangent {g._scalar('gls_shape_tangent_bytes') / 1e9:.3f} GB (4 directions)", flush=True)
            print(f"{name}: forward launch {t_fwd:.3f} ms = {t_fwd * 1e6 / P:.1f} ns/node; coordinate backward {t_x:.3f} ms; "
                  f"K tangent {t['K', 1]:.3f} ms (1 direction), {t['K', 4]:.3f} ms (4); "
                  f"coordinate tangent {t['X', 1]:.3f} ms = {t['X', 1] * 1e6 / P:.1f} ns/node (1 direction), {t['X', 4]:.3f} ms (4); "
                  f"coordinate / K tangent = {t['X', 1] / t['K', 1]:.2f} (1), {t['X', 4] / t['K', 4]:.2f} (4); "
                  f"per further direction {(t['X', 4] - t['X', 1]) / 3 / t['X', 1] * 100:.0f} % of the first "
                  f"(K tangent: {(t['K', 4] - t['K', 1]) / 3 / t['K', 1] * 100:.0f} %)", flush=True)
            I.release_scratch()
            del plan, I, ghat, w, nws
            continue
        gperm = torch.empty((E, 9), dtype=torch.float64, device="cuda")
        t_k = median_ms(lambda: plan.launch_weights_backward(ghat.data_ptr(), gperm.data_ptr(), stream=st.cuda_stream), st)
        assert torch.isfinite(gperm).all()
        del gperm
        I.release_scratch()                                # the K adjoint's contribution buffer goes before the coordinate adjoint's come
        gpts = torch.empty((P, 3), dtype=torch.float64, device="cuda")
        shape = lambda: plan.launch_weights_backward_points(ghat.data_ptr(), gpts.data_ptr(), stream=st.cuda_stream)
        t_x = median_ms(shape, st)
        assert torch.isfinite(gpts).all()
        print(f"{name}: buffers of the coordinate adjoint {g._scalar('gls_shape_contrib_bytes') / 1e9:.2f} GB", flush=True)
        try:
            os.environ["NIN_GLS_ADJ_ONLY"] = "9"          # no bin: the three gathers alone
            t_gather = median_ms(shape, st)
        finally:
            del os.environ["NIN_GLS_ADJ_ONLY"]
        print(f"{name}: forward launch {t_fwd:.3f} ms = {t_fwd * 1e6 / P:.1f} ns/node; K backward {t_k:.3f} ms = {t_k * 1e6 / P:.1f} ns/node; "
              f"coordinate backward {t_x:.3f} ms = {t_x * 1e6 / P:.1f} ns/node (its gathers {t_gather:.3f} ms); "
              f"coordinate / K = {t_x / t_k:.2f}; coordinate / forward = {t_x / t_fwd:.1f}", flush=True)
        I.release_scratch()
        del plan, I, gpts, ghat, w, nws


if __name__ == "__main__":
    main()
