"""The GLS adjoint (dL/dK) against the forward launch, same mesh, same session.  python tools/time_adjoint.py [hex216 del54 ...]

Per mesh: the bins of the adjoint kernel (Grid.gls_adjoint_plan), then HIP events around
  the forward launch (DevicePlan.launch),
  the whole backward (DevicePlan.launch_weights_backward: the four bins' kernels + the gather),
  the gather alone and every bin alone (NIN_GLS_ADJ_ONLY, which the library reads at every call; the gather runs behind each and is
  subtracted),
WARMUP calls first, median of REPS each; ms and ns per node of the bin.

--tangent: instead of the per-bin part, the tangent (DevicePlan.launch_weights_tangent) with n_tangents = 1 and 4 beside
the forward launch and the backward of the same session: ms, ns per node, the ratio to the backward, each direction beyond the first."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import mesh as M

CASES = {"hex216": lambda: M.hex_mesh(216, jitter=0.15), "hex64": lambda: M.hex_mesh(64, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "del20": lambda: M.delaunay_tet_mesh(20, seed=0),
         "delr24": lambda: M.delaunay_tet_mesh(24, seed=0, lattice="random"), "kuhn40": lambda: M.tet_mesh(40, jitter=0.1)}
WARMUP, REPS = 2, 7


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


def median_ms(run, st):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    return float(np.median(events_ms(run, st, REPS)))


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    if not torch.cuda.is_available():
        raise SystemExit("time_adjoint.py needs a GPU")
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
        gperm = torch.empty((E, 9), dtype=torch.float64, device="cuda")
        forward = lambda: plan.launch(w.data_ptr(), nws.data_ptr(), st.cuda_stream)
        backward = lambda: plan.launch_weights_backward(ghat.data_ptr(), gperm.data_ptr(), stream=st.cuda_stream)
        bins = g.gls_adjoint_plan()
        print(f"{name}: P={P} E={E} nnz_esup={plan.nnz}; adjoint bins {bins}; contribution buffer {plan.nnz * 80 / 1e9:.2f} GB", flush=True)
        t_fwd = median_ms(forward, st)
        t_bwd = median_ms(backward, st)
        print(f"{name}: forward launch {t_fwd:.3f} ms = {t_fwd * 1e6 / P:.1f} ns/node; backward {t_bwd:.3f} ms = {t_bwd * 1e6 / P:.1f} ns/node; "
              f"backward / forward = {t_bwd / t_fwd:.1f}", flush=True)
        if "--tangent" in sys.argv:
            del gperm, ghat
            I.release_scratch()                            # the backward's contribution buffer goes: the tangent needs none
            t_tan = {}
            for k in (1, 4):
                dK = torch.rand((k, E, 9), dtype=torch.float64, device="cuda") - 0.5
                dw = torch.empty((k, plan.nnz), dtype=torch.float64, device="cuda")
                dn = torch.empty((k, P), dtype=torch.float64, device="cuda")
                tangent = lambda: plan.launch_weights_tangent(dK.data_ptr(), dw.data_ptr(), k, 0, dn.data_ptr(), st.cuda_stream)
                t_tan[k] = median_ms(tangent, st)
                assert torch.isfinite(dw).all() and torch.isfinite(dn).all()
                print(f"{name}: tangent, n_tangents = {k}: {t_tan[k]:.3f} ms = {t_tan[k] * 1e6 / P:.1f} ns/node; / backward = "
                      f"{t_tan[k] / t_bwd:.2f}; / forward = {t_tan[k] / t_fwd:.1f}", flush=True)
                del dK, dw, dn
            print(f"{name}: each direction beyond the first {(t_tan[4] - t_tan[1]) / 3:.3f} ms = {(t_tan[4] - t_tan[1]) / 3 * 1e6 / P:.1f} ns/node; "
                  f"contribution buffer allocated: {g._scalar('gls_adjoint_contrib_bytes')} bytes", flush=True)
            del plan, I
            continue
        try:
            os.environ["NIN_GLS_ADJ_ONLY"] = "9"          # no bin: the gather alone
            t_gather = median_ms(backward, st)
            print(f"{name}: gather alone {t_gather:.3f} ms", flush=True)
            for b, (label, count) in enumerate(bins.items()):
                if count == 0:
                    continue
                os.environ["NIN_GLS_ADJ_ONLY"] = str(b)
                t = median_ms(backward, st) - t_gather
                print(f"{name}: bin {label}: {count} nodes, {t:.3f} ms = {t * 1e6 / count:.1f} ns/node", flush=True)
        finally:
            del os.environ["NIN_GLS_ADJ_ONLY"]
        assert torch.isfinite(gperm).all()
        I.release_scratch()
        del plan, I


if __name__ == "__main__":
    main()
