"""The resident GLS Jacobian against the per-call tangent and backward, same mesh, same session.
python tools/time_jacobian.py [hex216 del54 ...]

Per mesh, HIP events, WARMUP calls first, median of REPS each:
  linearize (DevicePlan.linearize's relinearize: one adjoint launch into the object's buffer),
  launch_jvp with 1 and 4 directions, launch_vjp with 1 and 4,
  the tangent launch with 1 direction and the backward call (what a Krylov iteration costs without the object),
  the gather alone (NIN_GLS_ADJ_ONLY=9: nin_adjoint_gather_kernel reads the same buffer in the same order as launch_vjp).
For the two new kernels the algorithmic bytes, computed here from the shapes -- the buffer and the index once per chunk of four
directions, the directions and the results once each -- and the share of the 6.3 TB/s HBM rate those bytes reach."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import ninpol_amd
from ninpol_amd import mesh as M

CASES = {"hex216": lambda: M.hex_mesh(216, jitter=0.15), "hex64": lambda: M.hex_mesh(64, jitter=0.15),
         "del54": lambda: M.delaunay_tet_mesh(54, seed=0), "del20": lambda: M.delaunay_tet_mesh(20, seed=0)}
WARMUP, REPS = 2, 7
HBM_TBS = 6.3


def median_ms(run, st):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        run()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def jvp_bytes(nnz, E, P, n):
    """C and esup once per chunk of four directions; per direction dperm + ddm-or-fold read (80 E) and the node values written (8 P)"""
    return -(-n // 4) * (80 * nnz + 4 * nnz) + n * (80 * E + 8 * P)


def vjp_bytes(nnz, E, P, n):
    """C and the index (cell_pos, cell_node: 8 nnz; cell_ptr: 4 E) once per chunk; per direction v read (8 P), grad_perm + fold written / read (80 E)"""
    return -(-n // 4) * (80 * nnz + 8 * nnz + 4 * E) + n * (8 * P + 80 * E)


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    if not torch.cuda.is_available():
        raise SystemExit("time_jacobian.py needs a GPU")
    torch.cuda.init()
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    for name in names:
        m = CASES[name]()
        M.attach_fields(m, "u", perm="ALH", neumann_plane=(2, 0.0))
        I = ninpol_amd.Interpolator(grid_build="device")
        I.load_mesh(mesh_obj=m)
        g = I.grid
        P, E = int(g.n_points), int(g.n_elems)
        plan = I.device_plan("u", "gls")
        nnz = plan.nnz
        f64 = dict(dtype=torch.float64, device="cuda")
        u, b = torch.rand(E, **f64) - 0.5, torch.rand(P, **f64) - 0.5
        print(f"{name}: P={P} E={E} nnz_esup={nnz}; Jacobian buffer {nnz * 80 / 1e9:.2f} GB", flush=True)
        J = plan.linearize(u.data_ptr(), b.data_ptr(), s)
        t = {"linearize": median_ms(lambda: J.relinearize(u.data_ptr(), b.data_ptr(), s), st)}
        print(f"{name}: linearize {t['linearize']:.3f} ms", flush=True)
        for k in (1, 4):
            dK, out = torch.rand((k, E, 9), **f64) - 0.5, torch.empty((k, P), **f64)
            t[f"jvp{k}"] = median_ms(lambda: J.launch_jvp(dK.data_ptr(), out.data_ptr(), k, 0, s), st)
            v, gp = torch.rand((k, P), **f64) - 0.5, torch.empty((k, E, 9), **f64)
            t[f"vjp{k}"] = median_ms(lambda: J.launch_vjp(v.data_ptr(), gp.data_ptr(), k, 0, s), st)
            assert torch.isfinite(out).all() and torch.isfinite(gp).all()
            for what, nbytes in ((f"jvp{k}", jvp_bytes(nnz, E, P, k)), (f"vjp{k}", vjp_bytes(nnz, E, P, k))):
                rate = nbytes / (t[what] * 1e-3) / 1e12
                print(f"{name}: launch_{what[:3]}, n = {k}: {t[what]:.3f} ms; {nbytes / 1e9:.3f} GB algorithmic = {rate:.2f} TB/s = "
                      f"{100 * rate / HBM_TBS:.0f} % of {HBM_TBS} TB/s", flush=True)
            del dK, out, v, gp
        dK, dw, dn = torch.rand((1, E, 9), **f64) - 0.5, torch.empty((1, nnz), **f64), torch.empty((1, P), **f64)
        t["tangent1"] = median_ms(lambda: plan.launch_weights_tangent(dK.data_ptr(), dw.data_ptr(), 1, 0, dn.data_ptr(), s), st)
        del dK, dw, dn
        ghat, gperm = torch.rand(nnz, **f64) - 0.5, torch.empty((E, 9), **f64)
        backward = lambda: plan.launch_weights_backward(ghat.data_ptr(), gperm.data_ptr(), stream=s)
        t["backward"] = median_ms(backward, st)
        try:
            os.environ["NIN_GLS_ADJ_ONLY"] = "9"          # no bin: the gather alone
            t["gather"] = median_ms(backward, st)
        finally:
            del os.environ["NIN_GLS_ADJ_ONLY"]
        print(f"{name}: tangent, 1 direction {t['tangent1']:.3f} ms; backward {t['backward']:.3f} ms; gather alone {t['gather']:.3f} ms", flush=True)
        print(f"{name}: tangent / jvp = {t['tangent1'] / t['jvp1']:.0f}; backward / vjp = {t['backward'] / t['vjp1']:.0f}; "
              f"vjp / gather = {t['vjp1'] / t['gather']:.2f}; each direction beyond the first: jvp {(t['jvp4'] - t['jvp1']) / 3:.3f} ms, "
              f"vjp {(t['vjp4'] - t['vjp1']) / 3:.3f} ms", flush=True)
        J.release()
        del ghat, gperm, plan, J
        I.release_scratch()
        del I


if __name__ == "__main__":
    main()
