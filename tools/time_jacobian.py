"""The resident GLS Jacobian against the per-call tangent and backward, same mesh, same session.
python tools/time_jacobian.py [--reduced] [hex216 del54 ...]

Per mesh, HIP events, WARMUP calls first, median of REPS each:
  linearize (DevicePlan.linearize's relinearize: one adjoint launch into the object's buffer),
  launch_jvp with 1 and 4 directions, launch_vjp with 1 and 4,
  the tangent launch with 1 direction and the backward call (what a Krylov iteration costs without the object),
  the gather alone (NIN_GLS_ADJ_ONLY=9: nin_adjoint_gather_kernel reads the same buffer in the same order as launch_vjp).
For the two new kernels the algorithmic bytes, computed here from the shapes -- the buffer and the index once per chunk of four
directions, the directions and the results once each -- and the share of the 6.3 TB/s HBM rate those bytes reach.

--reduced: beside the above, in the same session, the reduced Jacobian for M = 1, 3 and 6 parameters per cell --
linearize_reduced's relinearize, launch_jvp and launch_vjp with 1 and 4 directions, their algorithmic bytes ((8 M + 4) nnz for the
apply, (8 M + 8) nnz + 4 E for the transpose, 8 M E + 8 P more per direction) and ratios to the full products -- and for M = 1 the two
yardsticks: the route CellToNode takes for dscale without it (the torch product dscale * K, then the full launch_jvp) and
nin_spmv_device on the same pattern, which moves the same bytes.

--dirty: instead, the full relinearize and, in the same session, relinearize_dirty with 0.1 %, 1 % and 10 % of the cells
rewritten as one compact block at the middle of the mesh (update_permeability's scatter before every call, outside the events; HIP events
around the call, which waits for the stream once: they span that wait), and the library's own split of the call into compaction +
read-back, seed and adjoint launches (NIN_TIMING=1 makes it print them on stderr): REPS more steps, median of each."""
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


def rjvp_bytes(nnz, E, P, n, M):
    """R and esup once per chunk of four directions; per direction dtheta read (8 M E) and the node values written (8 P)"""
    return -(-n // 4) * (8 * M + 4) * nnz + n * (8 * M * E + 8 * P)


def rvjp_bytes(nnz, E, P, n, M):
    """R and the index (cell_pos, cell_node: 8 nnz; cell_ptr: 4 E) once per chunk; per direction v read (8 P), grad_theta written (8 M E)"""
    return -(-n // 4) * ((8 * M + 8) * nnz + 4 * E) + n * (8 * P + 8 * M * E)


def time_reduced(name, I, plan, J, t, u, b, st):
    """the reduced Jacobian beside the full one `J` whose times are in `t` (same session)"""
    g = I.grid
    P, E, nnz, s = int(g.n_points), int(g.n_elems), plan.nnz, st.cuda_stream
    f64 = dict(dtype=torch.float64, device="cuda")
    for M in (1, 3, 6):
        B = None if M == 1 else torch.rand((M, 9), **f64) - 0.5          # M = 1: the resident permeability; else one shared set
        bp = 0 if B is None else B.data_ptr()
        R = plan.linearize_reduced(u.data_ptr(), M, bp, False, b.data_ptr(), s)
        r = {"linearize": median_ms(lambda: R.relinearize(u.data_ptr(), bp, False, b.data_ptr(), s), st)}
        print(f"{name}: M = {M}: buffer {R.nbytes / 1e9:.3f} GB; linearize {r['linearize']:.3f} ms = {r['linearize'] / t['linearize']:.3f} x "
              f"the full linearize", flush=True)
        for k in (1, 4):
            dth, out = torch.rand((k, E, M), **f64) - 0.5, torch.empty((k, P), **f64)
            r[f"jvp{k}"] = median_ms(lambda: R.launch_jvp(dth.data_ptr(), out.data_ptr(), k, s), st)
            v, gt = torch.rand((k, P), **f64) - 0.5, torch.empty((k, E, M), **f64)
            r[f"vjp{k}"] = median_ms(lambda: R.launch_vjp(v.data_ptr(), gt.data_ptr(), k, s), st)
            assert torch.isfinite(out).all() and torch.isfinite(gt).all()
            for what, nbytes in ((f"jvp{k}", rjvp_bytes(nnz, E, P, k, M)), (f"vjp{k}", rvjp_bytes(nnz, E, P, k, M))):
                rate = nbytes / (r[what] * 1e-3) / 1e12
                print(f"{name}: M = {M}: launch_{what[:3]}, n = {k}: {r[what]:.3f} ms = {r[what] / t[what]:.3f} x the full product; "
                      f"{nbytes / 1e9:.3f} GB algorithmic = {rate:.2f} TB/s = {100 * rate / HBM_TBS:.0f} % of {HBM_TBS} TB/s", flush=True)
            del dth, out, v, gt
        if M == 1:
            # today's route for dscale: the (E, 9) direction dscale * K by torch, then the full product
            K = torch.rand((E, 9), **f64) + 0.5
            for k in (1, 4):
                ds, out = torch.rand((k, E), **f64) - 0.5, torch.empty((k, P), **f64)

                def today():
                    tperm = (K.reshape(1, E, 9) * ds[:, :, None]).contiguous()
                    J.launch_jvp(tperm.data_ptr(), out.data_ptr(), k, 0, s)
                ms = median_ms(today, st)
                print(f"{name}: dscale today (torch dscale * K, full launch_jvp), n = {k}: {ms:.3f} ms = {ms / r[f'jvp{k}']:.2f} x the "
                      f"reduced launch_jvp", flush=True)
                # the same bytes through the CSR kernel: R as a value array on esup's pattern
                w, x = torch.rand(nnz, **f64) - 0.5, torch.rand((k, E), **f64) - 0.5
                ms = median_ms(lambda: plan.launch_spmv(w.data_ptr(), x.data_ptr(), k, out.data_ptr(), s), st)
                print(f"{name}: nin_spmv_device on the same pattern, n = {k}: {ms:.3f} ms; reduced launch_jvp / spmv = {r[f'jvp{k}'] / ms:.2f}",
                      flush=True)
                gx = torch.empty((k, E), **f64)
                vv = torch.rand((k, P), **f64) - 0.5
                ms = median_ms(lambda: plan.launch_spmv_transpose(w.data_ptr(), vv.data_ptr(), k, gx.data_ptr(), s), st)
                print(f"{name}: nin_spmv_transpose_device, n = {k}: {ms:.3f} ms; reduced launch_vjp / spmv_transpose = {r[f'vjp{k}'] / ms:.2f}",
                      flush=True)
                del ds, out, w, x, gx, vv
            del K
        R.release()


def dirty_split(run, n):
    """medians of the three phases a dirty relinearisation reports under NIN_TIMING=1 (stderr is read back through a file)"""
    import re
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["NIN_TIMING"] = "1"
        try:
            for _ in range(n):
                run()
            torch.cuda.synchronize()
        finally:
            del os.environ["NIN_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        rows = [tuple(map(float, m.groups())) for m in
                re.finditer(r"\[nin_jac_dirty\] rows \d+ compact\+readback (\S+) seed (\S+) adjoint (\S+) ms", tmp.read())]
    if len(rows) != n:   # (a call with an empty set, or one that found everything dirty, reports no phases)
        return [float("nan")] * 3
    return [float(np.median([r[k] for r in rows])) for k in range(3)]


def time_dirty(name, I, redo, t_full, st, what="relinearize"):
    """redo() = the object's relinearize_dirty on the stream of `st`, returning its row count; t_full = its full relinearize (ms, this
    session).  Also tools/time_shape_adjoint.py --jacobian --dirty."""
    g = I.grid
    E, P = int(g.n_elems), int(g.n_points)
    C = np.asarray(g.centroids, dtype=np.float64).reshape(E, 3)
    far = np.abs(C - C.mean(axis=0)).max(axis=1)            # a cube around the middle of the mesh grows with this
    order = np.argsort(far, kind="stable")
    del C, far
    g.clear_dirty(st.cuda_stream)                           # the object holds a full result as of now
    for frac in (0.001, 0.01, 0.1):
        m = max(1, int(round(frac * E)))
        cells = torch.from_numpy(np.sort(order[:m])).to("cuda")
        K = (torch.tensor([1.5, 0.1, 0.0, 0.1, 1.2, 0.05, 0.0, 0.05, 1.1], dtype=torch.float64, device="cuda").repeat(m, 1) *
             (1.0 + torch.rand((m, 1), dtype=torch.float64, device="cuda"))).contiguous()
        rows = []

        def step():
            g.scatter_permeability_device(cells, K)        # marks the vertices of the block (outside the events)
            rows.append(redo())

        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            g.scatter_permeability_device(cells, K)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            rows.append(redo())
            b.record(st)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        t = float(np.median(ms))
        assert len(set(rows)) == 1 and 0 < rows[0] < P, rows
        split = dirty_split(step, REPS)
        print(f"{name}: {what}_dirty, {100 * frac:g} % of the cells ({m}) as one block: {rows[0]} rows = {100 * rows[0] / P:.2f} % of the nodes; "
              f"{t:.3f} ms = {t / t_full:.4f} x the full {what} ({t_full:.3f} ms); compaction + read-back {split[0]:.4f} ms, seed {split[1]:.4f} ms, "
              f"adjoint launches {split[2]:.4f} ms; {1e6 * split[2] / rows[0]:.1f} ns per row in the adjoint, full pass {1e6 * t_full / P:.1f} ns per row",
              flush=True)
        del cells, K


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["hex216", "del54"]
    reduced = "--reduced" in sys.argv[1:]
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
        if "--dirty" in sys.argv[1:]:
            time_dirty(name, I, lambda: J.relinearize_dirty(u.data_ptr(), b.data_ptr(), s), t["linearize"], st)
            J.release()
            del plan, J
            I.release_scratch()
            del I
            continue
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
        del ghat, gperm
        if reduced:
            time_reduced(name, I, plan, J, t, u, b, st)
        J.release()
        del plan, J
        I.release_scratch()
        del I


if __name__ == "__main__":
    main()
