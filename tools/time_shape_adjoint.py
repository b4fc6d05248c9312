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
and 4 beside the forward launch, the coordinate backward and the K tangent (n_tangents = 1 and 4) of the same session.

--jacobian: instead, the kept Jacobian in the node coordinates (DevicePlan.linearize_points; default meshes hex64 and
del20, hex216 where the memory allows): the linearisation, GlsShapeJacobian.launch_jvp and launch_vjp with 1 and 4 directions, beside
the one-shot coordinate tangent and coordinate backward, the three gathers alone and the forward launch of the same session.  Next to
the times: the algorithmic bytes of each product -- records and indices counted once per chunk of directions, the gathered geometry
tangents / shares / slots and the in- and outputs once per direction -- and the rate they give.

--assemble: instead, the same Jacobian assembled as a block-CSR matrix (default meshes hex216 and del54, the 2 M-cell
Delaunay mesh): the first GlsShapeJacobian.pattern() of an object (host clock: allocations, count, scan, one synchronisation, fill) and of
two further objects, launch_assemble (HIP events, median), and PointsJacobian.assemble() on the host, device-to-host copies and the
scipy constructor included (--no-host: left out) -- each beside its algorithmic bytes (records read, geometry and connectivity read
once, 24 bytes per block written) and beside the linearisation of the same run."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch

import ninpol_amd
from ninpol_amd import mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_adjoint import CASES, median_ms  # noqa: E402


APPLY_CHUNK, TRANSPOSE_CHUNK = 4, 2     # directions per pass over the records (csrc/launch.hpp)


def jacobian_bytes(g, nnz_e, n):
    """(J . dX, J^T . v): the bytes the algorithm needs for n directions"""
    P, E, F, nnz_f = int(g.n_points), int(g.n_elems), int(g.n_faces), int(g._scalar("nnz_fsup"))
    chunks = lambda c: -(-n // c)                                        # noqa: E731
    records = 24 * nnz_e + 48 * nnz_f + 24 * P
    # J . dX: per chunk the records, esup / fsup and their row pointers; per direction dX read by the geometry kernels (through inpoel,
    # inpofa) and by the node kernel, dC / dFN written once and gathered per entry, the output
    jvp = chunks(APPLY_CHUNK) * (records + 4 * (nnz_e + nnz_f) + 16 * P + 32 * E + 16 * F) + \
        n * (24 * P + 24 * E + 48 * F + 24 * nnz_e + 48 * nnz_f + 24 * P + 8 * P)
    # J^T . v: per chunk the records, the transpose index (ptr, pos, node), esup / fsup / inpofa; per field v, the slots and shares
    # written once and gathered per entry, the output
    vjp = chunks(TRANSPOSE_CHUNK) * (records + 8 * nnz_e + 4 * E + 4 * (nnz_e + nnz_f) + 16 * P + 16 * F + 16 * nnz_f) + \
        n * (8 * P + 96 * F + 24 * E + 24 * nnz_e + 24 * nnz_f + 24 * P)
    return jvp, vjp


def assembly_bytes(g, nnz_e, n_blocks):
    """(pattern, assemble): the bytes the algorithm needs, every array counted once"""
    P, E, F, nnz_f = int(g.n_points), int(g.n_elems), int(g.n_faces), int(g._scalar("nnz_fsup"))
    connectivity = 4 * (nnz_e + nnz_f) + 8 * (P + 1) + 32 * E + 16 * F            # esup, fsup, their row pointers, inpoel, inpofa
    # the symbolic pass reads the connectivity twice (count, fill), writes the counts, scans them and writes the columns
    pattern = 2 * connectivity + 3 * 8 * (P + 1) + 4 * n_blocks
    # the numeric pass: the records, the connectivity, the pattern, the coordinates and the float32 normals; 24 bytes per block written
    records = 24 * nnz_e + 48 * nnz_f + 24 * P
    assemble = records + connectivity + 8 * (P + 1) + 4 * n_blocks + 24 * P + 12 * F + 24 * n_blocks
    return pattern, assemble


def time_assemble(name, I, plan, st):
    from ninpol_amd.interpolator import GlsShapeJacobian, PointsJacobian
    g = I.grid
    P, E = int(g.n_points), int(g.n_elems)
    u = torch.rand(E, dtype=torch.float64, device="cuda") - 0.5
    b = torch.rand(P, dtype=torch.float64, device="cuda") - 0.5
    J = plan.linearize_points(u.data_ptr(), b.data_ptr(), st.cuda_stream)
    t_lin = median_ms(lambda: J.relinearize(u.data_ptr(), b.data_ptr(), st.cuda_stream), st)
    t_pat = []
    for obj in (J, GlsShapeJacobian(g), GlsShapeJacobian(g)):                   # the pattern needs no linearisation
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_blocks = obj.pattern(st.cuda_stream)[0]
        torch.cuda.synchronize()
        t_pat.append((time.perf_counter() - t0) * 1e3)
        if obj is not J:
            obj.release()
    values = torch.full((n_blocks, 3), float("nan"), dtype=torch.float64, device="cuda")
    t_asm = median_ms(lambda: J.launch_assemble(values.data_ptr(), st.cuda_stream), st)
    assert torch.isfinite(values).all()
    del values
    by_pat, by_asm = assembly_bytes(g, plan.nnz, n_blocks)
    print(f"{name}: n_blocks {n_blocks} = {n_blocks / P:.1f} per node; records {J.record_bytes / 1e9:.3f} GB, pattern "
          f"{(8 * (P + 1) + 4 * n_blocks) / 1e9:.3f} GB, values {24 * n_blocks / 1e9:.3f} GB; linearize {t_lin:.3f} ms", flush=True)
    print(f"{name}: first pattern() {t_pat[0]:.3f} ms (further objects {t_pat[1]:.3f}, {t_pat[2]:.3f} ms), {by_pat / 1e9:.4f} GB algorithmic = "
          f"{by_pat / t_pat[0] / 1e9:.3f} TB/s ({by_pat / t_pat[0] / 1e9 / 6.3 * 100:.1f} % of 6.3 TB/s); {t_pat[0] / t_lin * 100:.1f} % of linearize",
          flush=True)
    print(f"{name}: launch_assemble {t_asm:.4f} ms, {by_asm / 1e9:.4f} GB algorithmic = {by_asm / t_asm / 1e9:.3f} TB/s "
          f"({by_asm / t_asm / 1e9 / 6.3 * 100:.0f} % of 6.3 TB/s); {t_asm / t_lin * 100:.2f} % of linearize", flush=True)
    if "--no-host" not in sys.argv:
        t0 = time.perf_counter()
        A = PointsJacobian(J).assemble()
        t_host = (time.perf_counter() - t0) * 1e3
        print(f"{name}: PointsJacobian.assemble() on the host {t_host:.1f} ms (nnz {A.nnz}, device-to-host copies and the scipy constructor "
              f"included); {t_host / t_lin * 100:.0f} % of linearize", flush=True)
        del A
    J.release()


def time_jacobian(name, I, plan, st, t_fwd):
    g = I.grid
    P, E = int(g.n_points), int(g.n_elems)
    ghat = torch.rand(plan.nnz, dtype=torch.float64, device="cuda") - 0.5
    u = torch.rand(E, dtype=torch.float64, device="cuda") - 0.5
    b = torch.rand(P, dtype=torch.float64, device="cuda") - 0.5
    gpts = torch.empty((P, 3), dtype=torch.float64, device="cuda")
    shape = lambda: plan.launch_weights_backward_points(ghat.data_ptr(), gpts.data_ptr(), stream=st.cuda_stream)   # noqa: E731
    t_back = median_ms(shape, st)
    try:
        os.environ["NIN_GLS_ADJ_ONLY"] = "9"              # no bin: the three gathers alone
        t_gather = median_ms(shape, st)
    finally:
        del os.environ["NIN_GLS_ADJ_ONLY"]
    del gpts
    I.release_scratch()                                    # the one-shot adjoint's buffers go before the object's come
    t = {}
    for n in (1, 4):
        dX = torch.rand((n, P, 3), dtype=torch.float64, device="cuda") - 0.5
        dw = torch.empty((n, plan.nnz), dtype=torch.float64, device="cuda")
        t["tangent", n] = median_ms(lambda: plan.launch_weights_tangent_points(dX.data_ptr(), dw.data_ptr(), n, stream=st.cuda_stream), st)
        del dX, dw
    I.release_scratch()
    J = plan.linearize_points(u.data_ptr(), b.data_ptr(), st.cuda_stream)
    t_lin = median_ms(lambda: J.relinearize(u.data_ptr(), b.data_ptr(), st.cuda_stream), st)
    if "--dirty" in sys.argv:                              # the same object follows a block of rewritten cells
        from time_jacobian import time_dirty
        print(f"{name}: linearize {t_lin:.3f} ms", flush=True)
        time_dirty(name, I, lambda: J.relinearize_dirty(u.data_ptr(), b.data_ptr(), st.cuda_stream), t_lin, st)
        J.release()
        return
    for n in (1, 4):
        dX = torch.rand((n, P, 3), dtype=torch.float64, device="cuda") - 0.5
        v = torch.rand((n, P), dtype=torch.float64, device="cuda") - 0.5
        out = torch.full((n, P), float("nan"), dtype=torch.float64, device="cuda")
        grad = torch.full((n, P, 3), float("nan"), dtype=torch.float64, device="cuda")
        t["jvp", n] = median_ms(lambda: J.launch_jvp(dX.data_ptr(), out.data_ptr(), n, st.cuda_stream), st)
        t["vjp", n] = median_ms(lambda: J.launch_vjp(v.data_ptr(), grad.data_ptr(), n, st.cuda_stream), st)
        assert torch.isfinite(out).all() and torch.isfinite(grad).all()
        del dX, v, out, grad
    assert g._scalar("gls_shape_contrib_bytes") == 0 and g._scalar("gls_shape_tangent_bytes") == 0
    print(f"{name}: kept records {J.record_bytes / 1e9:.3f} GB, with the scratch of 4 directions {J.nbytes / 1e9:.3f} GB", flush=True)
    print(f"{name}: forward launch {t_fwd:.3f} ms; one-shot coordinate backward {t_back:.3f} ms (its gathers {t_gather:.3f} ms); one-shot "
          f"coordinate tangent {t['tangent', 1]:.3f} ms (1 direction), {t['tangent', 4]:.3f} ms (4); linearize {t_lin:.3f} ms", flush=True)
    for key, one_shot, i in (("jvp", t["tangent", 1], 0), ("vjp", t_back, 1)):
        for n in (1, 4):
            by = jacobian_bytes(g, plan.nnz, n)[i]
            print(f"{name}: launch_{key} n={n}: {t[key, n]:.4f} ms, {by / 1e9:.4f} GB algorithmic = {by / t[key, n] / 1e9:.3f} TB/s "
                  f"({by / t[key, n] / 1e9 / 6.3 * 100:.0f} % of 6.3 TB/s)" + (f"; one-shot / kept = {one_shot / t[key, 1]:.1f}" if n == 1 else
                  f"; a further direction {(t[key, 4] - t[key, 1]) / 3:.4f} ms = {(t[key, 4] - t[key, 1]) / 3 / t[key, 1] * 100:.0f} % of the first"),
                  flush=True)
    J.release()


def main():
    jacobian, assemble = "--jacobian" in sys.argv, "--assemble" in sys.argv
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or (["hex64", "del20"] if jacobian else ["hex216", "del54"])
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
        if assemble:
            time_assemble(name, I, plan, st)
            I.release_scratch()
            del plan, I, ghat, w, nws
            continue
        t_fwd = median_ms(forward, st)
        if jacobian:
            time_jacobian(name, I, plan, st, t_fwd)
            I.release_scratch()
            del plan, I, ghat, w, nws
            continue
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
