#!/usr/bin/env python3
"""Does another build of the library compute the same bits?  python tools/parent_identity.py PARENT_LIB.so [NEW_LIB.so]

For a refactor that must not change a result: every route below runs with PARENT_LIB.so (A) and with NEW_LIB.so (B, default: the
tree's own ninpol_amd/libninpol_amd.so) and every array is compared with np.array_equal -- no tolerance -- as are the gls_plan() dicts.
One fresh child process per (library, mesh, route set): the library is chosen with NINPOL_AMD_LIB, which is read at import.  A child
writes its arrays to an .npz under a temporary directory; this process compares.  Every child runs under its own `timeout -k 10`; after
the first child that fails, faults or times out nothing further is started.

Meshes (small: a few seconds each): jittered hexahedra, a mixed mesh, wedges and a random-cloud Delaunay mesh; the composite of the nine
parts of tests/test_gpu_composite.py (between them all 22 plan kernels have nodes); and a random-cloud Delaunay mesh WITH a Neumann plane,
for which mfx_boundary must have nodes and neumann_ws non-zero entries -- otherwise the boundary-face rows are never computed.
Routes per mesh: nin_weights_host over all nodes and over a shuffled subset (GLS, IDW and LS), interpolate() pipelined
(NIN_E2E_MIN_NODES=512), apply() fused and unfused, apply_transpose() with 3 fields, permeability_gradient() and
permeability_tangent() along two directions.  On the meshes of LOCAL also points_gradient(), points_tangent() along two directions
and permeability_jacobian() -- in the permeability and in the bases "scale", "diagonal", "symmetric" and one per-cell
(n_elems, 3, 9) array, each with neumann_values:
matmat / rmatmat over 5 columns, matvec, rmatvec and to_scipy().data -- and a
scatter of permeability, of points and of Neumann flags (device tensors), each followed by the dirty launch -- weights and neumann_ws
after each -- and by HostMatrix.update(), whose matrix must in the end be a fresh interpolate()'s in the same child.  On the composite
mesh the all-nodes route runs again under each switch set of SWITCHES (NIN_GLS_NO_SMALL is among them because only without the small-node
kernels does the one-wavefront block kernel, block1, get nodes on these meshes; block_only and global_scratch send EVERY node through
kernels_gls_block.hip and kernels_gls.hip), and on the mixed mesh the derivative routes run again under ADJ_SWITCHES (every
system of kernels_gls_adjoint.hip in global-memory scratch).
Exit status 1 if an array or a plan differs, if one of the plan kernels has no nodes on any mesh, if the Neumann Delaunay mesh leaves
one of the adjoint's three LDS bins without nodes, or if under ADJ_SWITCHES a node of the adjoint is left outside the global-scratch
bin (Grid.gls_adjoint_plan(): looked at, not compared).  Needs a GPU; reads nothing
outside the repository."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 240
# a switch set's name -> the variables it sets to 1
SWITCHES = {s: (s,) for s in ("NIN_MFW_LANE_COLUMNS", "NIN_MFW_NO_STRIPS", "NIN_MFW_SMALL_STRIPS", "NIN_GLS_MFW_GENERAL", "NIN_GLS_NO_MFX",
                              "NIN_GLS_NO_SMALL")}
SWITCHES.update(   # (as tests/util.py GLS_ROUTES spells them)
    block_only=("NIN_GLS_NO_GROUP", "NIN_GLS_NO_MFW", "NIN_GLS_NO_MFX", "NIN_GLS_NO_SMALL", "NIN_GLS_NO_QUAD4"),
    global_scratch=("NIN_GLS_NO_GROUP", "NIN_GLS_NO_MFW", "NIN_GLS_FORCE_GLOBAL"))
ADJ_SWITCHES = {"adjoint_global_scratch": ("NIN_GLS_ADJ_FORCE_GLOBAL",)}
PLANE = (2, 0.0)
LOCAL = ("mixed", "delaunay_neumann")


def _composite(M):
    parts = [M.hex_mesh(16, jitter=0.1, seed=1), M.delaunay_tet_mesh(10, seed=4, lattice="random"), M.delaunay_tet_mesh(8, seed=2),
             M.tet_mesh(6, jitter=0.1, seed=3), M.wedge_mesh(6, 5, 4, jitter=0.05, seed=5), M.mixed_mesh(10, 5, 5, jitter=0.1, seed=6),
             M.delaunay_wedge_mesh(12, 6, seed=7, lattice="random"), M.wedge_fan(30, 3), M.wedge_fan(50, 2)]   # test_gpu_composite._parts
    for i, p in enumerate(parts):
        M.attach_fields(p, "u", perm="ALH", neumann_plane=PLANE, seed=20 + i)
    return M.composite_mesh(parts)


def _with_fields(M, mesh, plane):
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=plane, seed=7)
    return mesh


MESHES = {
    "hex_jitter": lambda M: _with_fields(M, M.hex_mesh(20, jitter=0.15, seed=0), PLANE),
    "mixed": lambda M: _with_fields(M, M.mixed_mesh(10, 5, 5, jitter=0.1, seed=0), PLANE),
    "wedge": lambda M: _with_fields(M, M.wedge_mesh(9, 9, 8, jitter=0.05, seed=0), None),
    "delaunay_random": lambda M: _with_fields(M, M.delaunay_tet_mesh(14, seed=0, lattice="random"), None),
    "composite": _composite,
    "delaunay_neumann": lambda M: _with_fields(M, M.delaunay_tet_mesh(10, seed=4, lattice="random"), PLANE),
}


def local_routes(I, A):
    """scatter K, points and flags from device tensors; after each the dirty launch into full buffers and the host matrix's update"""
    import numpy as np
    import torch
    from ninpol_amd.interpolator import DevicePlan
    g = I.grid
    P, E = int(g.n_points), int(g.n_elems)
    rng = np.random.default_rng(11)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    plan = DevicePlan(I, "u", "gls")
    s = torch.cuda.current_stream().cuda_stream
    hm = plan.host_matrix(s)                                   # a full run; clears the dirty set
    csr, nws = torch.zeros(plan.nnz, dtype=torch.float64, device="cuda"), torch.zeros(P, dtype=torch.float64, device="cuda")
    plan.launch(csr.data_ptr(), nws.data_ptr(), s)
    cells, nodes = rng.choice(E, 5, replace=False), rng.choice(P, 7, replace=False)
    on_plane = np.flatnonzero(np.asarray(I.points_coords)[:, PLANE[0]] == PLANE[1])
    flagged = on_plane[:6] if len(on_plane) else nodes
    row = I.variable_to_index["points"]["neumann_flag_u"]
    steps = {
        "perm": lambda: I.update_permeability(dev(rng.uniform(0.5, 2.0, (5, 1, 1)) * np.eye(3)), cells=dev(cells)),
        "points": lambda: I.update_points(dev(np.asarray(I.points_coords)[nodes] + rng.uniform(-1e-3, 1e-3, (7, 3))), nodes=dev(nodes)),
        "flags": lambda: I.update_neumann_flags("u", dev(1.0 - np.asarray(I.points_data)[row][flagged]), nodes=dev(flagged)),
    }
    for name, step in steps.items():
        step()
        A[f"local.{name}.rows"] = np.array(plan.launch_dirty(csr.data_ptr(), nws.data_ptr(), s, clear=False))
        torch.cuda.current_stream().synchronize()
        A[f"local.{name}.csr"], A[f"local.{name}.nws"] = csr.cpu().numpy(), nws.cpu().numpy()
        A[f"local.{name}.hm_rows"] = np.array(hm.update(stream=s))
        W = hm.W
        A[f"local.{name}.hm_data"], A[f"local.{name}.hm_indices"], A[f"local.{name}.hm_indptr"] = W.data.copy(), W.indices.copy(), W.indptr.copy()
        A[f"local.{name}.hm_nws"] = np.array(hm.neumann)
        assert A[f"local.{name}.rows"] > 0 and A[f"local.{name}.hm_rows"] == A[f"local.{name}.rows"], name
    torch.cuda.current_stream().synchronize()
    W, n = I.interpolate("u", "gls")                           # the mesh as it is now, every row
    for got, ref in ((hm.W.data, W.data), (hm.W.indices, W.indices), (hm.W.indptr, W.indptr), (hm.neumann, n)):
        assert np.array_equal(np.asarray(got), np.asarray(ref)), "the host matrix is not a fresh interpolate()'s"
    A["local.interp.data"], A["local.interp.nws"] = W.data, n


def adjoint_routes(I, A, kept=False):
    """permeability_gradient() for 3 node fields, permeability_tangent() along 2 directions (fixed seeds); kept: points_gradient() for 3
    node fields too, points_tangent() along 2 directions, and permeability_jacobian() with neumann_values in the permeability and in
    every kind of basis -- matmat over 5 directions and rmatmat over 5 node fields (5 crosses the chunk of 4 and leaves a chunk of 1),
    matvec, rmatvec, to_scipy().data"""
    import numpy as np
    P, E = int(I.grid.n_points), int(I.grid.n_elems)
    A["perm_gradient.g"] = I.permeability_gradient("u", np.random.default_rng(8).random((3, P)))
    A["perm_tangent.v"], A["perm_tangent.nws"] = I.permeability_tangent("u", np.random.default_rng(9).standard_normal((2, E, 3, 3)))
    if not kept:
        return
    A["points_gradient.g"] = I.points_gradient("u", np.random.default_rng(10).random((3, P)))
    A["points_tangent.v"], A["points_tangent.nws"] = I.points_tangent("u", np.random.default_rng(16).standard_normal((2, P, 3)))
    b = np.random.default_rng(12).standard_normal(P)
    bases = {"perm": None, "scale": "scale", "diagonal": "diagonal", "symmetric": "symmetric",
             "per_cell": np.random.default_rng(13).uniform(-1.0, 1.0, (E, 3, 9))}
    for name, basis in bases.items():
        J = I.permeability_jacobian("u", neumann_values=b, basis=basis)
        D, V = np.random.default_rng(14).standard_normal((J.shape[1], 5)), np.random.default_rng(15).standard_normal((P, 5))
        A[f"jacobian.{name}.matmat"], A[f"jacobian.{name}.rmatmat"] = J.matmat(D), J.rmatmat(V)
        A[f"jacobian.{name}.matvec"], A[f"jacobian.{name}.rmatvec"] = J.matvec(D[:, 0]), J.rmatvec(V[:, 0])
        A[f"jacobian.{name}.scipy"] = J.to_scipy().data
        J.release()


def child(mesh_name, route_set, out):
    """route_set: 'routes' (all of them), a name of SWITCHES (the all-nodes route under it) or of ADJ_SWITCHES (... and adjoint_routes)"""
    import numpy as np
    if route_set == "routes":
        os.environ["NIN_E2E_MIN_NODES"] = "512"
    else:
        for var in {**SWITCHES, **ADJ_SWITCHES}[route_set]:
            os.environ[var] = "1"
    sys.path.insert(0, ROOT)
    if mesh_name in LOCAL and route_set == "routes":
        import torch                                           # (torch's own HIP runtime has to open the device before the library's does)
        torch.cuda.init()
    import ninpol_amd
    from ninpol_amd import mesh as M
    from ninpol_amd.interpolator import _run_weights
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=MESHES[mesh_name](M))
    P = int(I.grid.n_points)

    def weights(targets, meth="gls"):
        return _run_weights(I.grid, meth, I.cells_data, I.points_data, I.variable_to_index, "u", np.asarray(targets, dtype=np.int64), False)

    A = {}
    A["all.csr"], A["all.nws"] = weights(())
    if route_set == "routes":
        subset = np.random.default_rng(5).permutation(P)[:max(1, P // 3)]
        A["targets.csr"], A["targets.nws"] = weights(subset)
        for meth in ("idw", "ls"):
            A[f"{meth}.all.csr"], A[f"{meth}.all.nws"] = weights((), meth)
            A[f"{meth}.targets.csr"], A[f"{meth}.targets.nws"] = weights(subset, meth)
        W, A["interp.nws"] = I.interpolate("u", "gls")
        A["interp.data"], A["interp.indices"], A["interp.indptr"] = W.data, W.indices, W.indptr
        A["apply_fused.v"], A["apply_fused.nws"] = I.apply("u", "gls", values=np.random.default_rng(6).random((3, int(I.grid.n_elems))))
        os.environ["NIN_APPLY_NO_FUSION"] = "1"                # (the library reads this switch at every apply call)
        A["apply_unfused.v"], A["apply_unfused.nws"] = I.apply("u", "gls", values=np.random.default_rng(6).random((3, int(I.grid.n_elems))))
        A["apply_transpose.x"] = I.apply_transpose("u", "gls", np.random.default_rng(8).random((3, P)))
        adjoint_routes(I, A, kept=mesh_name in LOCAL)
        A["__adjoint_bins__"] = np.array(list(I.grid.gls_adjoint_plan().values()))   # (not compared: see main())
        if mesh_name in LOCAL:
            local_routes(I, A)
    elif route_set in ADJ_SWITCHES:
        adjoint_routes(I, A, kept=True)
        A["__adjoint_bins__"] = np.array(list(I.grid.gls_adjoint_plan().values()))   # (not compared: main() wants every node in the last bin)
    plan = {k: int(v) for k, v in I.grid.gls_plan().items()}
    np.savez(out, __plan__=np.array(json.dumps(plan)), __kernels__=np.array(json.dumps(list(I.grid.PLAN_KERNELS))),
             **{k: np.asarray(v) for k, v in A.items()})


def run_child(lib, mesh_name, route_set, out):
    env = dict(os.environ, NINPOL_AMD_LIB=os.path.abspath(lib))
    for s in sum({**SWITCHES, **ADJ_SWITCHES}.values(), ("NIN_E2E_MIN_NODES", "NIN_APPLY_NO_FUSION")):
        env.pop(s, None)
    rc = subprocess.call(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", mesh_name,
                          route_set, out], env=env)
    if rc != 0:
        print(f"STOPPED: the child for {os.path.basename(lib)} / {mesh_name} / {route_set} ended with status {rc}; nothing further was started",
              flush=True)
        sys.exit(2)


def main():
    import numpy as np
    lib_a = sys.argv[1]
    lib_b = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "ninpol_amd", "libninpol_amd.so")
    jobs = [(m, "routes") for m in MESHES] + [("composite", s) for s in SWITCHES] + [("mixed", s) for s in ADJ_SWITCHES]
    lines, plans, bad, kernels, unmet = [], {}, 0, [], []
    with tempfile.TemporaryDirectory() as tmp:
        for mesh_name, route_set in jobs:
            z = []
            for tag, lib in (("a", lib_a), ("b", lib_b)):
                out = os.path.join(tmp, f"{tag}.{mesh_name}.{route_set}.npz")
                run_child(lib, mesh_name, route_set, out)
                z.append(np.load(out))
            a, b = z
            pa, pb = json.loads(str(a["__plan__"])), json.loads(str(b["__plan__"]))
            kernels = json.loads(str(b["__kernels__"]))
            label = mesh_name if route_set == "routes" else f"{mesh_name}[{route_set}{'=1' if SWITCHES.get(route_set) == (route_set,) else ''}]"
            plans[label] = (pa, pb)
            bad += pa != pb
            for k in sorted(set(a.files) | set(b.files)):
                if k.startswith("__"):
                    continue
                same = k in a.files and k in b.files and (np.array_equal(a[k], b[k]) or   # (rows of NaNs, LS on wedges: the same bytes)
                                                          (a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes()))
                bad += not same
                lines.append((f"{label}.{k}", str(b[k].shape) if k in b.files else "missing", "equal" if same else "DIFFERENT",
                              int(np.count_nonzero(b[k])) if k in b.files else 0))
            if route_set in ADJ_SWITCHES and (np.count_nonzero(b["__adjoint_bins__"][:-1]) or not b["__adjoint_bins__"][-1]):
                unmet.append(f"{label}: the adjoint's nodes are not all in the global-scratch bin")
            if mesh_name == "delaunay_neumann":
                if not all(b["__adjoint_bins__"][:3]):
                    unmet.append(f"the Neumann Delaunay mesh leaves an LDS bin of the adjoint empty: {b['__adjoint_bins__'].tolist()}")
                if not pb.get("mfx_boundary", 0) > 0:
                    unmet.append("the Neumann Delaunay mesh has no mfx_boundary nodes")
                if not np.count_nonzero(b["all.nws"]) > 0:
                    unmet.append("the Neumann Delaunay mesh has no non-zero neumann_ws")
    print("parent library (A) against this commit's (B): np.array_equal on every array, no tolerance")
    w = max(len(l[0]) for l in lines)
    for name, shape, verdict, nz in lines:
        print(f"  {name:<{w}}  {shape:<13}  {verdict}  nonzero {nz}")
    print("gls_plan() dicts: " + ("equal" if all(pa == pb for pa, pb in plans.values()) else "DIFFERENT"))
    for label, (pa, pb) in plans.items():
        print(f"  {label}: " + ", ".join(f"{k}={v}" for k, v in pb.items() if v) + ("" if pa == pb else f"   (A: {pa})"))
    covered = [k for k in kernels if any(pb.get(k, 0) for _, pb in plans.values())]
    missing = [k for k in kernels if k not in covered]
    print(f"plan kernels with nodes on at least one mesh ({len(covered)} of {len(kernels)}): " + ", ".join(covered))
    print("plan kernels NOT covered by these meshes: " + (", ".join(missing) or "none"))
    print("coverage conditions: " + ("; ".join(unmet) if unmet else
                                     "the Neumann Delaunay mesh has mfx_boundary nodes, non-zero neumann_ws and nodes in each LDS bin of the adjoint, "
                                     "the forced adjoint runs in global scratch"))
    ok = not bad and not missing and not unmet
    print("RESULT: " + ("all equal, every plan kernel covered" if ok else "DIFFERENT" if bad else "all equal, but a coverage condition above is NOT met"))
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:5])
    elif len(sys.argv) < 2:
        sys.exit(__doc__)
    else:
        sys.exit(main())
