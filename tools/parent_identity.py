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
Routes per mesh: nin_weights_host over all nodes and over a shuffled subset, interpolate() pipelined (NIN_E2E_MIN_NODES=512), apply()
fused and unfused.  On the composite mesh the all-nodes route runs again under each switch of SWITCHES.
Exit status 1 if an array or a plan differs, or if one of the plan kernels has no nodes on any mesh.  Needs a GPU; reads nothing
outside the repository."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 240
SWITCHES = ("NIN_MFW_LANE_COLUMNS", "NIN_MFW_NO_STRIPS", "NIN_MFW_SMALL_STRIPS", "NIN_GLS_MFW_GENERAL", "NIN_GLS_NO_MFX")
PLANE = (2, 0.0)


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


def child(mesh_name, route_set, out):
    """route_set: 'routes' (all of them) or the name of a switch (the all-nodes route under it)"""
    import numpy as np
    if route_set == "routes":
        os.environ["NIN_E2E_MIN_NODES"] = "512"
    else:
        os.environ[route_set] = "1"
    sys.path.insert(0, ROOT)
    import ninpol_amd
    from ninpol_amd import mesh as M
    from ninpol_amd.interpolator import _run_weights
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=MESHES[mesh_name](M))
    P = int(I.grid.n_points)

    def weights(targets):
        return _run_weights(I.grid, "gls", I.cells_data, I.points_data, I.variable_to_index, "u", np.asarray(targets, dtype=np.int64), False)

    A = {}
    A["all.csr"], A["all.nws"] = weights(())
    if route_set == "routes":
        A["targets.csr"], A["targets.nws"] = weights(np.random.default_rng(5).permutation(P)[:max(1, P // 3)])
        W, A["interp.nws"] = I.interpolate("u", "gls")
        A["interp.data"], A["interp.indices"], A["interp.indptr"] = W.data, W.indices, W.indptr
        A["apply_fused.v"], A["apply_fused.nws"] = I.apply("u", "gls", values=np.random.default_rng(6).random((3, int(I.grid.n_elems))))
        os.environ["NIN_APPLY_NO_FUSION"] = "1"                # (the library reads this switch at every apply call)
        A["apply_unfused.v"], A["apply_unfused.nws"] = I.apply("u", "gls", values=np.random.default_rng(6).random((3, int(I.grid.n_elems))))
    plan = {k: int(v) for k, v in I.grid.gls_plan().items()}
    np.savez(out, __plan__=np.array(json.dumps(plan)), __kernels__=np.array(json.dumps(list(I.grid.PLAN_KERNELS))),
             **{k: np.asarray(v) for k, v in A.items()})


def run_child(lib, mesh_name, route_set, out):
    env = dict(os.environ, NINPOL_AMD_LIB=os.path.abspath(lib))
    for s in SWITCHES + ("NIN_E2E_MIN_NODES", "NIN_APPLY_NO_FUSION"):
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
    jobs = [(m, "routes") for m in MESHES] + [("composite", s) for s in SWITCHES]
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
            label = mesh_name if route_set == "routes" else f"{mesh_name}[{route_set}=1]"
            plans[label] = (pa, pb)
            bad += pa != pb
            for k in sorted(set(a.files) | set(b.files)):
                if k.startswith("__"):
                    continue
                same = k in a.files and k in b.files and np.array_equal(a[k], b[k])
                bad += not same
                lines.append((f"{label}.{k}", str(b[k].shape) if k in b.files else "missing", "equal" if same else "DIFFERENT",
                              int(np.count_nonzero(b[k])) if k in b.files else 0))
            if mesh_name == "delaunay_neumann":
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
    print("Neumann Delaunay mesh: " + ("; ".join(unmet) if unmet else "mfx_boundary has nodes, neumann_ws has non-zero entries"))
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
