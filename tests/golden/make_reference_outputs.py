#!/usr/bin/env python3
"""Generate tests/golden/reference_outputs/*.npz from the REFERENCE ITSELF (oracle/_ref, built by oracle/build_ref.py).

Run once where the reference tree is present (`python tests/golden/make_reference_outputs.py [name ...]`: every mesh, or only
the named ones -- a new mesh is added without rewriting the files of the others).  The files are data: the
meshes of tests/test_oracle.py::test_port_matches_reference as generated (points and cell blocks: Qhull's output and the
labelling of a relabelled mesh are stored, not regenerated) and, per mesh, the reference's Grid arrays and the dense weight table and neumann_ws of its prepare() for
IDW, LS and GLS; plus the edge tables of test_host.py::test_edges_match_reference.  Where oracle/_ref is not built, those
two tests compare against these files instead of the live reference.
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import ninpol_oracle as O  # noqa: E402
import test_host  # noqa: E402
import test_oracle  # noqa: E402
import util  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402

OUT = os.path.join(HERE, "reference_outputs")


def main():
    assert O.have_reference(), "build oracle/_ref first (python oracle/build_ref.py)"
    os.makedirs(OUT, exist_ok=True)
    only = set(sys.argv[1:])
    unknown = only - {m[0] for m in test_oracle._meshes()} - {"edges"}
    assert not unknown, f"no such mesh: {sorted(unknown)}"
    for name, mesh, perm, plane in test_oracle._meshes():
        if only and name not in only:
            continue
        out = {"points": mesh.points, "n_blocks": np.array(len(mesh.cells))}
        for b, blk in enumerate(mesh.cells):
            out[f"block{b}_type"] = np.array(blk.type)
            out[f"block{b}_data"] = blk.data
        M.attach_fields(mesh, "u", perm=perm, neumann_plane=plane, seed=7)
        ref = O.OracleInterpolator("reference")
        ref.load_mesh(mesh)
        for k in util.GRID_SCALARS:
            out["grid_" + k] = np.array(getattr(ref.grid, k))
        for k in util.GRID_ARRAYS:
            out["grid_" + k] = np.asarray(getattr(ref.grid, k))
        for meth in ("idw", "ls", "gls"):
            w, nw = ref.prepare(meth, "u")
            out[f"{meth}_weights"] = w
            out[f"{meth}_neumann_ws"] = nw
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")
    if only and "edges" not in only:
        return
    mesh = test_host.edges_mesh()
    args = O.process_mesh(mesh)
    edges = O._ref_driver().build_grid(*args, np.ascontiguousarray(mesh.points), 1).get_data()
    np.savez_compressed(os.path.join(OUT, "edges.npz"), **{k: np.asarray(v) for k, v in edges.items()})
    print("edges", os.path.getsize(os.path.join(OUT, "edges.npz")), "bytes")


if __name__ == "__main__":
    main()
