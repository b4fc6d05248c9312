"""The inputs of tests/test_gpu_rows_paths.py, pinned on the CPU with the oracle alone: every mesh of tests/rows_paths.py reaches the
path it was made for, so that the GPU tests cannot pass by missing the branch.  These are conditions on the inputs, not measurements;
every threshold lies under the figure counted when the meshes were made (the docstrings of rows_paths.py carry those)."""
import numpy as np
import pytest

import rows_paths as R
from ninpol_amd import mesh as M


def oracle_of(oracle_lib, mesh):
    o = oracle_lib.OracleInterpolator("port", threads=4)
    o.load_mesh(mesh)
    return o


@pytest.mark.parametrize("at", [0, 70])
def test_fan_has_one_tile_past_the_cap(oracle_lib, at):
    g = oracle_of(oracle_lib, R.fan_fields(R.fan_axis_first(60, 16, at))).grid
    assert g.n_points == 1037 and g.MX_ELEMENTS_PER_POINT == 120
    cap, tn, runs = R.rows_tiling(g.esup_ptr)
    assert (cap, tn) == (R.CAP_LONG, 64)
    over = np.flatnonzero(runs > cap)
    assert len(over) == 1 and np.count_nonzero(runs <= cap) >= 15
    axis = R.fan_axis_nodes(16, at)
    assert np.array_equal(R.tiles_of(axis, tn), over), "the tile past the cap is the one that holds the axis block"
    n = np.diff(g.esup_ptr)
    assert np.array_equal(np.sort(n[axis]), [60, 60] + [120] * 15) and n[np.setdiff1d(np.arange(1037), axis)].max() <= 6
    # the long tile holds computed rows and skipped ones
    flag = R.fan_fields(R.fan_axis_first(60, 16, at)).point_data["neumann_flag_u"]
    tile = R.nodes_of_tiles(over, tn, 1037)
    skipped = (np.asarray(g.boundary_points)[tile] != 0) & (flag[tile] == 0)
    assert 5 <= skipped.sum() <= len(tile) - 30


def test_delaunay_small_has_tiles_of_32(oracle_lib):
    g = oracle_of(oracle_lib, M.attach_fields(R.delaunay_small(), "u", perm="LIN", neumann_plane=(2, 0.0), seed=3)).grid
    cap, tn, runs = R.rows_tiling(g.esup_ptr)
    assert (cap, tn) == (R.CAP_LONG, 32) and len(runs) >= 16
    assert not np.any(runs > cap)
    assert g.n_points >= 256, "interpolate() in pieces needs 256 nodes"


@pytest.mark.parametrize("kind,axis,long_rows", [("tet", 0, 100), ("tet", 1, 100), ("wedge", 1, 40)])
def test_flat_meshes_take_the_ls_fallback(oracle_lib, kind, axis, long_rows):
    o = oracle_of(oracle_lib, R.flat_on_axis(kind, 5, axis))
    w, _ = o.prepare("ls", "u")
    assert np.isfinite(w).all()
    n = np.diff(o.grid.esup_ptr)
    assert np.count_nonzero(R.fallback_rows(o.grid, w) & (n > 8)) >= long_rows
    assert np.all(np.asarray(o.grid.point_coords)[:, axis] == 0.0) and np.all(np.asarray(o.grid.centroids)[:, axis] == 0.0)


def test_flat_mesh_in_z_is_the_control(oracle_lib):
    o = oracle_of(oracle_lib, R.flat_on_axis("tet", 5, 2))
    w, _ = o.prepare("ls", "u")
    assert np.isfinite(w).all()
    assert not R.fallback_rows(o.grid, w).any(), "the planar branch, not the fallback"


def test_tiny_tet_has_unit_rows_in_every_chunk(oracle_lib):
    o = oracle_of(oracle_lib, R.tiny_tet())
    w, _ = o.prepare("idw", "u")
    assert np.isfinite(w).all()
    nodes, j = R.unit_rows(o.grid, w)
    assert np.count_nonzero(j >= 8) >= 10 and np.count_nonzero(j >= 16) >= 3
    assert o.grid.n_points - len(nodes) >= 30
    others = np.setdiff1d(np.arange(o.grid.n_points), nodes)
    assert np.all(np.count_nonzero(w[others], axis=1) == np.diff(o.grid.esup_ptr)[others]), "the other rows are ordinary: no zero entry"
    # with the default flags (the interior rows only) the counts of the issue that asked for this mesh
    o = oracle_of(oracle_lib, R.tiny_tet(flags_one=False))
    w, _ = o.prepare("idw", "u")
    nodes, j = R.unit_rows(o.grid, w)
    assert (len(nodes), np.count_nonzero(j >= 8), np.count_nonzero(j >= 16), np.count_nonzero(j == 0)) == (17, 13, 6, 0)
    assert np.count_nonzero(np.any(w != 0.0, axis=1)) == 64


def test_tiny_tet_of_343_nodes_has_unit_rows_in_every_piece(oracle_lib):
    """interpolate() runs in pieces from 256 nodes on (four pieces, cut at multiples of 64 nodes): the mesh of the pieces test"""
    o = oracle_of(oracle_lib, R.tiny_tet(n=6))
    w, _ = o.prepare("idw", "u")
    P = o.grid.n_points
    assert P == 343
    nodes, j = R.unit_rows(o.grid, w)
    assert np.count_nonzero(j >= 8) >= 20 and np.count_nonzero(j >= 16) >= 5 and P - len(nodes) >= 200
    cuts = [(P * k // 4) & ~63 for k in range(4)] + [P]
    assert all(np.count_nonzero((nodes >= a) & (nodes < b)) >= 3 for a, b in zip(cuts[:-1], cuts[1:]))


def test_tiny_tet_controls(oracle_lib):
    o = oracle_of(oracle_lib, R.tiny_tet(length=1.0))
    w, _ = o.prepare("idw", "u")
    assert len(R.unit_rows(o.grid, w)[0]) == 0
    o = oracle_of(oracle_lib, R.tiny_tet(length=5e-9))
    w, _ = o.prepare("idw", "u")
    assert np.all(w[:, 0] == 1.0) and np.all(w[:, 1:] == 0.0), "every computed row is e_0"


def test_apply_model_reproduces_scipy(oracle_lib):
    mesh = M.attach_fields(M.hex_mesh(4), "u", perm="LIN", neumann_plane=(2, 0.0))
    o = oracle_of(oracle_lib, mesh)
    u = np.concatenate(mesh.cell_data["u"])
    rng = np.random.default_rng(0)
    for meth in ("idw", "ls"):
        W, _ = o.interpolate("u", meth)
        for field in (u, np.sin(3.0 * u), rng.uniform(-1.0, 1.0, len(u))):
            ref, bound = R.apply_model(W.indptr, W.indices, W.data, field)
            assert ref.dtype == np.longdouble and bound.dtype == np.longdouble
            got = W.dot(field)
            fin = np.isfinite(np.asarray(ref, dtype=float))          # (LS: the nodes of the Neumann plane have NaN rows on this mesh)
            assert np.array_equal(np.isfinite(got), fin), meth
            assert np.all(np.abs(got[fin] - ref[fin]) <= bound[fin]), meth
            # the bound bites: a sum that drops its row's last entry is outside it wherever that entry is not 0
            rows = np.flatnonzero(fin & (np.diff(W.indptr) > 0))
            last = W.indptr[rows + 1] - 1
            term = W.data[last] * field[W.indices[last]]
            off = np.abs((got[rows] - term) - ref[rows]) > bound[rows]
            assert np.array_equal(off, term != 0.0) and off.sum() >= 27, meth
