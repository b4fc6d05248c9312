"""Local mesh motion without a GPU: the dependency argument the device path rests on -- moving node p can move only the rows of the
vertices of the cells around p -- pinned on the oracle's own arithmetic (GLS, IDW and LS), and Interpolator.update_points(rows,
nodes=ids) on a host-only grid against a fresh load of the moved mesh, bit for bit."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import util
from ninpol_amd import mesh as M
import test_update_fields_host as UH

ROOT = UH.ROOT
lib = UH.lib
loaded = UH.loaded
PLANE = (2, 0.0)
METHODS = ("gls", "idw", "ls")
GEOMETRY = ("point_coords", "centroids", "faces_centers", "normal_faces", "faces_areas")
NEW_SYMBOLS = ("nin_grid_scatter_points_device", "nin_grid_scatter_points")

MESHES = {"hex543": lambda: M.hex_mesh(5, 4, 3, jitter=0.1, seed=1), "tet3": lambda: M.tet_mesh(3),
          "mixed533": lambda: M.mixed_mesh(5, 3, 3)}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def bits(a):
    """the float64 values as their 64-bit patterns: "did not move AT ALL" must also hold for a row the method leaves as NaN (the LS rows
    of the unjittered mixed mesh's nodes in the Neumann plane are: their cell centroids are coplanar), where `!=` is always true"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def with_points(mesh, X):
    m = copy.copy(mesh)
    m.points = np.ascontiguousarray(X)
    return m


def verts_around(inpoel, esup, esup_ptr, nodes):
    """the distinct vertices of the cells around `nodes`: the rows a move of `nodes` can reach"""
    nodes = np.unique(np.asarray(nodes, dtype=np.int64))
    cells = np.unique(np.concatenate([esup[esup_ptr[p]:esup_ptr[p + 1]] for p in nodes] + [np.zeros(0, dtype=np.int64)]))
    v = np.asarray(inpoel)[cells.astype(np.int64)].reshape(-1)
    return np.unique(v[v >= 0])


def nudge(mesh, nodes, seed, size=0.02):
    """the rows of `nodes` moved by a random offset, small against the cells (a fifth of an edge at the most)"""
    X = np.asarray(mesh.points, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(X[nodes] + rng.uniform(-size, size, (len(nodes), X.shape[1])))


# ---- 1. the locality argument, on the reference's own arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_only_the_vertices_of_the_cells_around_a_moved_node_can_move(lib, oracle_lib, name):
    """A numpy model of the dirty set -- the vertices of the cells around the moved nodes -- against the oracle's GLS, IDW and LS rows
    before and after the move, on three meshes with a Neumann plane: no row outside the set moves AT ALL (array_equal), and it is not
    vacuous: rows inside the set do move.  One interior node, one boundary node, a set of about ten."""
    mesh = M.attach_fields(MESHES[name](), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    I = loaded(mesh)
    g = I.grid
    P = int(g.n_points)
    inpoel, esup, esup_ptr = np.asarray(g.inpoel), np.asarray(g.esup), np.asarray(g.esup_ptr)
    boundary = np.asarray(g.boundary_points).astype(bool)
    X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))

    def oracle_rows(X):
        o = oracle_lib.OracleInterpolator("port", threads=2)
        o.load_mesh(with_points(mesh, X))
        out = {}
        for meth in METHODS:
            W, nws = o.interpolate("u", meth)
            out[meth] = (np.asarray(W.todense()), np.asarray(nws))
        return out

    before = oracle_rows(X0)
    assert np.count_nonzero(before["gls"][1]) > 0                       # Neumann rows are in play
    rng = np.random.default_rng(12)
    interior, on_boundary = np.flatnonzero(~boundary), np.flatnonzero(boundary)
    assert len(interior) and len(on_boundary)
    sets = {"interior": interior[[len(interior) // 2]], "boundary": on_boundary[[len(on_boundary) // 3]],
            "ten": rng.choice(P, size=min(10, P // 4), replace=False)}
    for tag, nodes in sets.items():
        X = X0.copy()
        X[nodes] = nudge(mesh, nodes, 5)
        after = oracle_rows(X)
        dirty = np.zeros(P, dtype=bool)
        dirty[verts_around(inpoel, esup, esup_ptr, nodes)] = True
        assert dirty[nodes].all() and not dirty.all(), (name, tag)
        any_moved = False
        for meth in METHODS:
            (W0, n0), (W, nws) = before[meth], after[meth]
            moved = (bits(W) != bits(W0)).any(axis=1) | (bits(nws) != bits(n0))
            assert not (moved & ~dirty).any(), \
                f"{name} {tag} {meth}: nodes {np.flatnonzero(moved & ~dirty)} moved outside the vertices of the cells around {nodes}"
            assert np.array_equal(bits(W[~dirty]), bits(W0[~dirty])) and np.array_equal(bits(nws[~dirty]), bits(n0[~dirty])), (name, tag, meth)
            any_moved |= bool((moved & dirty).any())
        assert any_moved, (name, tag)


# ---- 2. update_points(rows, nodes=ids) on a host-only grid ------------------------------------------------------------------------------
def test_the_entry_points_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/ninpol_amd.h"
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(L, name), f"{name} is not exported by the library"
    Lb = lib.load()
    assert len(Lb.nin_grid_scatter_points_device.argtypes) == 7 and len(Lb.nin_grid_scatter_points.argtypes) == 5


@pytest.mark.parametrize("name", sorted(MESHES) + ["quad_tri_2d"])
def test_host_local_move_equals_a_fresh_load(lib, name):
    if name == "quad_tri_2d":
        mesh = M.quad_tri_mesh_2d(6, jitter=0.1, seed=2)
        mesh = with_points(M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(0, 0.0), seed=2), np.asarray(mesh.points)[:, :2])
    else:
        mesh = M.attach_fields(MESHES[name](), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))
    P = len(X0)
    rng = np.random.default_rng(9)
    nodes = rng.choice(P, size=P // 4, replace=False)                      # unsorted
    rows = nudge(mesh, nodes, 6)
    X1 = X0.copy()
    X1[nodes] = rows
    F = loaded(with_points(mesh, X1))
    I = loaded(mesh)
    I.update_points(rows, nodes=nodes)
    for k in util.GRID_ARRAYS:
        assert same(getattr(I.grid, k), getattr(F.grid, k)), (name, k)
    assert np.array_equal(I.points_coords, X1) and I.points_coords.shape == X0.shape
    assert not np.array_equal(np.asarray(I.grid.centroids), np.asarray(loaded(mesh).grid.centroids))
    assert I.grid.device == -1 and I.grid.geometry_updates == 0 and I.grid.dirty_nodes == 0      # nothing went to a device
    # m = 0 is a no-op; lists, int32 ids and duplicates with equal rows give the same mesh
    I.update_points(np.zeros((0, X0.shape[1])), nodes=np.zeros(0, dtype=np.int64))
    for k in GEOMETRY:
        assert same(getattr(I.grid, k), getattr(F.grid, k)), (name, k, "m = 0")
    J = loaded(mesh)
    dup = np.concatenate([nodes, nodes[:5]]).astype(np.int32)
    J.update_points(np.concatenate([rows, rows[:5]]).tolist(), nodes=dup.tolist())
    for k in GEOMETRY:
        assert same(getattr(J.grid, k), getattr(F.grid, k)), (name, k, "duplicates")
    assert np.array_equal(J.points_coords, X1)
    # a second local move on top of the first
    more = rng.choice(P, size=3, replace=False)
    rows2 = nudge(with_points(mesh, X1), more, 7)
    X2 = X1.copy()
    X2[more] = rows2
    I.update_points(rows2, nodes=more)
    F2 = loaded(with_points(mesh, X2))
    for k in GEOMETRY:
        assert same(getattr(I.grid, k), getattr(F2.grid, k)), (name, k, "second move")
    assert np.array_equal(I.points_coords, X2)


def test_host_id_validation_and_argument_checks(lib):
    mesh = M.attach_fields(MESHES["hex543"](), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    I = loaded(mesh)
    P = int(I.grid.n_points)
    before = {k: np.array(getattr(I.grid, k)) for k in GEOMETRY}
    X0 = np.array(I.points_coords)
    rows = np.asarray(mesh.points, dtype=np.float64)[:3] + 0.01
    for bad in ([0, 1, P], [-1, 0, 1], [0, 2 ** 40, 1]):
        with pytest.raises(ValueError, match=r"nodes must lie in \[0, %d\)" % P):
            I.update_points(rows, nodes=bad)
    with pytest.raises(TypeError, match="integers"):
        I.update_points(rows, nodes=np.array([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="shape"):
        I.update_points(rows, nodes=np.zeros((3, 1), dtype=np.int64))
    for bad_rows in (np.zeros((4, 3)), np.zeros((3, 2)), np.zeros(9), np.zeros((P, 3))):
        with pytest.raises(ValueError, match="shape"):
            I.update_points(bad_rows, nodes=[0, 1, 2])
    with pytest.raises(TypeError, match="float64"):
        I.update_points(rows.astype(np.float32), nodes=[0, 1, 2])
    # as found, not as designed: an empty LIST of ids is refused (numpy makes `[]` float64); update_neumann_flags takes it
    with pytest.raises(TypeError, match="nodes must be integers, not float64"):
        I.update_points(np.zeros((0, 3)), nodes=[])
    for k in GEOMETRY:
        assert np.array_equal(getattr(I.grid, k), before[k]), ("a refused call changed the grid", k)
    assert np.array_equal(I.points_coords, X0)
    import ninpol_amd
    with pytest.raises(ValueError, match="Grid not initialized. Please load a mesh first."):
        ninpol_amd.Interpolator().update_points(rows, nodes=[0, 1, 2])


def test_error_codes_of_the_c_entry_points(lib):
    L = lib.load()
    mesh = M.attach_fields(MESHES["hex543"](), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    I = loaded(mesh)
    g = I.grid._h
    P = int(I.grid.n_points)
    before = np.array(I.grid.point_coords)
    xyz = np.zeros((2, 3))
    ids = np.zeros(2, dtype=np.int64)
    p, q = xyz.ctypes.data_as(ctypes.c_void_p), ids.ctypes.data_as(ctypes.c_void_p)

    def check(rc, code, what, text):
        assert rc == code, (what, rc)
        assert text in L.nin_last_error().decode(), (what, L.nin_last_error().decode())

    check(L.nin_grid_scatter_points_device(None, q, 1, 2, p, 3, None), lib.NIN_EINVAL, "NULL grid", "NULL")
    check(L.nin_grid_scatter_points_device(g, q, 1, 2, p, 2, None), lib.NIN_EINVAL, "coords_dim", "coords_dim")
    check(L.nin_grid_scatter_points_device(g, q, 1, 2, p, 3, None), lib.NIN_ENODEVICE, "host-only grid", "not on a device")
    check(L.nin_grid_scatter_points(None, q, 2, p, 3), lib.NIN_EINVAL, "NULL grid", "NULL")
    check(L.nin_grid_scatter_points(g, None, 2, p, 3), lib.NIN_EINVAL, "NULL ids", "NULL")
    check(L.nin_grid_scatter_points(g, q, 2, None, 3), lib.NIN_EINVAL, "NULL rows", "NULL")
    check(L.nin_grid_scatter_points(g, q, 2, p, 2), lib.NIN_EINVAL, "coords_dim", "coords_dim")
    ids[:] = (0, P)
    check(L.nin_grid_scatter_points(g, q, 2, p, 3), lib.NIN_EINVAL, "an id outside the mesh", "1 of 2 node ids")
    assert L.nin_grid_scatter_points(g, None, 0, None, 3) == lib.NIN_OK               # n == 0: a no-op
    I.grid._cache.clear()
    assert np.array_equal(I.grid.point_coords, before) and I.grid.geometry_updates == 0
