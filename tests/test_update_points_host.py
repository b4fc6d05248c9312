"""Moving meshes on a host-only grid (no GPU): Interpolator.update_points / Grid.load_point_coords / nin_grid_update_points give a
loaded grid new node coordinates.  The yardstick is a FRESH Interpolator loaded with the moved mesh (which the golden fixtures and
the oracle pin) and, beside it, the oracle's own grid of the moved mesh; every comparison is bit for bit."""
import copy
import ctypes

import numpy as np
import pytest

import util
from ninpol_amd import mesh as M

CONNECTIVITY = ("esup", "esup_ptr", "psup", "psup_ptr", "fsup", "fsup_ptr", "esuf", "esuf_ptr", "esuel", "infael", "inpofa",
                "inpoel", "boundary_faces", "boundary_points")
GEOMETRY = ("point_coords", "centroids", "faces_centers", "normal_faces", "faces_areas")
KINDS = ("hex", "tet", "wedge", "mixed", "quad_tri_2d", "mixed_3d")


@pytest.fixture(scope="module")
def lib():
    from ninpol_amd import build as nbuild
    nbuild.build()
    from ninpol_amd import _lib
    return _lib


def moved(points):
    """a smooth map of the unit box: a mild shear plus small sine terms (every cell stays valid whatever its size); an in-plane
    map, so that a flat mesh stays flat and a 2-D mesh keeps z = 0"""
    X = np.asarray(points, dtype=np.float64)
    Y = X.copy()
    Y[:, 0] += 0.05 * X[:, 1] + 0.01 * np.sin(2.0 * np.pi * X[:, 1])
    Y[:, 1] += 0.03 * X[:, 0] + 0.01 * np.sin(2.0 * np.pi * X[:, 0])
    if X.shape[1] > 2:
        Y[:, 2] += X[:, 2] * (0.04 * X[:, 0] + 0.01 * np.sin(2.0 * np.pi * X[:, 1]))
    return np.ascontiguousarray(Y)


def make_mesh(kind):
    if kind == "quad_tri_2d":
        m = M.quad_tri_mesh_2d(6, jitter=0.1, seed=2)
        M.attach_fields(m, "u", perm="ALH", neumann_plane=(0, 0.0), seed=2)
        return m
    if kind == "mixed_3d":   # not squashed: normals with three live components
        m = M.mixed_mesh(6, 4, 4, jitter=0.1, seed=5)
        M.attach_fields(m, "u", perm="ALH", neumann_plane=(2, 0.0), seed=5)
        return m
    return util.flat_mesh(kind)


def with_points(mesh, X):
    m = copy.deepcopy(mesh)
    m.points = np.ascontiguousarray(X)
    return m


def loaded(mesh):
    import ninpol_amd
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    assert I.grid.device == -1
    return I


def snapshot(grid):
    return {k: np.array(getattr(grid, k)) for k in util.GRID_ARRAYS}, {k: int(getattr(grid, k)) for k in util.GRID_SCALARS}


def assert_same(a, b, names, what):
    for k in names:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (what, k)


@pytest.mark.parametrize("kind", KINDS)
def test_updated_grid_equals_a_fresh_load(lib, kind):
    mesh = make_mesh(kind)
    X1 = moved(mesh.points)
    I = loaded(mesh)
    arrays0, scalars0 = snapshot(I.grid)
    I.update_points(X1)
    arrays1, scalars1 = snapshot(I.grid)
    fresh, fresh_scalars = snapshot(loaded(with_points(mesh, X1)).grid)
    assert_same(arrays1, fresh, util.GRID_ARRAYS, kind)
    assert scalars1 == fresh_scalars == scalars0
    assert_same(arrays1, arrays0, CONNECTIVITY, kind + ": connectivity changed")
    for k in GEOMETRY:   # the map really moved something (the normals of a mesh squashed into z = 0 stay (0, 0, +-1))
        assert k == "normal_faces" and kind in ("hex", "tet", "wedge", "mixed") or not np.array_equal(arrays1[k], arrays0[k]), (kind, k)
    np.testing.assert_array_equal(I.points_coords, X1)
    assert I.grid.geometry_updates == 0   # host-only: no device copy was touched


@pytest.mark.parametrize("kind", KINDS)
def test_there_and_back_restores_every_bit(lib, kind):
    mesh = make_mesh(kind)
    I = loaded(mesh)
    arrays0, _ = snapshot(I.grid)
    I.update_points(moved(mesh.points))
    I.update_points(mesh.points)
    arrays2, _ = snapshot(I.grid)
    assert_same(arrays2, arrays0, util.GRID_ARRAYS, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_updated_geometry_equals_the_oracle_grid_of_the_moved_mesh(lib, oracle_lib, kind):
    mesh = make_mesh(kind)
    X1 = moved(mesh.points)
    I = loaded(mesh)
    I.update_points(X1)
    o = oracle_lib.OracleInterpolator("port", threads=2)
    o.load_mesh(with_points(mesh, X1))
    for k in util.GRID_SCALARS:
        assert int(getattr(I.grid, k)) == int(getattr(o.grid, k)), (kind, k)
    for k in util.GRID_ARRAYS:
        a, b = np.asarray(getattr(I.grid, k)), np.asarray(getattr(o.grid, k))
        assert a.shape == b.shape, (kind, k, a.shape, b.shape)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (kind, k)


def test_grid_load_point_coords(lib):
    """Grid.load_point_coords(coords) is the same operation; with None it stays the reference-compatible no-op"""
    mesh = make_mesh("mixed")
    X1 = moved(mesh.points)
    I = loaded(mesh)
    arrays0, _ = snapshot(I.grid)
    assert I.grid.load_point_coords(None) is None and I.grid.load_point_coords() is None
    assert I.grid.calculate_centroids() is None and I.grid.calculate_normal_faces() is None
    assert_same(snapshot(I.grid)[0], arrays0, util.GRID_ARRAYS, "no-op forms")
    assert I.grid.load_point_coords(X1.tolist()) is None     # anything numpy converts
    fresh, _ = snapshot(loaded(with_points(mesh, X1)).grid)
    assert_same(snapshot(I.grid)[0], fresh, util.GRID_ARRAYS, "load_point_coords")


def test_error_codes_of_the_c_entry_points(lib):
    L = lib.load()
    mesh = make_mesh("hex")
    I = loaded(mesh)
    g = I.grid._h
    X = np.ascontiguousarray(mesh.points, dtype=np.float64)
    p = X.ctypes.data_as(ctypes.c_void_p)
    arrays0, _ = snapshot(I.grid)

    def check(rc, code, what, text=None):
        assert rc == code, (what, rc)
        msg = L.nin_last_error().decode()
        assert msg.strip(), (what, "no error text")
        if text:
            assert text in msg, (what, msg)

    check(L.nin_grid_update_points(None, p, 3), lib.NIN_EINVAL, "NULL grid", "NULL")
    check(L.nin_grid_update_points(g, None, 3), lib.NIN_EINVAL, "NULL xyz", "NULL")
    check(L.nin_grid_update_points(g, p, 2), lib.NIN_EINVAL, "coords_dim", "coords_dim")
    check(L.nin_grid_update_points_device(None, p, 3, None), lib.NIN_EINVAL, "device: NULL grid", "NULL")
    check(L.nin_grid_update_points_device(g, None, 3, None), lib.NIN_EINVAL, "device: NULL xyz", "NULL")
    check(L.nin_grid_update_points_device(g, p, 2, None), lib.NIN_EINVAL, "device: coords_dim", "coords_dim")
    check(L.nin_grid_update_points_device(g, p, 3, None), lib.NIN_ENODEVICE, "device entry point, host-only grid", "not on a device")
    assert_same(snapshot(I.grid)[0], arrays0, util.GRID_ARRAYS, "a refused call changed the grid")
    assert L.nin_grid_update_points(g, p, 3) == lib.NIN_OK
    assert L.nin_grid_geometry_updates(g) == 0 and L.nin_grid_has_transpose_index(g) == 0
    assert L.nin_grid_geometry_updates(None) == 0 and L.nin_grid_has_transpose_index(None) == 0


def test_python_argument_checks(lib):
    import ninpol_amd
    I = ninpol_amd.Interpolator()
    with pytest.raises(ValueError, match="Grid not initialized. Please load a mesh first."):
        I.update_points(np.zeros((4, 3)))
    mesh = make_mesh("hex")
    I = loaded(mesh)
    arrays0, _ = snapshot(I.grid)
    P = I.grid.n_points
    for bad in (np.zeros((P, 2)), np.zeros((P + 1, 3)), np.zeros(3 * P), np.zeros((P, 3, 1))):
        with pytest.raises(ValueError, match="shape"):
            I.update_points(bad)
    with pytest.raises(ValueError):
        I.update_points(np.full((P, 3), "x", dtype=object))
    with pytest.raises(ValueError):
        I.update_points([[1.0, 2.0, 3.0], [1.0, 2.0]])
    assert_same(snapshot(I.grid)[0], arrays0, util.GRID_ARRAYS, "a refused call changed the grid")
    np.testing.assert_array_equal(I.points_coords, np.asarray(mesh.points, dtype=np.float64))
    I.update_points(np.asarray(mesh.points, dtype=np.float32))      # a dtype that converts
    np.testing.assert_array_equal(I.grid.point_coords, np.asarray(mesh.points, dtype=np.float32).astype(np.float64))


def test_two_column_coordinates(lib):
    """a 2-D mesh given as (P, 2): coords_dim 2 through the update, point_coords keeps the caller's width"""
    mesh = make_mesh("quad_tri_2d")
    m2 = with_points(mesh, np.asarray(mesh.points)[:, :2])
    I = loaded(m2)
    X1 = moved(m2.points)
    assert X1.shape[1] == 2
    I.update_points(X1)
    fresh, _ = snapshot(loaded(with_points(m2, X1)).grid)
    assert_same(snapshot(I.grid)[0], fresh, util.GRID_ARRAYS, "(P, 2)")
    assert I.grid.point_coords.shape == X1.shape
    with pytest.raises(ValueError, match="shape"):
        I.update_points(np.zeros((I.grid.n_points, 3)))
