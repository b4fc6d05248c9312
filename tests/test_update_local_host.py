"""Local permeability updates without a GPU: Interpolator.update_permeability(K, cells=...) with host arrays, the C entry points as far
as they go on a host-only grid, and the dependency argument the device path rests on -- a change to cell e can move only the rows of
the vertices of e -- pinned on the oracle's own arithmetic."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from ninpol_amd import mesh as M
import test_update_fields_host as UH

ROOT = UH.ROOT
NEW_SYMBOLS = ("nin_fields_scatter_permeability_device", "nin_weights_dirty_device", "nin_grid_dirty_nodes", "nin_grid_dirty_reset")
lib = UH.lib
base_mesh, new_K, with_K, loaded, rows = UH.base_mesh, UH.new_K, UH.with_K, UH.loaded, UH.rows


def test_the_entry_points_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/ninpol_amd.h"
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(L, name), f"{name} is not exported by the library"
    Lb = lib.load()
    assert len(Lb.nin_fields_scatter_permeability_device.argtypes) == 7 and len(Lb.nin_weights_dirty_device.argtypes) == 8
    assert Lb.nin_grid_dirty_nodes.restype is ctypes.c_int64


@pytest.mark.parametrize("scaled", (False, True), ids=("plain", "scaled"))
@pytest.mark.parametrize("shape", ("m33", "m9"))
def test_host_cells_update_equals_a_fresh_load(lib, shape, scaled):
    mesh = base_mesh()
    K1 = new_K(mesh)
    E = len(K1)
    rng = np.random.default_rng(8)
    cells = rng.choice(E, size=E // 4, replace=False)                       # unsorted
    m = len(cells)
    scale = rng.uniform(0.1, 10.0, m) if scaled else None
    I = loaded(mesh)
    K0 = rows(I)[0].reshape(E, 9).copy()
    I.update_permeability(K1[cells].reshape(m, 3, 3) if shape == "m33" else K1[cells], scale=scale, cells=cells)
    expected = K0.copy()
    expected[cells] = scale[:, None] * K1[cells] if scaled else K1[cells]
    F = loaded(with_K(mesh, expected))
    got, ref = rows(I), rows(F)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(ref[0], expected.reshape(-1))
    untouched = np.setdiff1d(np.arange(E), cells)
    assert np.array_equal(got[0].reshape(E, 9)[untouched], K0[untouched]) and not np.array_equal(got[0].reshape(E, 9)[cells], K0[cells])
    # bookkeeping: nothing is resident anywhere, nothing went to a device, the rows are simply the newer ones
    assert not I.permeability_on_device and I.grid.field_updates == 0 and I.grid.device == -1 and I.grid._perm_key is None
    assert I.grid.dirty_nodes == 0
    keep = [i for n, i in I.variable_to_index["cells"].items() if n not in ("permeability", "diff_mag")]
    assert np.array_equal(np.asarray(I.cells_data)[keep], np.asarray(F.cells_data)[keep])
    assert np.array_equal(I.fetch_permeability(), expected.reshape(E, 3, 3))
    # lists, int32 ids, duplicates with equal rows, no cells at all
    J = loaded(mesh)
    dup = np.concatenate([cells, cells[:5]]).astype(np.int32)
    Kd = np.concatenate([K1[cells], K1[cells[:5]]])
    J.update_permeability(Kd.tolist(), scale=None if scale is None else np.concatenate([scale, scale[:5]]), cells=dup.tolist())
    assert np.array_equal(rows(J)[0], ref[0]) and np.array_equal(rows(J)[1], ref[1])
    J.update_permeability(np.zeros((0, 9)), cells=np.zeros(0, dtype=np.int64))
    assert np.array_equal(rows(J)[0], ref[0])


def test_host_id_validation_and_argument_checks(lib):
    mesh = base_mesh()
    I = loaded(mesh)
    E = I.grid.n_elems
    before = rows(I)
    K = new_K(mesh)[:3]
    for bad in ([0, 1, E], [-1, 0, 1], [0, 2 ** 40, 1]):
        with pytest.raises(ValueError, match=r"cells must lie in \[0, %d\)" % E):
            I.update_permeability(K, cells=bad)
    with pytest.raises(TypeError, match="integers"):
        I.update_permeability(K, cells=np.array([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="shape"):
        I.update_permeability(K, cells=np.zeros((3, 1), dtype=np.int64))
    for badK in (np.zeros((4, 9)), np.zeros((3, 3)), np.zeros(27), np.zeros((E, 9))):
        with pytest.raises(ValueError, match="shape"):
            I.update_permeability(badK, cells=[0, 1, 2])
    with pytest.raises(ValueError, match="shape"):
        I.update_permeability(K, scale=np.ones(4), cells=[0, 1, 2])
    with pytest.raises(TypeError, match="float64"):
        I.update_permeability(K.astype(np.float32), cells=[0, 1, 2])
    with pytest.raises(TypeError, match="float64"):
        I.update_permeability(K, scale=np.ones(3, dtype=np.float32), cells=[0, 1, 2])
    # as found, not as designed: an empty LIST of ids is refused (numpy makes `[]` float64); update_neumann_flags takes it
    with pytest.raises(TypeError, match="cells must be integers, not float64"):
        I.update_permeability(np.zeros((0, 9)), cells=[])
    assert np.array_equal(rows(I)[0], before[0]) and np.array_equal(rows(I)[1], before[1]), "a refused call changed the table"
    import ninpol_amd
    with pytest.raises(ValueError, match="Grid not initialized. Please load a mesh first."):
        ninpol_amd.Interpolator().update_permeability(K, cells=[0, 1, 2])


def test_error_codes_of_the_c_entry_points(lib):
    L = lib.load()
    I = loaded(base_mesh())
    g = I.grid._h
    K = np.zeros((2, 9))
    ids = np.zeros(2, dtype=np.int64)
    p, q = K.ctypes.data_as(ctypes.c_void_p), ids.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int64(-5)

    def check(rc, code, what, text):
        assert rc == code, (what, rc)
        assert text in L.nin_last_error().decode(), (what, L.nin_last_error().decode())

    check(L.nin_fields_scatter_permeability_device(None, q, 1, 2, p, None, None), lib.NIN_EINVAL, "NULL grid", "NULL")
    check(L.nin_fields_scatter_permeability_device(g, q, 1, -1, p, None, None), lib.NIN_EINVAL, "negative n", "negative")
    check(L.nin_fields_scatter_permeability_device(g, q, 1, 2, p, None, None), lib.NIN_ENODEVICE, "host-only grid", "not on a device")
    check(L.nin_weights_dirty_device(None, 0, 1, p, p, None, 1, ctypes.byref(n)), lib.NIN_EINVAL, "NULL grid", "NULL")
    assert n.value == 0
    check(L.nin_weights_dirty_device(g, 0, 1, None, p, None, 1, None), lib.NIN_EINVAL, "NULL buffer", "NULL")
    check(L.nin_weights_dirty_device(g, 0, 1, p, p, None, 1, ctypes.byref(n)), lib.NIN_ENODEVICE, "host-only grid", "not on a device")
    check(L.nin_grid_dirty_reset(None, 0, None), lib.NIN_EINVAL, "NULL grid", "NULL")
    check(L.nin_grid_dirty_reset(g, 0, None), lib.NIN_ENODEVICE, "host-only grid", "not on a device")
    assert L.nin_grid_dirty_nodes(g) == 0 and L.nin_grid_dirty_nodes(None) == 0
    assert not K.any() and I.grid.field_updates == 0 and I.grid.device == -1


# ---- the dependency argument, on the reference's own arithmetic ------------------------------------------------------------------------
def test_only_the_vertices_of_a_changed_cell_can_move(lib, oracle_lib):
    """A numpy model of the dirty set -- the vertices of the changed cells -- against the oracle's GLS rows for K0 and for the patched
    K on a mixed mesh with a Neumann plane: no node outside the set moves AT ALL (array_equal), so the set is the moved nodes or a
    superset of them; and it is not vacuous: nodes inside the set do move."""
    mesh = M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2)
    M.attach_fields(mesh, "u", perm="LIN", neumann_plane=(2, 0.0), seed=3)
    I = loaded(mesh)
    E, P = int(I.grid.n_elems), int(I.grid.n_points)
    inpoel = np.asarray(I.grid.inpoel)
    K0 = rows(I)[0].reshape(E, 9).copy()
    K1 = new_K(mesh)

    def oracle_rows(K):
        o = oracle_lib.OracleInterpolator("port", threads=2)
        o.load_mesh(with_K(mesh, K))
        W, nws = o.interpolate("u", "gls")
        return np.asarray(W.todense()), np.asarray(nws)

    W0, n0 = oracle_rows(K0)
    assert np.count_nonzero(n0) > 0                                   # Neumann rows are in play
    rng = np.random.default_rng(12)
    for cells in (np.array([E // 2]), np.array([0]), rng.choice(E, size=max(E // 20, 2), replace=False)):
        K = K0.copy()
        K[cells] = K1[cells]
        W, nws = oracle_rows(K)
        v = inpoel[cells].reshape(-1)
        dirty = np.zeros(P, dtype=bool)
        dirty[np.unique(v[v >= 0])] = True
        moved = (W != W0).any(axis=1) | (nws != n0)
        assert not (moved & ~dirty).any(), f"nodes {np.flatnonzero(moved & ~dirty)} moved outside the vertices of cells {cells}"
        assert np.array_equal(W[~dirty], W0[~dirty]) and np.array_equal(nws[~dirty], n0[~dirty])
        assert (moved & dirty).any()
