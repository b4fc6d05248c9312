"""Changing Neumann flags without a GPU: Interpolator.update_neumann_flags with host arrays, the C entry points of the device path as far
as they go on a host-only grid, and the dependency argument the device path rests on -- the flag of node n is read by row n only --
pinned on the oracle's own arithmetic.  The yardstick is a FRESH Interpolator loaded with a mesh that carries the new flags; every
comparison is bit for bit."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from ninpol_amd import mesh as M
import test_update_fields_host as UH

ROOT = UH.ROOT
NEW_SYMBOLS = ("nin_fields_set_flags_device", "nin_fields_scatter_flags_device", "nin_fields_get_flags", "nin_grid_flag_updates")
lib = UH.lib
base_mesh, loaded = UH.base_mesh, UH.loaded
# what the truncation rule has to sort: (long long)x != 0
VALUES = np.array([0.0, 1.0, 2.0, -1.0, 0.5, -0.5, 1e-300, 255.0, 4294967296.0])
IS_SET = np.array([0, 1, 1, 1, 0, 0, 0, 1, 1], dtype=bool)


def with_flags(mesh, flags, variable="u"):
    """the same mesh (same K, same Neumann values) carrying `flags` as neumann_flag_<variable>"""
    m = copy.deepcopy(mesh)
    m.point_data["neumann_flag_" + variable] = np.array(flags, dtype=np.float64)
    return m


def row(I, variable="u"):
    return np.array(I.points_data[I.variable_to_index["points"]["neumann_flag_" + variable]][:I.grid.n_points])


def test_the_truncation_rule_of_the_value_set():
    assert np.array_equal(VALUES.astype(np.int64) != 0, IS_SET)


def test_the_entry_points_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/ninpol_amd.h"
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(L, name), f"{name} is not exported by the library"
    Lb = lib.load()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert list(Lb.nin_fields_set_flags_device.argtypes) == [vp, vp, i32, vp]
    assert list(Lb.nin_fields_scatter_flags_device.argtypes) == [vp, vp, i32, i64, vp, i32, vp]
    assert list(Lb.nin_fields_get_flags.argtypes) == [vp, vp]
    assert list(Lb.nin_grid_flag_updates.argtypes) == [vp]
    assert Lb.nin_grid_flag_updates.restype is i64
    for name in NEW_SYMBOLS[:3]:
        assert getattr(Lb, name).restype is i32                                # ctypes' default: the int error code


def test_error_codes_of_the_c_entry_points(lib):
    L = lib.load()
    I = loaded(base_mesh())
    g = I.grid._h
    P = I.grid.n_points
    f = np.zeros(P)
    ids = np.zeros(2, dtype=np.int64)
    out = np.full(P, 7, dtype=np.uint8)
    p, q, o = (a.ctypes.data_as(ctypes.c_void_p) for a in (f, ids, out))
    before = row(I)

    def check(rc, code, what, text):
        assert rc == code, (what, rc)
        assert text in L.nin_last_error().decode(), (what, L.nin_last_error().decode())

    check(L.nin_fields_set_flags_device(None, p, 0, None), lib.NIN_EINVAL, "set: NULL grid", "NULL")
    check(L.nin_fields_set_flags_device(g, None, 0, None), lib.NIN_EINVAL, "set: NULL flags", "NULL")
    check(L.nin_fields_set_flags_device(g, p, 0, None), lib.NIN_ENODEVICE, "set: host-only grid", "not on a device")
    check(L.nin_fields_set_flags_device(g, p, 1, None), lib.NIN_ENODEVICE, "set: host-only grid, bytes", "not on a device")
    check(L.nin_fields_scatter_flags_device(None, q, 1, 2, p, 0, None), lib.NIN_EINVAL, "scatter: NULL grid", "NULL")
    check(L.nin_fields_scatter_flags_device(g, q, 1, -1, p, 0, None), lib.NIN_EINVAL, "scatter: negative n", "negative")
    check(L.nin_fields_scatter_flags_device(g, q, 1, 2, p, 0, None), lib.NIN_ENODEVICE, "scatter: host-only grid", "not on a device")
    check(L.nin_fields_scatter_flags_device(g, None, 1, 2, p, 0, None), lib.NIN_ENODEVICE, "scatter: host-only grid, NULL ids", "not on a device")
    check(L.nin_fields_get_flags(None, o), lib.NIN_EINVAL, "get: NULL grid", "NULL")
    check(L.nin_fields_get_flags(g, None), lib.NIN_EINVAL, "get: NULL output", "NULL")
    check(L.nin_fields_get_flags(g, o), lib.NIN_ENODEVICE, "get: host-only grid", "not on a device")
    assert L.nin_grid_flag_updates(g) == 0 and L.nin_grid_flag_updates(None) == 0
    assert (out == 7).all() and not f.any()                                 # a refused call wrote nothing
    assert np.array_equal(row(I), before) and I.grid.flag_updates == 0 and I.grid.device == -1
    assert I.grid.fetch_flags() is None and I.grid.dirty_nodes == 0


def test_host_whole_array_equals_a_fresh_load(lib):
    mesh = base_mesh()
    I = loaded(mesh)
    P = I.grid.n_points
    rng = np.random.default_rng(21)
    flags = VALUES[rng.integers(0, len(VALUES), P)]
    flags[:len(VALUES)] = VALUES                                              # every value at least once
    before = np.array(I.points_data)
    I.update_neumann_flags("u", flags)
    F = loaded(with_flags(mesh, flags))
    assert np.array_equal(row(I), row(F)) and np.array_equal(row(F), flags) and not np.array_equal(row(I), before[I.variable_to_index["points"]["neumann_flag_u"]][:P])
    # every other row of the table, and all of cells_data, is untouched
    keep = [i for n, i in I.variable_to_index["points"].items() if n != "neumann_flag_u"]
    assert np.array_equal(np.asarray(I.points_data)[keep], before[keep]) and np.array_equal(np.asarray(I.cells_data), np.asarray(F.cells_data))
    # bookkeeping: nothing is resident anywhere, nothing went to a device
    assert not I.neumann_flags_on_device and I.grid.flag_updates == 0 and I.grid.device == -1 and I.grid.dirty_nodes == 0
    assert np.array_equal(I.fetch_neumann_flags("u"), flags)                  # nothing resident: the row as it is
    assert np.array_equal(row(I), flags)
    # bool, integers and lists are taken as they convert
    on = IS_SET[rng.integers(0, len(IS_SET), P)]
    for form in (on, on.astype(np.uint8), on.astype(np.int64), on.tolist(), on.astype(np.float64).tolist()):
        J = loaded(mesh)
        J.update_neumann_flags("u", form)
        assert np.array_equal(row(J), on.astype(np.float64))


def test_host_nodes_update_equals_a_fresh_load(lib):
    mesh = base_mesh()
    I = loaded(mesh)
    P = I.grid.n_points
    rng = np.random.default_rng(22)
    nodes = rng.choice(P, size=P // 3, replace=False)                         # unsorted
    vals = VALUES[rng.integers(0, len(VALUES), len(nodes))]
    vals[:len(VALUES)] = VALUES
    f0 = row(I)
    expected = f0.copy()
    expected[nodes] = vals
    I.update_neumann_flags("u", vals, nodes=nodes)
    F = loaded(with_flags(mesh, expected))
    assert np.array_equal(row(I), row(F)) and np.array_equal(row(I), expected)
    untouched = np.setdiff1d(np.arange(P), nodes)
    assert np.array_equal(row(I)[untouched], f0[untouched]) and not np.array_equal(row(I)[nodes], f0[nodes])
    assert not I.neumann_flags_on_device and I.grid.flag_updates == 0 and I.grid.device == -1 and I.grid.dirty_nodes == 0
    # lists, int32 ids, duplicates with equal values, no nodes at all
    J = loaded(mesh)
    dup = np.concatenate([nodes, nodes[:5]]).astype(np.int32)
    J.update_neumann_flags("u", np.concatenate([vals, vals[:5]]).tolist(), nodes=dup.tolist())
    assert np.array_equal(row(J), expected)
    J.update_neumann_flags("u", np.concatenate([vals, vals[:5]]), nodes=dup)
    assert np.array_equal(row(J), expected)
    J.update_neumann_flags("u", np.zeros(0), nodes=np.zeros(0, dtype=np.int64))
    J.update_neumann_flags("u", [], nodes=[])
    assert np.array_equal(row(J), expected)


def test_cpu_torch_tensors_are_host_arrays(lib):
    torch = pytest.importorskip("torch")
    mesh = base_mesh()
    I, J = loaded(mesh), loaded(mesh)
    P = I.grid.n_points
    flags = VALUES[np.random.default_rng(23).integers(0, len(VALUES), P)]
    I.update_neumann_flags("u", torch.from_numpy(flags))
    J.update_neumann_flags("u", flags)
    assert np.array_equal(row(I), row(J))
    I.update_neumann_flags("u", torch.tensor([True, False]), nodes=torch.tensor([3, 4]))
    J.update_neumann_flags("u", [1.0, 0.0], nodes=[3, 4])
    assert np.array_equal(row(I), row(J))


def test_validation_errors_leave_the_row_unchanged(lib):
    import ninpol_amd
    with pytest.raises(ValueError, match="Grid not initialized. Please load a mesh first."):
        ninpol_amd.Interpolator().update_neumann_flags("u", np.zeros(3))
    with pytest.raises(ValueError, match="Grid not initialized. Please load a mesh first."):
        ninpol_amd.Interpolator().fetch_neumann_flags("u")
    assert not ninpol_amd.Interpolator().neumann_flags_on_device
    I = loaded(base_mesh())
    P = I.grid.n_points
    before = np.array(I.points_data)
    ok = np.ones(3)
    for variable in ("w", "permeability", ""):
        with pytest.raises(ValueError, match="not found in points data"):
            I.update_neumann_flags(variable, np.zeros(P))
        with pytest.raises(ValueError, match="not found in points data"):
            I.fetch_neumann_flags(variable)
    for bad in ([0, 1, P], [-1, 0, 1], [0, 2 ** 40, 1]):
        with pytest.raises(ValueError, match=r"nodes must lie in \[0, %d\)" % P):
            I.update_neumann_flags("u", ok, nodes=bad)
    with pytest.raises(TypeError, match="integers"):
        I.update_neumann_flags("u", ok, nodes=np.array([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="shape"):
        I.update_neumann_flags("u", ok, nodes=np.zeros((3, 1), dtype=np.int64))
    for bad in (np.zeros(4), np.zeros((3, 1)), np.zeros(P)):
        with pytest.raises(ValueError, match="shape"):
            I.update_neumann_flags("u", bad, nodes=[0, 1, 2])
    for bad in (np.zeros(P + 1), np.zeros(P - 1), np.zeros((P, 1)), np.zeros(0)):
        with pytest.raises(ValueError, match="shape"):
            I.update_neumann_flags("u", bad)
    for bad in (np.zeros(P, dtype=np.float32), np.zeros(P, dtype=np.float16), np.zeros(P, dtype=complex), np.array(["a"] * P)):
        with pytest.raises(TypeError, match="float64"):
            I.update_neumann_flags("u", bad)
    with pytest.raises(TypeError, match="float64"):
        I.update_neumann_flags("u", ok.astype(np.float32), nodes=[0, 1, 2])
    with pytest.raises(ValueError):
        I.update_neumann_flags("u", [[1.0, 2.0], [1.0]])
    # as found, not as designed: an empty LIST of ids (numpy makes `[]` float64) is taken here and changes nothing; update_points and
    # update_permeability refuse it with a TypeError
    assert I.update_neumann_flags("u", [], nodes=[]) is None
    assert np.array_equal(np.asarray(I.points_data), before), "a refused call changed the table"


# ---- the dependency argument, on the reference's own arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize("meth", ("gls", "idw", "ls"))
def test_a_flag_moves_its_own_row_only(lib, oracle_lib, meth):
    """The marking rule -- exactly the nodes whose Neumann bit changed -- against the oracle's rows before and after six random flags
    are flipped, three times over, on a mixed mesh with a Neumann plane: no row outside the flipped nodes moves AT ALL (array_equal), so
    the set is the moved rows or a superset of them; and it is not vacuous: rows inside it do move.  (If this ever failed, the rule
    would have to widen to what the oracle shows.)"""
    mesh = M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2)
    M.attach_fields(mesh, "u", perm="LIN", neumann_plane=(2, 0.0), seed=3)
    f0 = np.array(mesh.point_data["neumann_flag_u"])
    P = len(f0)
    assert P == 89

    def oracle_rows(flags):
        o = oracle_lib.OracleInterpolator("port", threads=2)
        o.load_mesh(with_flags(mesh, flags))
        W, nws = o.interpolate("u", meth)
        return np.asarray(W.todense()), np.asarray(nws)

    W0, n0 = oracle_rows(f0)
    if meth == "gls":
        assert np.count_nonzero(n0) > 0                               # Neumann rows are in play
    rng = np.random.default_rng(14)
    for _ in range(3):
        nodes = rng.choice(P, size=6, replace=False)
        f1 = f0.copy()
        f1[nodes] = 1.0 - f1[nodes]
        W, nws = oracle_rows(f1)
        dirty = np.zeros(P, dtype=bool)
        dirty[nodes] = True
        moved = (W != W0).any(axis=1) | (nws != n0)
        assert not (moved & ~dirty).any(), f"{meth}: nodes {np.flatnonzero(moved & ~dirty)} moved, flipped were {nodes}"
        assert np.array_equal(W[~dirty], W0[~dirty]) and np.array_equal(nws[~dirty], n0[~dirty])
        assert (moved & dirty).any()
