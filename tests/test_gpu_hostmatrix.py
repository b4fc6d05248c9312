"""A host matrix kept current: DevicePlan.host_matrix() and HostMatrix.update() (csrc/csr_dirty.hip, csrc/csr_patch.cpp).  After local
updates of K, of the points or of the Neumann flags only the dirty rows are recomputed, packed, transferred and patched into the scipy
matrix.  The yardstick throughout is a FRESH Interpolator loaded with a mesh that carries the new K, points or flags, and its
interpolate(); every comparison is bit for bit (np.array_equal) on indptr, indices, data and neumann."""
import numpy as np
import pytest

import test_gpu_update_fields as UF
import test_gpu_update_local as UL
import test_gpu_update_points_local as PL
import test_update_flags_host as FH
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

PLANE = UF.PLANE
same, on_device, with_K, _loaded, K_of = UF.same, UF.on_device, UF.with_K, UF._loaded, UF.K_of
ids_on_device, verts_of = UL.ids_on_device, UL.verts_of
with_points, with_flags = PL.with_points, FH.with_flags
C = UL.C          # the composite mesh of test_gpu_update_local.py: every non-empty plan kernel
SENTINEL = -7.0


def arrays_of(Mx):
    return Mx.W.indptr, Mx.W.indices, Mx.W.data, Mx.neumann


def assert_current(Mx, mesh, meth, what):
    """M is what interpolate() of a fresh load_mesh() of `mesh` returns"""
    W, nws = _loaded(mesh).interpolate("u", meth)
    assert Mx.W.shape == W.shape, what
    for name, a, b in zip(("indptr", "indices", "data", "neumann"), arrays_of(Mx), (W.indptr, W.indices, W.data, nws)):
        assert same(a, b), (what, name)


def identity_of(Mx):
    return [Mx.W] + list(arrays_of(Mx)), [a.ctypes.data for a in arrays_of(Mx)]


def assert_same_objects(Mx, ident, what):
    objs, addrs = ident
    now, now_addrs = identity_of(Mx)
    assert all(a is b for a, b in zip(now, objs)) and now_addrs == addrs, (what, "M.W was replaced although no row's count changed")


def poison_rows(Mx, rows):
    """the host entries of `rows` overwritten: an update that does not bring them all back fails the comparison"""
    indptr = Mx.W.indptr
    for p in rows:
        Mx.W.data[indptr[p]:indptr[p + 1]] = SENTINEL
        Mx.W.indices[indptr[p]:indptr[p + 1]] = -1
        Mx.neumann[p] = SENTINEL


# ---- 1. the corners of the pack kernels -----------------------------------------------------------------------------------------------
CORNERS = {"hex_120_nodes": lambda: M.hex_mesh(5, 4, 3), "fan_153_nodes": lambda: M.wedge_fan(50, 2)}   # the fan's axis node: a 100-entry row


def cells_with_n_vertices(inpoel, n, seed):
    """a connected set of cells whose distinct vertices are exactly n (grown cell by cell, started again when it overshoots)"""
    vs = [set(int(v) for v in row if v >= 0) for row in np.asarray(inpoel)]
    for attempt in range(500):
        rng = np.random.default_rng(seed + attempt)
        chosen, verts = [], set()
        while len(verts) < n:
            fits = [c for c in range(len(vs)) if c not in chosen and (not chosen or vs[c] & verts) and len(verts | vs[c]) <= n]
            if not fits:
                break
            c = int(rng.choice(fits))
            chosen.append(c)
            verts |= vs[c]
        if len(verts) == n:
            return np.array(chosen, dtype=np.int64)
    raise AssertionError(f"no set of cells with exactly {n} vertices found")


@pytest.mark.parametrize("meth", ("idw", "ls"))
@pytest.mark.parametrize("name", sorted(CORNERS))
def test_pack_kernel_corners(name, meth):
    """Dirty sets of 0, 63, 64, 65 and all nodes from update_permeability(cells=) with device ids (and once with numpy ids), and of one
    node -- no set of cells has a single vertex -- from update_neumann_flags(nodes=) on an interior node, whose flag no weight reads.
    IDW and LS do not read K either, so the dirty rows of the host arrays are overwritten first: update() has to bring every one back."""
    mesh = M.attach_fields(CORNERS[name](), "u", perm="LIN", neumann_plane=PLANE, seed=2)
    I = _loaded(mesh)
    plan = I.device_plan("u", meth)
    Mx = plan.host_matrix()
    P, E = int(I.grid.n_points), int(I.grid.n_elems)
    assert P == int(name.split("_")[1]) and I.grid.dirty_nodes == 0
    assert int(np.diff(np.array(I.grid.esup_ptr)).max()) == (100 if name.startswith("fan") else 8)
    assert_current(Mx, mesh, meth, "host_matrix()")
    inpoel = np.array(I.grid.inpoel)
    K_now, K1 = K_of(mesh, "LIN", 2), K_of(mesh, "ALH", 7)
    rng = np.random.default_rng(5)
    cases = [("numpy_ids", cells_with_n_vertices(inpoel, 64, 1)), (0, np.zeros(0, np.int64))]
    cases += [(n, cells_with_n_vertices(inpoel, n, 10 * n)) for n in (63, 64, 65)] + [(P, rng.permutation(E))]
    for j, (n_nodes, cells) in enumerate(cases):
        rows = (1.0 + j) * K1[cells]
        K_now[cells] = rows
        dirty = verts_of(inpoel, cells) if len(cells) else np.zeros(0, np.int64)
        if n_nodes == "numpy_ids":
            I.update_permeability(rows, cells=cells)
        else:
            assert len(dirty) == n_nodes
            I.update_permeability(on_device(rows), cells=ids_on_device(cells, np.int32 if j % 2 else np.int64))
        assert I.grid.dirty_nodes == len(dirty)
        poison_rows(Mx, dirty)
        ident = identity_of(Mx)
        assert Mx.update() == len(dirty), n_nodes
        assert Mx.structure_changed is False, n_nodes
        assert_same_objects(Mx, ident, n_nodes)
        assert_current(Mx, with_K(mesh, K_now), meth, n_nodes)
        assert I.grid.dirty_nodes == 0
    # one node
    interior = np.flatnonzero(np.array(I.grid.boundary_points) == 0)
    p = int(interior[np.argmax(np.diff(np.array(I.grid.esup_ptr))[interior])])       # (on the fan: the axis node with its 100-entry row)
    flags = FH.row(I, "u").copy()
    assert flags[p] == 0.0
    flags[p] = 1.0
    I.update_neumann_flags("u", on_device(np.array([1.0])), nodes=ids_on_device(np.array([p])))
    assert I.grid.dirty_nodes == 1
    poison_rows(Mx, [p])
    ident = identity_of(Mx)
    assert Mx.update() == 1 and Mx.structure_changed is False
    assert_same_objects(Mx, ident, "one node")
    assert_current(Mx, with_flags(with_K(mesh, K_now), flags), meth, "one node")
    Mx.release()


# ---- 2. every plan kernel ---------------------------------------------------------------------------------------------------------------
def test_every_plan_kernel(C):
    I = _loaded(C.mesh)
    plan = I.device_plan("u", "gls")
    Mx = plan.host_matrix()
    assert I.grid.dirty_nodes == 0
    assert_current(Mx, C.mesh, "gls", "host_matrix()")
    cells = C.cell_sets()["b"]
    nodes, _ = PL.node_set(C)
    X0 = np.ascontiguousarray(np.asarray(C.mesh.points, dtype=np.float64))
    K_now, X_now = C.K0.copy(), X0.copy()
    half = len(cells) // 2
    steps = {"K": (cells[:half], None), "points": (None, nodes[: len(nodes) // 2]), "both": (cells[half:], nodes[len(nodes) // 2:])}
    for what, (cs, ns) in steps.items():
        if cs is not None:
            K_now[cs] = C.K1[cs]
            I.update_permeability(on_device(C.K1[cs]), cells=ids_on_device(cs))
        if ns is not None:
            X_now[ns] = PL.wobble(X0, 0.004)[ns]
            I.update_points(on_device(X_now[ns]), nodes=ids_on_device(ns, np.int32))
        expected = I.grid.dirty_nodes
        assert 0 < expected < C.P, what
        on = np.zeros(C.P, dtype=bool)
        if cs is not None:
            on[verts_of(C.inpoel, cs)] = True
        if ns is not None:
            on[PL.verts_around(C.inpoel, C.esup, C.esup_ptr, ns)] = True
        assert int(on.sum()) == expected, what
        # a row outside the set is not touched: a sentinel in one clean row's data survives
        indptr = Mx.W.indptr
        clean = int(np.flatnonzero(~on & (np.diff(indptr) > 0))[3])
        kept = Mx.W.data[indptr[clean]]
        Mx.W.data[indptr[clean]] = SENTINEL
        assert Mx.update() == expected, what
        assert Mx.W.data[Mx.W.indptr[clean]] == SENTINEL, (what, "a row outside the dirty set was written")
        Mx.W.data[Mx.W.indptr[clean]] = kept
        now = with_points(with_K(C.mesh, K_now), X_now)
        assert_current(Mx, now, "gls", what)
        before = [a.copy() for a in arrays_of(Mx)]
        ident = identity_of(Mx)
        assert Mx.update() == 0 and Mx.structure_changed is False, (what, "a second update")
        assert_same_objects(Mx, ident, what)
        assert all(same(a, b) for a, b in zip(arrays_of(Mx), before)), (what, "a second update changed something")
    assert not same(K_now, C.K0) and not same(X_now, X0)
    Mx.release()


# ---- 3 .. 6 on one small mesh -------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def small():
    mesh = M.attach_fields(M.hex_mesh(6), "u", perm="LIN", neumann_plane=PLANE, seed=2)
    I = _loaded(mesh)
    plan = I.device_plan("u", "gls")
    Mx = plan.host_matrix()
    assert I.grid.dirty_nodes == 0
    yield {"mesh": mesh, "I": I, "plan": plan, "M": Mx, "K0": K_of(mesh, "LIN", 2), "K1": K_of(mesh, "ALH", 7), "E": int(I.grid.n_elems),
           "P": int(I.grid.n_points), "inpoel": np.array(I.grid.inpoel)}
    Mx.release()


def test_structure_change(small):
    mesh, I, Mx = small["mesh"], small["I"], small["M"]
    X = np.asarray(mesh.points)
    inside = (X[:, 0] > 0.1) & (X[:, 0] < 0.9) & (X[:, 1] > 0.1) & (X[:, 1] < 0.9)      # nodes inside a face: four cells each
    bottom, top = np.flatnonzero(inside & (X[:, 2] == 0.0)), np.flatnonzero(inside & (X[:, 2] == 1.0))
    flags = FH.row(I, "u").copy()
    assert (flags[bottom] == 1.0).all() and (flags[top] == 0.0).all()
    ids = np.concatenate([bottom[:7], top[:3]])                # seven Neumann nodes become Dirichlet, three boundary nodes Neumann
    values = np.concatenate([np.zeros(7), np.ones(3)])
    flags[ids] = values
    old = identity_of(Mx)
    nnz0 = int(Mx.W.indptr[-1])
    I.update_neumann_flags("u", on_device(values), nodes=ids_on_device(ids))
    assert Mx.update() == len(ids)
    assert Mx.structure_changed is True
    assert all(a is not b for a, b in zip(identity_of(Mx)[0][:4], old[0][:4])) and Mx.neumann is old[0][4]
    assert_current(Mx, with_flags(mesh, flags), "gls", "flags")
    assert int(Mx.W.indptr[-1]) != nnz0 and (np.diff(Mx.W.indptr)[bottom[:7]] == 0).all() and (np.diff(Mx.W.indptr)[top[:3]] > 0).all()
    # K alone on the new structure: in place again
    cells = np.random.default_rng(3).choice(small["E"], size=20, replace=False)
    K_now = small["K0"].copy()
    K_now[cells] = small["K1"][cells]
    I.update_permeability(on_device(small["K1"][cells]), cells=ids_on_device(cells))
    ident = identity_of(Mx)
    assert Mx.update() == len(verts_of(small["inpoel"], cells))
    assert Mx.structure_changed is False
    assert_same_objects(Mx, ident, "K on the new structure")
    assert_current(Mx, with_flags(with_K(mesh, K_now), flags), "gls", "K on the new structure")


def test_full_fallbacks(small):
    mesh, I, plan, Mx, P = small["mesh"], small["I"], small["plan"], small["M"], small["P"]
    assert_current(Mx, mesh, "gls", "host_matrix()")
    I.update_permeability(on_device(small["K1"]))                       # the whole table from the device: every node is dirty
    assert I.grid.dirty_nodes == -1
    assert Mx.update() == P and I.grid.dirty_nodes == 0
    assert_current(Mx, with_K(mesh, small["K1"]), "gls", "whole-array update")
    K2 = 2.0 * small["K1"]
    I.update_permeability(K2)                                           # the host rows edited; refresh() finds them and uploads
    plan.refresh()
    assert I.grid.dirty_nodes == -1
    assert Mx.update() == P and I.grid.dirty_nodes == 0
    assert_current(Mx, with_K(mesh, K2), "gls", "refresh()")
    held = Mx.W
    Mx.release()
    assert Mx.update() == P and I.grid.dirty_nodes == 0
    assert Mx.W is not held
    assert_current(Mx, with_K(mesh, K2), "gls", "release()")
    cells = np.arange(5)                                                # ... and it goes on in place afterwards
    K2[cells] = small["K0"][cells]
    I.update_permeability(on_device(small["K0"][cells]), cells=ids_on_device(cells))
    assert Mx.update() == len(verts_of(small["inpoel"], cells)) and Mx.structure_changed is False
    assert_current(Mx, with_K(mesh, K2), "gls", "after release()")


def test_refused_ids(small):
    from ninpol_amd._lib import NinpolError
    mesh, I, Mx, E = small["mesh"], small["I"], small["M"], small["E"]
    good = np.array([3, 40, 41, 100])
    ids = np.concatenate([good, [E]])                                   # one cell id out of range
    K_now = small["K0"].copy()
    K_now[good] = small["K1"][good]
    I.update_permeability(on_device(np.concatenate([small["K1"][good], np.full((1, 9), 5.0)])), cells=ids_on_device(ids))
    before = [a.copy() for a in arrays_of(Mx)]
    ident = identity_of(Mx)
    n_dirty = I.grid.dirty_nodes
    with pytest.raises(NinpolError, match=r"\b1 cell ids outside"):
        Mx.update()
    assert_same_objects(Mx, ident, "refused ids")
    assert all(same(a, b) for a, b in zip(arrays_of(Mx), before)) and I.grid.dirty_nodes == n_dirty
    more = np.array([7, 150])
    K_now[more] = small["K1"][more]
    I.update_permeability(on_device(small["K1"][more]), cells=ids_on_device(more))
    assert Mx.update() == len(verts_of(small["inpoel"], np.concatenate([good, more])))
    assert_current(Mx, with_K(mesh, K_now), "gls", "after the refusal")


def test_isolation_from_interpolate(small):
    mesh, I, Mx = small["mesh"], small["I"], small["M"]
    K_now = small["K0"].copy()
    for step, cells in enumerate((np.array([1, 2, 60]), np.array([100, 101, 215]))):
        K_now[cells] = small["K1"][cells]
        I.update_permeability(on_device(small["K1"][cells]), cells=ids_on_device(cells))
        assert Mx.update() == len(verts_of(small["inpoel"], cells)), step
        assert_current(Mx, with_K(mesh, K_now), "gls", step)
        if step == 0:
            W, _ = I.interpolate("u", "idw")                            # the grid's call scratch is overwritten; M's buffers are its own
            assert W.nnz > 0
