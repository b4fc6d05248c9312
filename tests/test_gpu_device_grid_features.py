"""Local updates, the incremental interpolate() and apply on grids BUILT ON THE DEVICE (Interpolator(grid_build="device"),
csrc/grid_device.hip), in every state of the device-built grid's host mirror (tests/device_grid_twins.py: STATES).

Every test loads one mesh into two Interpolators, grid_build="host" and grid_build="device", drives both through the same calls with
the same inputs and compares every output by bytes; where the feature's own tests use a fresh load of the final mesh as yardstick
(tests/test_gpu_update_points_local.py, test_gpu_update_local.py, test_gpu_update_flags.py, test_gpu_hostmatrix.py) the device-built
object is compared with that fresh host-built load too.  There is no tolerance in this module: the host-built path is already held to
the oracle and the 80-bit models, and byte equality carries that over.

The meshes are the smallest the feature tests use: the composite of test_gpu_update_local.py (every non-empty kernel of the GLS launch
plan owns nodes) and quad_tri_mesh_2d(11, 8) for IDW / LS in two dimensions, with 2-column and 3-column coordinate rows.  The derivative
and gradient operations are in tests/test_gpu_device_grid_derivatives.py."""
import numpy as np
import pytest

import device_grid_twins as TW
import test_gpu_update_fields as UF
import test_gpu_update_flags as UFL
import test_gpu_update_local as UL
import test_gpu_update_points as UP
import test_gpu_update_points_local as UPL
import test_update_points_local_host as LH
import test_update_flags_host as FH
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

STATES = TW.STATES
GEOMETRY = TW.GEOMETRY
fresh_same, on_device, with_K = UF.same, UF.on_device, UF.with_K          # fresh_same: np.array_equal, NaN patterns equal
with_points, with_flags = UP.with_points, FH.with_flags
ids_on_device, stream, _buffers, _host, _torch, verts_of = UL.ids_on_device, UL.stream, UL._buffers, UL._host, UL._torch, UL.verts_of
verts_around = LH.verts_around
FULL = UL.FULL
C = UL.C          # the composite mesh of test_gpu_update_local.py: every non-empty plan kernel, with the owner kernel of every node


def _plans(I, methods):
    from ninpol_amd.interpolator import DevicePlan
    return {m: DevicePlan(I, "u", m) for m in methods}


def _full_launch(plans):
    bufs = {m: _buffers(p, FULL) for m, p in plans.items()}
    for m, p in plans.items():
        p.launch(bufs[m][0].data_ptr(), bufs[m][1].data_ptr(), stream())
    return bufs


# ---- the walk of a local-motion test and its fresh loads ------------------------------------------------------------------------------

class Walk:
    """A mesh and four stations: X0 -> XA (nodes A move) -> XB (nodes B) -> XC (nodes C) -> X0 again (everything moved goes back).  The
    fresh, host-built loads of the stations are made once and shared by every state: their grids, their interpolate() and their full
    launches are the yardsticks."""

    def __init__(self, mesh, methods, sets, amp):
        self.mesh, self.methods = mesh, methods
        X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))
        dim = 2 if np.all(X0[:, 2:] == 0.0) else 3          # (a 2-D mesh keeps z = 0 also when its rows have three columns)
        self.X = {"0": X0}
        self.nodes = dict(zip("ABC", sets))
        prev = X0
        for k in "ABC":
            X = prev.copy()
            n = self.nodes[k]
            X[n, :dim] = UPL.wobble(prev[:, :dim], amp)[n]
            assert np.abs(X[n] - prev[n]).max() > 0
            self.X[k] = prev = X
        self.nodes["0"] = np.unique(np.concatenate(sets))
        self._fresh = {}

    def fresh(self, k):
        if k not in self._fresh:
            I = TW.load(with_points(self.mesh, self.X[k]), "host")
            plans = _plans(I, self.methods)
            launch = {m: _host(b) for m, b in _full_launch(plans).items()}
            self._fresh[k] = {"I": I, "interp": {m: I.interpolate("u", m) for m in self.methods}, "launch": launch}
            g = I.grid
            self._fresh[k]["conn"] = (np.array(g.inpoel), np.array(g.esup), np.array(g.esup_ptr))
        return self._fresh[k]

    def dirty(self, *ks):
        conn = self.fresh("0")["conn"]
        return np.unique(np.concatenate([verts_around(*conn, self.nodes[k]) for k in ks]))


def drive_local_motion(walk, state, what):
    torch = _torch()
    methods = walk.methods
    H, D = TW.twins(walk.mesh)
    TW.enter(H, D, state)
    P = int(H.grid.n_points)
    # A: ids and rows on the host.  In the state pre_adoption the device-built grid takes them before it is "on the device"
    nA = walk.nodes["A"].astype(np.int64)
    for I in (H, D):
        if state == "pre_adoption":
            assert I.grid.device < 0
        I.update_points(walk.X["A"][nA], nodes=nA)
        assert np.array_equal(I.points_coords, walk.X["A"])
    if state == "pre_adoption":
        assert H.grid.device < 0 and D.grid.device < 0 and H.grid.geometry_updates == 0 and D.grid.geometry_updates == 1
    FA = walk.fresh("A")
    for m in methods:
        got = {b: I.interpolate("u", m) for b, I in (("host", H), ("device", D))}
        TW.assert_csr_same(got["device"], got["host"], (what, "A", m, "twins"))
        UP.assert_csr_same(got["device"], FA["interp"][m], (what, "A", m, "fresh"))
        assert not fresh_same(got["device"][0].data, walk.fresh("0")["interp"][m][0].data), (what, m, "the move changed nothing")
    # full results in the callers' buffers and in a HostMatrix, the dirty set cleared
    side = {}
    for b, I in (("host", H), ("device", D)):
        plans = _plans(I, methods)
        bufs = _full_launch(plans)
        Mx = plans[methods[0]].host_matrix(stream())
        I.grid.clear_dirty(stream())
        torch.cuda.synchronize()
        assert I.grid.dirty_nodes == 0
        side[b] = (plans, bufs, Mx)
    for m in methods:
        assert fresh_same(_host(side["device"][1][m])[0], FA["launch"][m][0]) and fresh_same(_host(side["device"][1][m])[1], FA["launch"][m][1])
    # B: int32 ids on the device; C: int64 ids on the device, behind B with nothing read in between (the geometry bits are cleared already)
    for I in (H, D):
        I.update_points(on_device(walk.X["B"][walk.nodes["B"]]), nodes=ids_on_device(walk.nodes["B"], np.int32))
        I.update_points(on_device(walk.X["C"][walk.nodes["C"]]), nodes=ids_on_device(walk.nodes["C"], np.int64))
    dirty = walk.dirty("B", "C")
    assert 0 < len(dirty) < P
    assert H.grid.dirty_nodes == D.grid.dirty_nodes == len(dirty), what
    FC = walk.fresh("C")
    for m in methods:
        for b in ("host", "device"):
            plans, bufs, _ = side[b]
            assert plans[m].launch_dirty(bufs[m][0].data_ptr(), bufs[m][1].data_ptr(), stream(), clear=False) == len(dirty), (what, m, b)
        (wh, nh), (wd, nd) = _host(side["host"][1][m]), _host(side["device"][1][m])
        assert wd.tobytes() == wh.tobytes() and nd.tobytes() == nh.tobytes(), (what, "launch_dirty", m, "twins")
        assert fresh_same(wd, FC["launch"][m][0]) and fresh_same(nd, FC["launch"][m][1]), (what, "launch_dirty", m, "fresh")
        assert not fresh_same(wd, FA["launch"][m][0]), (what, m, "B and C changed nothing")
        if m != "ls":          # (LS leaves NaN in degenerate rows)
            assert np.all(np.isfinite(wd)) and np.count_nonzero(wd) > 0
    # the incremental interpolate(): the dirty rows recomputed, brought over and patched into the host matrix
    for b, I in (("host", H), ("device", D)):
        Mx = side[b][2]
        assert Mx.update(stream=stream()) == len(dirty) and I.grid.dirty_nodes == 0, (what, b)
    Mh, Md = side["host"][2], side["device"][2]
    TW.assert_csr_same((Md.W, Md.neumann), (Mh.W, Mh.neumann), (what, "HostMatrix", "twins"))
    UP.assert_csr_same((Md.W, Md.neumann), FC["interp"][methods[0]], (what, "HostMatrix", "fresh"))
    # the geometry, read back lazily
    torch.cuda.synchronize()
    for k in GEOMETRY:
        assert TW.same(getattr(D.grid, k), getattr(H.grid, k)), (what, "C", k, "twins")
        assert fresh_same(getattr(D.grid, k), getattr(FC["I"].grid, k)), (what, "C", k, "fresh")
        assert not fresh_same(getattr(D.grid, k), getattr(FA["I"].grid, k)), (what, k, "B and C moved nothing")
    for I in (H, D):
        assert np.array_equal(I.points_coords, walk.X["C"])
    # 0: the geometry bits are set again by the reads above; everything that moved goes back, and the grid is the original mesh's
    n0 = walk.nodes["0"]
    for I in (H, D):
        I.update_points(on_device(walk.X["0"][n0]), nodes=ids_on_device(n0, np.int64))
    torch.cuda.synchronize()
    F0 = walk.fresh("0")
    UP.assert_grid_same(D.grid, F0["I"].grid, (what, "0", "fresh"), names=TW.ARRAYS[:-1])
    for m in methods:
        TW.assert_csr_same(D.interpolate("u", m), H.interpolate("u", m), (what, "0", m, "twins"))
        UP.assert_csr_same(D.interpolate("u", m), F0["interp"][m], (what, "0", m, "fresh"))
    assert H.grid.geometry_updates + (1 if state == "pre_adoption" else 0) == D.grid.geometry_updates
    TW.assert_lazy_arrays_same(H, D, what)


# ---- 1. local mesh motion on the composite: every kernel of the plan, every state -----------------------------------------------------

@pytest.fixture(scope="module")
def walk3(C):
    rng = np.random.default_rng(77)
    nA, dirtyA = UPL.node_set(C)          # ~2 % of the nodes, one owned by every non-empty plan kernel among them
    nB = rng.choice(C.P, size=max(C.P // 100, 2), replace=False)
    nC = rng.choice(C.P, size=max(C.P // 100, 2), replace=False)
    w = Walk(C.mesh, UF.METHODS, (nA, nB, nC), 0.002)
    assert set(C.owner[dirtyA].tolist()) == set(C.owner.tolist())
    return w


@pytest.mark.parametrize("state", STATES)
def test_local_motion_on_the_composite(walk3, state):
    drive_local_motion(walk3, state, ("composite", state))


# ---- 2. local mesh motion in two dimensions: IDW and LS, 2-column and 3-column rows ---------------------------------------------------

@pytest.fixture(scope="module", params=(2, 3), ids=("2_columns", "3_columns"))
def walk2(request):
    mesh = M.quad_tri_mesh_2d(11, 8, jitter=0.1, seed=4)
    M.attach_fields(mesh, "u", perm="LIN", neumann_plane=(0, 0.0), seed=5)
    pts = np.asarray(mesh.points, dtype=np.float64)
    P = len(pts)
    rng = np.random.default_rng(6)
    sets = [rng.choice(P, size=4, replace=False) for _ in range(3)]          # (few: B and C together must leave rows clean)
    w = Walk(mesh, ("idw", "ls"), sets, 0.004)
    # the rows every call sees have `columns` columns; the stations keep three so that the fresh loads can be cut the same way
    w.columns = request.param
    w.mesh = with_points(mesh, pts[:, :w.columns])
    w.X = {k: np.ascontiguousarray(X[:, :w.columns]) for k, X in w.X.items()}
    return w


@pytest.mark.parametrize("state", STATES)
def test_local_motion_in_two_dimensions(walk2, state):
    drive_local_motion(walk2, state, ("quad_tri_2d", walk2.columns, state))
    assert walk2.fresh("0")["I"].grid.point_coords.shape[1] == walk2.columns and int(walk2.fresh("0")["I"].grid.dim) == 2


# ---- 3. local permeability and flag updates, marks without an update -------------------------------------------------------------------

@pytest.fixture(scope="module")
def change(C):
    f1, changed, to_dir, boundary = UFL.flag_change(C)
    cells = C.cell_sets()["b"]
    K_now = C.K0.copy()
    K_now[cells] = C.K1[cells]
    mesh1 = with_flags(with_K(C.mesh, K_now), f1)
    F = TW.load(mesh1, "host")
    launch = {m: _host(b) for m, b in _full_launch(_plans(F, UF.METHODS)).items()}
    return {"f1": f1, "changed": changed, "cells": cells, "K_now": K_now, "launch": launch, "F": F}


@pytest.mark.parametrize("state", STATES[:4])
def test_local_permeability_flags_and_marks(C, change, state):
    torch = _torch()
    what = ("fields", state)
    H, D = TW.twins(C.mesh)
    TW.enter(H, D, state)
    side = {}
    for b, I in (("host", H), ("device", D)):
        plans = _plans(I, UF.METHODS)
        bufs = _full_launch(plans)
        I.grid.clear_dirty(stream())
        torch.cuda.synchronize()
        side[b] = (plans, bufs)
    w0 = {m: _host(side["device"][1][m]) for m in UF.METHODS}
    for m in UF.METHODS:
        assert w0[m][0].tobytes() == _host(side["host"][1][m])[0].tobytes(), (what, m, "before")
    # marks of the vertices of a cell: inpoel has to be on the device, and (but for lent_released) no geometry update has brought it yet
    marked = C.cell_sets()["a"]
    cells, f1, changed = change["cells"], change["f1"], change["changed"]
    order = np.random.default_rng(3).permutation(changed)
    for I in (H, D):
        I.grid.mark_dirty(cells=ids_on_device(marked, np.int32))
        assert I.grid.dirty_nodes == len(verts_of(C.inpoel, marked)), what
        I.update_permeability(on_device(C.K1[cells]), cells=ids_on_device(cells))
        I.update_neumann_flags("u", on_device(f1[order]), nodes=ids_on_device(order, np.int32))
    dirty = np.unique(np.concatenate([verts_of(C.inpoel, marked), verts_of(C.inpoel, cells), changed]))
    assert 0 < len(dirty) < C.P
    assert H.grid.dirty_nodes == D.grid.dirty_nodes == len(dirty), what
    for i, m in enumerate(UF.METHODS):
        last = i == len(UF.METHODS) - 1
        for b in ("host", "device"):
            plans, bufs = side[b]
            assert plans[m].launch_dirty(bufs[m][0].data_ptr(), bufs[m][1].data_ptr(), stream(), clear=last) == len(dirty), (what, m, b)
        (wh, nh), (wd, nd) = _host(side["host"][1][m]), _host(side["device"][1][m])
        assert wd.tobytes() == wh.tobytes() and nd.tobytes() == nh.tobytes(), (what, m, "twins")
        assert fresh_same(wd, change["launch"][m][0]) and fresh_same(nd, change["launch"][m][1]), (what, m, "fresh")
        assert not fresh_same(wd, w0[m][0]), (what, m, "the updates changed nothing")
    assert H.grid.dirty_nodes == D.grid.dirty_nodes == 0
    # the tables read back
    (ph, dh), (pd, dd) = H.grid.fetch_permeability(), D.grid.fetch_permeability()
    assert pd.tobytes() == ph.tobytes() and dd.tobytes() == dh.tobytes(), what
    assert fresh_same(pd, change["K_now"]) and not fresh_same(pd, C.K0) and fresh_same(dd, D.compute_diffusion_magnitude(change["K_now"]))
    fh, fd = H.grid.fetch_flags(), D.grid.fetch_flags()
    assert fd.tobytes() == fh.tobytes() and np.array_equal(fd != 0, UFL.bits_of(f1)), what
    assert np.array_equal(D.fetch_neumann_flags("u") != 0, UFL.bits_of(f1))
    for k in TW.ARRAYS[:-1]:
        assert fresh_same(getattr(D.grid, k), getattr(change["F"].grid, k)), (what, k, "fresh")
    TW.assert_lazy_arrays_same(H, D, what)


# ---- 4. apply, the transpose index across release_scratch(), spmv on the caller's weights ----------------------------------------------

@pytest.mark.parametrize("state", ("cold", "lent_released"))
def test_apply_and_transpose(C, state):
    torch = _torch()
    what = ("apply", state)
    H, D = TW.twins(C.mesh)
    TW.enter(H, D, state)
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-1.0, 1.0, (2, C.E)), rng.uniform(-1.0, 1.0, (2, C.P))
    got = {}
    for b, I in (("host", H), ("device", D)):
        r = {}
        for m in UF.METHODS:
            r[m, "apply"] = I.apply("u", m, values=u)
            r[m, "T"] = I.apply_transpose("u", m, v)
        assert I.grid.has_transpose_index
        I.grid.release_scratch()
        assert not I.grid.has_transpose_index
        for m in UF.METHODS:
            r[m, "T again"] = I.apply_transpose("u", m, v)          # the index is built again
            r[m, "apply again"] = I.apply("u", m, values=u)
        assert I.grid.has_transpose_index
        plan = _plans(I, ("gls",))["gls"]
        w = _full_launch({"gls": plan})["gls"]
        ud = on_device(u)
        out = torch.full((2, C.P), float("nan"), dtype=torch.float64, device="cuda")
        plan.launch_spmv(w[0].data_ptr(), ud.data_ptr(), 2, out.data_ptr(), stream())
        cells = torch.full((2, C.E), float("nan"), dtype=torch.float64, device="cuda")
        plan.launch_spmv_transpose(w[0].data_ptr(), on_device(v).data_ptr(), 2, cells.data_ptr(), stream())
        torch.cuda.synchronize()
        r["spmv"], r["spmv T"] = out.cpu().numpy(), cells.cpu().numpy()
        got[b] = r
    for key, d in got["device"].items():
        h = got["host"][key]
        for i, (a, bb) in enumerate(zip(d if isinstance(d, tuple) else (d,), h if isinstance(h, tuple) else (h,))):
            assert a.tobytes() == bb.tobytes(), (what, key)
            if key[0] != "ls":          # (LS leaves NaN in degenerate rows; neumann_ws, the second of a pair, is zero but for GLS)
                assert np.all(np.isfinite(a)) and (np.count_nonzero(a) > 0 or i == 1), (what, key)
    for m in UF.METHODS:
        assert got["device"][m, "T"].tobytes() == got["device"][m, "T again"].tobytes(), (what, m)
        assert got["device"][m, "apply"][0].tobytes() == got["device"][m, "apply again"][0].tobytes(), (what, m)
    TW.assert_lazy_arrays_same(H, D, what)


# ---- 5. the edge arrays of a device-built grid after local updates ----------------------------------------------------------------------

def test_edges_and_every_array_after_local_updates():
    torch = _torch()
    mesh = M.attach_fields(M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))
    P = len(X0)
    nodes = np.random.default_rng(4).choice(P, size=P // 5, replace=False)
    X1 = X0.copy()
    X1[nodes] = UPL.wobble(X0, 0.01)[nodes]
    H, D = TW.twins(mesh, build_edges=True)
    E = int(H.grid.n_elems)
    cells = np.arange(0, E, 7)
    K1 = UF.K_of(mesh, "LIN", 9)
    for I in (H, D):
        I.interpolate("u", "gls")
        I.update_points(on_device(X1[nodes]), nodes=ids_on_device(nodes))
        I.update_permeability(on_device(K1[cells]), cells=ids_on_device(cells, np.int32))
    torch.cuda.synchronize()
    K_now = np.ascontiguousarray(np.concatenate(mesh.cell_data["permeability"])).copy()
    K_now[cells] = K1[cells]
    F = TW.load(with_points(with_K(mesh, K_now), X1), "host", build_edges=True)
    for m in UF.METHODS:
        TW.assert_csr_same(D.interpolate("u", m), H.interpolate("u", m), ("edges", m, "twins"))
        UP.assert_csr_same(D.interpolate("u", m), F.interpolate("u", m), ("edges", m, "fresh"))
    TW.assert_lazy_arrays_same(H, D, "edges", edges=True)
    for k in TW.ARRAYS[:-1] + ("inedel", "inpoed"):
        assert fresh_same(getattr(D.grid, k), getattr(F.grid, k)), ("edges", k, "fresh")
