"""Local mesh motion on the device: Interpolator.update_points(rows, nodes=ids) writes the new coordinates, makes the geometry around the
moved nodes again and marks the vertices of the cells around them; DevicePlan.launch_dirty recomputes exactly the marked rows in place
(csrc/grid_scatter.hip).  The yardstick throughout is a FRESH Interpolator loaded with the moved mesh; comparisons are bit for bit
(np.array_equal, NaN patterns equal); GLS is also held to the oracle on the moved mesh within the suite's bars."""
import numpy as np
import pytest

import util
import test_gpu_update_fields as UF
import test_gpu_update_local as UL
import test_gpu_update_points as UP
import test_update_points_local_host as LH
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

METHODS, PLANE = UF.METHODS, UF.PLANE
GEOMETRY = UP.GEOMETRY
same, on_device, with_K, _loaded = UF.same, UF.on_device, UF.with_K, UF._loaded
with_points, assert_grid_same = UP.with_points, UP.assert_grid_same
ids_on_device, stream, _buffers, _host, _torch = UL.ids_on_device, UL.stream, UL._buffers, UL._host, UL._torch
verts_around = LH.verts_around
FULL, KEPT = UL.FULL, UL.KEPT
C = UL.C          # the composite mesh of test_gpu_update_local.py: every non-empty plan kernel, with the owner kernel of every node


def wobble(X, amp):
    """new positions for every node: an offset of at most `amp` per component, a function of the node's own old position only (so
    duplicate ids carry equal rows and a subset of the nodes can be moved by it)"""
    X = np.asarray(X, dtype=np.float64)
    D = np.zeros_like(X)
    D[:, 0] = np.sin(41.0 * X[:, 1] + 3.0 * X[:, 0])
    D[:, 1] = np.sin(37.0 * X[:, 0] + 1.0)
    if X.shape[1] > 2:
        D[:, 2] = np.sin(29.0 * (X[:, 0] + X[:, 1]) + 5.0 * X[:, 2])
    return np.ascontiguousarray(X + amp * D)


def assert_geometry_same(g, ref, what):
    for k in GEOMETRY:
        assert same(getattr(g, k), getattr(ref, k)), (what, k)


# ---- 3. the scatter's corners ----------------------------------------------------------------------------------------------------------
CORNERS = {"120_nodes": (lambda: M.hex_mesh(5, 4, 3), 0.02), "4913_nodes": (lambda: M.hex_mesh(16), 0.006)}
CASES = ("m0", "m1", "m63", "m64", "m65", "all_shuffled", "duplicates")


@pytest.fixture(scope="module", params=sorted(CORNERS))
def corner(request):
    make, amp = CORNERS[request.param]
    mesh = M.attach_fields(make(), "u", perm="LIN", neumann_plane=PLANE, seed=2)
    I = _loaded(mesh)
    I.interpolate("u", "idw")                                        # the grid goes to the device
    g = I.grid
    P = int(g.n_points)
    assert P == int(request.param.split("_")[0]) and g.device >= 0 and g.dirty_nodes == -1
    return {"I": I, "P": P, "mesh": mesh, "amp": amp, "X": np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64)),
            "inpoel": np.array(g.inpoel), "esup": np.array(g.esup), "esup_ptr": np.array(g.esup_ptr)}


@pytest.mark.parametrize("case", CASES)
def test_scatter_corners(corner, case):
    I, P, X = corner["I"], corner["P"], corner["X"]
    rng = np.random.default_rng(len(case) + P)
    if case == "all_shuffled":
        ids = rng.permutation(P)
    elif case == "duplicates":
        ids = np.tile(rng.choice(P, size=20, replace=False), 2)
    else:
        ids = rng.permutation(P)[:int(case[1:])]
    m = len(ids)
    for j, dt in enumerate((np.int32, np.int64)):
        rows = wobble(X, (1.0 + j) * corner["amp"])[ids]            # a row per NODE, from the mesh as it is now
        X[ids] = rows
        I.grid.clear_dirty()
        n0 = I.grid.geometry_updates
        I.update_points(on_device(rows), nodes=ids_on_device(ids, dt))
        what = (case, dt.__name__)
        assert I.grid.geometry_updates == n0 + (1 if m else 0), what
        F = _loaded(with_points(corner["mesh"], X))
        assert_geometry_same(I.grid, F.grid, what)
        assert I.grid.dirty_nodes == len(verts_around(corner["inpoel"], corner["esup"], corner["esup_ptr"], ids)) if m else \
            I.grid.dirty_nodes == 0, what
    np.testing.assert_array_equal(I.points_coords, X)                # read back from the grid on first use


# ---- 4, 5. every kernel of the plan, in place; GLS against the oracle ------------------------------------------------------------------
def node_set(c):
    """~2 % of the nodes, unsorted, with a node owned by every non-empty plan kernel among them (a moved node is a vertex of the cells
    around it, so it is dirty itself)"""
    rng = np.random.default_rng(31)
    owners = sorted(set(c.owner.tolist()))
    first = np.array([np.flatnonzero(c.owner == k)[0] for k in owners], dtype=np.int64)
    extra = rng.choice(c.P, size=max(c.P // 50, 1), replace=False)
    nodes = rng.permutation(np.unique(np.concatenate([first, extra])))
    dirty = verts_around(c.inpoel, c.esup, c.esup_ptr, nodes)
    assert set(c.owner[dirty].tolist()) == set(owners), "a plan kernel without a dirty node"
    assert len(dirty) < c.P // 2, "the set is no small part of the mesh"
    return nodes, dirty


def fresh_launch(mesh, meth, add_neumann=True):
    from ninpol_amd.interpolator import DevicePlan
    plan = DevicePlan(_loaded(mesh), "u", meth)
    b = _buffers(plan, FULL)
    plan.launch(b[0].data_ptr(), b[1].data_ptr(), stream(), add_neumann=add_neumann)
    return _host(b)


def oracle_check(oracle_lib, c, mesh, w, nws, what):
    import scipy.sparse as sp
    o = oracle_lib.OracleInterpolator("port", threads=8)
    o.load_mesh(mesh)
    Wo, nwo = o.interpolate("u", "gls")
    W = sp.csr_matrix((w, c.esup.astype(Wo.indices.dtype), c.esup_ptr.astype(Wo.indptr.dtype)), shape=(c.P, c.E))
    W.eliminate_zeros()
    err = util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data)
    el = util.csr_elementwise_err(W, Wo.indptr, Wo.indices, Wo.data)
    print(f"{what}: GLS after a local move vs oracle on the moved mesh: row-scaled {err:.3e}, element-wise {el:.3e}")
    assert err <= util.WEIGHT_RTOL
    assert el <= util.ELEMENTWISE_RTOL_GLS
    assert util.rowscaled_err(nws, nwo) <= util.WEIGHT_RTOL


@pytest.mark.parametrize("meth", METHODS)
def test_every_kernel_in_place(C, oracle_lib, meth):
    torch = _torch()
    from ninpol_amd.grid import Grid
    # the composite covers every non-empty plan kernel: each owns nodes (Ctx.owner found them kernel by kernel)
    assert set(C.owner.tolist()) == {k for k, name in enumerate(Grid.PLAN_KERNELS) if C.plan[name]} and (C.owner >= 0).all()
    I, plan, marked, clean = UL._start(C, meth, True)
    nodes, dirty = node_set(C)
    X0 = np.ascontiguousarray(np.asarray(C.mesh.points, dtype=np.float64))
    X1 = X0.copy()
    X1[nodes] = wobble(X0, 0.004)[nodes]
    I.update_points(on_device(X1[nodes]), nodes=ids_on_device(nodes))
    assert I.grid.dirty_nodes == len(dirty)
    on = np.zeros(C.P, dtype=bool)
    on[dirty] = True
    on_rows = on[C.rows]
    marked[0][torch.from_numpy(~on_rows).cuda()] = KEPT
    marked[1][torch.from_numpy(~on).cuda()] = KEPT
    n = plan.launch_dirty(marked[0].data_ptr(), marked[1].data_ptr(), stream(), clear=False)
    assert n == len(dirty) and I.grid.dirty_nodes == len(dirty)
    n = plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream(), clear=True)
    assert n == len(dirty) and I.grid.dirty_nodes == 0
    mesh1 = with_points(C.mesh, X1)
    fw, fn = fresh_launch(mesh1, meth)
    w, nws = _host(marked)
    assert same(w[on_rows], fw[on_rows]) and same(nws[on], fn[on]), "dirty rows"
    assert (w[~on_rows] == KEPT).all() and (nws[~on] == KEPT).all(), "a row outside the set was written"
    w, nws = _host(clean)
    assert same(w, fw) and same(nws, fn), "the whole buffer: a row outside the marked set depended on the moved nodes"
    assert not same(w, C.fresh(C.K0, meth, True, "K0")[0]), "the move changed nothing"
    assert_geometry_same(I.grid, _loaded(mesh1).grid, meth)
    if meth == "gls":
        oracle_check(oracle_lib, C, mesh1, w, nws, "composite")


# ---- 6. composition with a local permeability update ------------------------------------------------------------------------------------
def test_a_local_move_and_a_local_permeability_update_in_one_step(C):
    I, plan, marked, clean = UL._start(C, "gls", True)
    nodes, dirty_nodes = node_set(C)
    cells = C.cell_sets()["b"]
    X0 = np.ascontiguousarray(np.asarray(C.mesh.points, dtype=np.float64))
    X1 = X0.copy()
    X1[nodes] = wobble(X0, 0.004)[nodes]
    K_now = C.K0.copy()
    K_now[cells] = C.K1[cells]
    I.update_points(on_device(X1[nodes]), nodes=ids_on_device(nodes, np.int32))
    I.update_permeability(on_device(C.K1[cells]), cells=ids_on_device(cells))
    union = np.union1d(dirty_nodes, UL.verts_of(C.inpoel, cells))
    assert len(union) > max(len(dirty_nodes), len(UL.verts_of(C.inpoel, cells)))
    assert I.grid.dirty_nodes == len(union)
    assert plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream()) == len(union)
    assert I.grid.dirty_nodes == 0
    fw, fn = fresh_launch(with_points(with_K(C.mesh, K_now), X1), "gls")
    w, nws = _host(clean)
    assert same(w, fw) and same(nws, fn)
    # the whole-mesh form makes everything dirty
    I.update_points(on_device(X1))
    assert I.grid.dirty_nodes == -1


# ---- 7. refused ids --------------------------------------------------------------------------------------------------------------------
def test_ids_outside_the_mesh(C):
    from ninpol_amd._lib import NinpolError
    I, plan, marked, clean = UL._start(C, "gls", True)
    before = {k: np.array(getattr(I.grid, k)) for k in GEOMETRY}
    w0, n0 = _host(clean)
    ids = np.array([-1, C.P])                                        # both refused by the kernel's check: nothing is accessed through them
    rows = np.full((2, 3), 0.5)
    for dt in (np.int64, np.int32):
        I.update_points(on_device(rows), nodes=ids_on_device(ids, dt))
        assert I.grid.dirty_nodes == 0, "a refused id marked a node"
        for k in GEOMETRY:
            assert same(getattr(I.grid, k), before[k]), ("a refused id moved something", k)
        probe = _buffers(plan, KEPT)
        with pytest.raises(NinpolError, match=r"\b2 node ids outside"):
            plan.launch_dirty(probe[0].data_ptr(), probe[1].data_ptr(), stream())
        assert (_host(probe)[0] == KEPT).all() and (_host(probe)[1] == KEPT).all(), "nothing was launched"
        assert plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream()) == 0          # the call after that goes through
    assert same(_host(clean)[0], w0) and same(_host(clean)[1], n0)


# ---- 8 .. 11 on a small mesh ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    mesh = M.attach_fields(M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))
    P = len(X0)
    nodes = np.random.default_rng(4).choice(P, size=P // 5, replace=False)
    X1 = X0.copy()
    X1[nodes] = wobble(X0, 0.01)[nodes]
    g = _loaded(mesh).grid
    dirty = verts_around(np.array(g.inpoel), np.array(g.esup), np.array(g.esup_ptr), nodes)
    return {"mesh": mesh, "mesh1": with_points(mesh, X1), "X0": X0, "X1": X1, "nodes": nodes, "dirty": dirty, "P": P}


@pytest.mark.parametrize("meth", METHODS)
def test_device_pointer_path_on_a_side_stream(small, meth):
    """device tensors on a non-default stream: the full launch, the clear, the local move and the dirty launch on that stream, then
    equal to a fresh load of the moved mesh"""
    torch = _torch()
    from ninpol_amd.interpolator import DevicePlan
    fw, fn = fresh_launch(small["mesh1"], meth)
    I = _loaded(small["mesh"])
    plan = DevicePlan(I, "u", meth)
    w = torch.full((plan.nnz,), -7.0, dtype=torch.float64, device="cuda")
    nws = torch.full((plan.n_points,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ids_host, rows_host = torch.from_numpy(small["nodes"]), torch.from_numpy(small["X1"][small["nodes"]])
    with torch.cuda.stream(s):
        plan.launch(w.data_ptr(), nws.data_ptr(), s.cuda_stream)
        I.grid.clear_dirty(s.cuda_stream)
        ids, rows = ids_host.to("cuda", non_blocking=False), rows_host.to("cuda", non_blocking=False)
        I.update_points(rows, nodes=ids)
        n = plan.launch_dirty(w.data_ptr(), nws.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert n == len(small["dirty"]) and I.grid.geometry_updates == 1
    assert same(w.cpu().numpy(), fw) and same(nws.cpu().numpy(), fn), meth
    assert_geometry_same(I.grid, _loaded(small["mesh1"]).grid, "side stream")
    np.testing.assert_array_equal(I.points_coords, small["X1"])      # read back from the grid on first use
    with pytest.raises(ValueError, match="shape"):
        I.update_points(rows[:-1], nodes=ids)
    with pytest.raises(TypeError, match="float64"):
        I.update_points(rows.float(), nodes=ids)
    with pytest.raises(TypeError, match="int32 or int64"):
        I.update_points(rows, nodes=ids.to(torch.int16))
    with pytest.raises(TypeError, match="points must be"):
        I.update_points(rows.cpu().numpy(), nodes=ids)
    with pytest.raises(TypeError, match="on the host"):
        I.update_points(rows, nodes=small["nodes"])
    assert I.grid.geometry_updates == 1 and I.grid.dirty_nodes == 0            # every refusal came before any side effect


@pytest.mark.parametrize("columns", (3, 2))
def test_two_dimensional_mesh(columns):
    """2-column rows on a 2-D mesh: grid arrays, IDW and LS bit-identical to a fresh load (2-D GLS is unpinned, DESIGN section 7: not
    asserted), the dirty launch in place included"""
    torch = _torch()
    from ninpol_amd.interpolator import DevicePlan
    mesh = M.quad_tri_mesh_2d(12, jitter=0.1, seed=2)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(0, 0.0), seed=2)
    mesh = with_points(mesh, np.asarray(mesh.points)[:, :columns])
    X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))
    P = len(X0)
    nodes = np.random.default_rng(6).choice(P, size=P // 6, replace=False)
    X1 = X0.copy()
    X1[nodes, :2] = wobble(X0[:, :2], 0.008)[nodes]
    F = _loaded(with_points(mesh, X1))
    I = _loaded(mesh)
    plans = {m: DevicePlan(I, "u", m) for m in ("idw", "ls")}
    bufs = {m: _buffers(plans[m], FULL) for m in plans}
    for m in plans:
        plans[m].launch(bufs[m][0].data_ptr(), bufs[m][1].data_ptr(), stream())
    I.grid.clear_dirty(stream())
    I.update_points(on_device(X1[nodes]), nodes=ids_on_device(nodes, np.int32))
    g = I.grid
    dirty = verts_around(np.array(g.inpoel), np.array(g.esup), np.array(g.esup_ptr), nodes)
    assert g.geometry_updates == 1 and g.dirty_nodes == len(dirty)
    for m in plans:
        n = plans[m].launch_dirty(bufs[m][0].data_ptr(), bufs[m][1].data_ptr(), stream(), clear=(m == "ls"))
        assert n == len(dirty), m
        fw, fn = fresh_launch(with_points(mesh, X1), m)
        assert same(_host(bufs[m])[0], fw) and same(_host(bufs[m])[1], fn), (columns, m)
    torch.cuda.synchronize()
    assert_grid_same(I.grid, F.grid, columns)
    assert I.grid.point_coords.shape == (P, columns)
    for m in ("idw", "ls"):
        UP.assert_csr_same(I.interpolate("u", m), F.interpolate("u", m), (columns, m))


def test_numpy_arguments_on_a_grid_that_is_on_a_device(small):
    """the host form runs the same kernels: the same geometry and the same dirty set as the device form, and a patched points_coords"""
    torch = _torch()
    D, H = _loaded(small["mesh"]), _loaded(small["mesh"])
    for I in (D, H):
        I.interpolate("u", "idw")
        I.grid.clear_dirty()
        assert I.grid.device >= 0 and I.grid.dirty_nodes == 0
    nodes, rows = small["nodes"], small["X1"][small["nodes"]]
    D.update_points(on_device(rows), nodes=ids_on_device(nodes))
    pc = H.points_coords
    H.update_points(rows, nodes=nodes)
    torch.cuda.synchronize()
    assert H.points_coords is pc and np.array_equal(pc, small["X1"])               # patched in place
    assert H.grid.geometry_updates == 1 and D.grid.geometry_updates == 1
    assert H.grid.dirty_nodes == D.grid.dirty_nodes == len(small["dirty"])
    F = _loaded(small["mesh1"])
    for I in (D, H):
        assert_grid_same(I.grid, F.grid, "numpy" if I is H else "device")
    for meth in METHODS:
        UP.assert_csr_same(H.interpolate("u", meth), F.interpolate("u", meth), meth)
    # lists and int32 ids; ids are checked on the host
    H.update_points(small["X0"][nodes].tolist(), nodes=nodes.astype(np.int32).tolist())
    assert_geometry_same(H.grid, _loaded(small["mesh"]).grid, "back")
    with pytest.raises(ValueError, match=r"nodes must lie in \[0, %d\)" % small["P"]):
        H.update_points(rows[:1], nodes=[small["P"]])


def test_cell_to_node_dirty_only(small, monkeypatch):
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    monkeypatch.setenv("NIN_APPLY_NO_FUSION", "1")
    I = _loaded(small["mesh"])
    E = int(I.grid.n_elems)
    op = CellToNode(I, "u", "gls")
    I.grid.clear_dirty()                                   # op.weights is a full result as of now
    u = torch.from_numpy(np.random.default_rng(17).uniform(0.5, 1.5, E)).cuda()
    y_old = op(u)
    old_weights = op.weights
    I.update_points(on_device(small["X1"][small["nodes"]]), nodes=ids_on_device(small["nodes"]))
    assert same(op(u).cpu().numpy(), y_old.cpu().numpy())                          # nothing recomputes behind the caller's back
    op.recompute_weights(dirty_only=True)
    assert I.grid.dirty_nodes == 0 and op.weights is not old_weights
    fresh_op = CellToNode(_loaded(small["mesh1"]), "u", "gls")
    fresh_op.refresh()
    assert same(op.weights.cpu().numpy(), fresh_op.weights.cpu().numpy())
    assert same(op.neumann_ws.cpu().numpy(), fresh_op.neumann_ws.cpu().numpy())
    assert not same(op.weights.cpu().numpy(), old_weights.cpu().numpy())
    assert same(op(u).cpu().numpy(), fresh_op(u).cpu().numpy())
