"""Every kernel on RELABELLED meshes (mesh.relabel_mesh: a random renumbering of the nodes, of the cells inside each block, and a
random orientation-preserving rotation of every cell's vertex list): what a real mesher's file looks like.  The generators of
mesh.py emit one labelling, and on it every interior node of a structured mesh gets the same descriptor words (one cube-node
descriptor on a hexahedron mesh of any size: tests/test_relabel.py counts them); here every node gets its own -- which cell is
E_l, the sort of the faces by slot, the side bits, the position fields, the order of the global faces, the rows a run of 16 list
entries reads.

The yardstick is the ORACLE ON THE SAME RELABELLED MESH, at the bars of the rest of the suite (util.WEIGHT_RTOL row-scaled,
util.elementwise_rtol, 1e-14 for IDW / LS, bit equality for the grid): the reference itself is not equivariant under cell
reordering or vertex rotation (the float32 normal of a non-planar face depends on which cell and which vertices come first: up
to 7e-2 of a row's largest weight on jittered hexahedra, 2e-8 .. 7e-8 on tetrahedra, O(1) on some Neumann boundary rows), so
"relabelled and mapped back equals the original" is asked only of a NODE-ONLY renumbering, where the oracle is bit-identical
(tests/test_relabel.py) -- and there without any tolerance."""
import numpy as np
import pytest

import test_gpu_composite as TC
import test_gpu_parity as TP
import test_gpu_update_points as TU
import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

TIGHT = 1e-14
METHODS = ("gls", "idw", "ls")
ONE_WAVE = ("mfw_large", "mfw_small", "mfw_general", "mfx", "hex8")
# node classes that follow from the cell graph around a node alone (the others depend on a greedy front set or a row count
# taken in esup order, and may trade nodes with each other under a relabelling)
TOPOLOGICAL = ("hex8", "quad4", "mfw_large", "mfw_small", "mfx_boundary")


def _interp(**kw):
    import ninpol_amd
    return ninpol_amd.Interpolator(**kw)


def _loaded(mesh, **kw):
    I = _interp(**kw)
    I.load_mesh(mesh_obj=mesh)
    return I


def _tol(meth):
    return util.WEIGHT_RTOL if meth == "gls" else TIGHT


def _oracle(oracle_lib, mesh, threads=16):
    o = oracle_lib.OracleInterpolator("port", threads=threads)
    o.load_mesh(mesh)
    return o


def _assert_grid_is_oracles(I, o):
    for k in util.GRID_SCALARS:
        assert getattr(I.grid, k) == getattr(o.grid, k), k
    for k in util.GRID_ARRAYS:
        np.testing.assert_array_equal(getattr(I.grid, k), getattr(o.grid, k), err_msg=k)


# ---- a. per family ----------------------------------------------------------------------------------------------------------

_FAMILIES = {m[0]: m[1:] for m in TP._meshes()}      # the meshes of test_gpu_matches_oracle: mesh, perm, Neumann plane
_cache = {}


def _family(oracle_lib, name):
    """the family's mesh with its fields, relabelled (all three switches), and the oracle's tables on the relabelled mesh"""
    if name not in _cache:
        mesh, perm, plane = _FAMILIES[name]
        M.attach_fields(mesh, "u", perm=perm, neumann_plane=plane, seed=7)
        r = M.relabel_mesh(mesh, seed=1000 + sorted(_FAMILIES).index(name))
        o = _oracle(oracle_lib, r)
        _cache[name] = (mesh, r, o, {meth: o.prepare(meth, "u") for meth in METHODS}, {meth: o.interpolate("u", meth)[0] for meth in METHODS})
    return _cache[name]


@pytest.mark.parametrize("grid_build", ["host", "device"])
@pytest.mark.parametrize("name", list(_FAMILIES))
def test_gpu_relabelled_family_matches_oracle(oracle_lib, name, grid_build):
    """test_gpu_matches_oracle's meshes (same generator arguments, permeability, Neumann plane), relabelled: grid bit-equal, the
    dense tables and interpolate()'s CSR (pattern exact) of all three methods, row-scaled and element by element; grid built
    on the host and on the device."""
    mesh, r, o, dense, csr = _family(oracle_lib, name)
    perm = _FAMILIES[name][1]
    I = _loaded(r, grid_build=grid_build)
    _assert_grid_is_oracles(I, o)
    for meth in METHODS:
        wo, no = dense[meth]
        w, nw = I.prepare_interpolator(meth, "u", np.arange(I.grid.n_points))
        Wo = csr[meth]
        W, _ = I.interpolate("u", meth)
        rs = max(util.rowscaled_err(w, wo), util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data))
        ew = max(util.elementwise_err(w, wo), util.csr_elementwise_err(W, Wo.indptr, Wo.indices, Wo.data))
        print(f"relabelled {name} {meth} ({grid_build} grid): row-scaled {rs:.2e}, element-wise (floor {util.ELEMENTWISE_FLOOR:g}) {ew:.2e}")
        assert rs <= _tol(meth), (meth, rs)
        assert util.rowscaled_err(nw, no) <= _tol(meth), meth
        assert ew <= util.elementwise_rtol(meth, perm), (meth, ew)
    assert np.any(dense["gls"][0] != 0)


# ---- d. the plan under relabelling --------------------------------------------------------------------------------------------

def _plans(mesh, seed):
    r = M.relabel_mesh(mesh, seed=seed)
    out = []
    for m in (mesh, r):
        I = _loaded(m)
        I.grid.to_device(0)
        out.append(I.grid.gls_plan())
    n_interior = int(np.sum(np.asarray(I.grid.boundary_points) == 0))
    return out[0], out[1], n_interior


def _print_plans(name, a, b):
    show = lambda p: {k: v for k, v in p.items() if v}
    print(f"plan {name}: generator order {show(a)}")
    print(f"plan {name}: relabelled      {show(b)}")


@pytest.mark.parametrize("name", list(_FAMILIES))
def test_gpu_plan_classes_that_are_topology_survive_relabelling(name):
    """Cube nodes, the quad nodes of a boundary face, the two-coloured nodes (large and small) and the wide kernel's boundary
    nodes are classes of the cell graph around a node: the same counts on the relabelled mesh, and the same total.  (The size
    classes of a greedy front set or of a row count may trade nodes with each other; both plans are printed.)"""
    mesh, perm, plane = _FAMILIES[name]
    M.attach_fields(mesh, "u", perm=perm, neumann_plane=plane, seed=7)
    a, b, _ = _plans(mesh, seed=2000 + sorted(_FAMILIES).index(name))
    _print_plans(name, a, b)
    for k in TOPOLOGICAL:
        assert a[k] == b[k], (k, a[k], b[k])
    assert sum(a.values()) == sum(b.values()) == mesh.points.shape[0]


@pytest.mark.parametrize("lattice", ["bcc", "random"])
def test_gpu_one_wavefront_share_survives_relabelling(lattice):
    """The mesh of test_gpu_wide_multifrontal_kernel_on_unstructured_tetrahedra, relabelled: the share of interior nodes on a
    one-wavefront multifrontal kernel stays above that test's bars (0.95 body-centred cloud, 0.85 random cloud) -- the greedy
    front sets, taken in esup order, must not depend on a friendly numbering."""
    mesh = M.delaunay_tet_mesh(11, seed=21, lattice=lattice)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(1, 0.0), seed=2)
    a, b, n_interior = _plans(mesh, seed=31)
    _print_plans(f"delaunay11 {lattice}", a, b)
    share = lambda p: sum(p[k] for k in ONE_WAVE) / n_interior
    print(f"delaunay11 {lattice}: one-wavefront share of {n_interior} interior nodes {share(a):.4f} generator order, {share(b):.4f} relabelled")
    for k in TOPOLOGICAL:
        assert a[k] == b[k], (k, a[k], b[k])
    assert share(b) >= (0.95 if lattice == "bcc" else 0.85), (b, n_interior)


# ---- c. every route ---------------------------------------------------------------------------------------------------------

_ROUTE_MESHES = {"hex": lambda: M.hex_mesh(9, jitter=0.15, seed=5), "tet": lambda: M.tet_mesh(5, jitter=0.1, seed=3),
                 "wedge": lambda: M.wedge_mesh(5, jitter=0.05, seed=3), "mixed": lambda: M.mixed_mesh(8, 4, 4, jitter=0.1, seed=3)}


@pytest.mark.parametrize("kind", sorted(_ROUTE_MESHES))
def test_gpu_every_gls_route_on_relabelled_mesh(oracle_lib, monkeypatch, kind):
    """test_gpu_parity._GLS_ROUTES forced in turn on a relabelled mesh with a Neumann plane: each against the oracle, and the
    plan says the forced kernel ran (the assertions of test_gpu_gls_degenerate_zero_pivot_column on the plans)."""
    mesh = _ROUTE_MESHES[kind]()
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(2, 0.0), seed=4)
    r = M.relabel_mesh(mesh, seed=77)
    o = _oracle(oracle_lib, r, threads=8)
    wo, no = o.prepare("gls", "u")
    plans = {}
    for route, switches in TP._GLS_ROUTES.items():
        with monkeypatch.context() as mp:
            for sw in switches:
                mp.setenv(sw, "1")
            I = _loaded(r)
            I.grid.to_device(0)
            plans[route] = I.grid.gls_plan()
            w, nw = I.prepare_interpolator("gls", "u", np.arange(I.grid.n_points))
        rs = util.rowscaled_err(w, wo)
        print(f"relabelled {kind} route {route}: row-scaled {rs:.2e}")
        assert rs <= util.WEIGHT_RTOL, (route, rs)
        assert util.rowscaled_err(nw, no) <= util.WEIGHT_RTOL, route
    d = plans["default"]
    assert (d["hex8"] > 0) == (kind in ("hex", "mixed"))
    assert (d["mfw_large"] > 0) == (kind in ("tet", "mixed")) and (d["mfw_small"] > 0) == (kind == "wedge")
    assert (d["mfx"] > 0) == (kind == "mixed") and d["mfw_general"] == 0
    assert (plans["general_kind"]["mfw_general"] > 0) == (kind == "mixed") and plans["general_kind"]["mfx"] == 0
    assert plans["no_cube_kernel"]["hex8"] == 0 and plans["no_cube_kernel"]["mfw_small"] >= d["hex8"]
    assert plans["no_general_kind"]["mfw_general"] == 0 and plans["no_general_kind"]["mfx"] == 0
    assert plans["wide_for_two_coloured"]["mfx"] >= d["mfw_large"] + d["mfx"]
    assert plans["wide_for_two_coloured"]["mfw_large"] == 0 and plans["wide_for_two_coloured"]["mfw_small"] == 0
    assert plans["no_boundary_in_wide"]["mfx_boundary"] == 0
    small = ("small4", "small8", "small12")
    assert sum(d[k] for k in small) > 0 and all(plans["no_small_kernel"][k] == 0 for k in small)
    assert (d["quad4"] > 0 or kind == "tet") and plans["no_quad_kernel"]["quad4"] == 0
    assert sum(plans["no_quad_kernel"][k] for k in small) == sum(d[k] for k in small) + d["quad4"]
    for route in ("block_only", "global_scratch"):
        assert all(plans[route][k] == 0 for k in ("hex8", "mfw_large", "mfw_small", "mfw_general", "mfx", "mfx_boundary", "quad4") + small), route
    assert plans["global_scratch"]["scratch"] > 0
    assert all(sum(p.values()) == I.grid.n_points for p in plans.values())


# ---- e. node-only relabelling: no tolerance -----------------------------------------------------------------------------------

_NODE_ONLY = [("hex20_jitter_neu", ()), ("hex20_jitter_neu", ("NIN_GLS_NO_GROUP",)), ("mixed1266", ()),
              ("delaunay8_random_cloud_fan", ()), ("delaunay_prisms12_random_fan", ())]


@pytest.mark.parametrize("name,switches", _NODE_ONLY, ids=[n + ("_" + "_".join(s) if s else "") for n, s in _NODE_ONLY])
def test_gpu_node_only_relabelling_is_bit_identical(monkeypatch, name, switches):
    """Renumbering the nodes alone leaves every node's cells, faces and their order as they were (the oracle is bit-identical
    there: tests/test_relabel.py), and a node's arithmetic does not depend on its neighbours in the list (abi_plan.hip): the LS and
    GLS tables and neumann_ws of the node-relabelled mesh, rows mapped back, equal those of the original bit for bit -- through
    the cube-node kernel and, with it switched off, the one-wavefront kernel; the mixed mesh; the random cloud (wide kernel,
    tiles in global memory) and unstructured prisms.  IDW to its bar (1e-14).  The launch plan is the same key by key."""
    for sw in switches:
        monkeypatch.setenv(sw, "1")
    mesh, perm, plane = _FAMILIES[name]
    M.attach_fields(mesh, "u", perm=perm, neumann_plane=plane, seed=7)
    r = M.relabel_mesh(mesh, seed=5, cells=False, rotate=False)
    new = r.new_node_of_old
    A, B = _loaded(mesh), _loaded(r)
    for meth in METHODS:
        wa, na = A.prepare_interpolator(meth, "u", np.arange(A.grid.n_points))
        wb, nb = B.prepare_interpolator(meth, "u", np.arange(B.grid.n_points))
        assert np.any(np.nan_to_num(wa) != 0)
        if meth == "idw":
            assert util.rowscaled_err(wb[new], wa) <= TIGHT
        else:
            diff = np.flatnonzero(~np.all((wb[new] == wa) | (np.isnan(wa) & np.isnan(wb[new])), axis=1))
            assert len(diff) == 0, (meth, len(diff), diff[:10], np.diff(np.asarray(A.grid.esup_ptr))[diff[:10]])
        assert np.array_equal(nb[new], na, equal_nan=True), meth
    pa, pb = dict(A.grid.gls_plan()), dict(B.grid.gls_plan())
    assert pa == pb, (pa, pb)
    if name.startswith("hex"):
        assert (pa["hex8"] == 0) == bool(switches) and pa["hex8"] + pa["mfw_small"] == 19 ** 3


# ---- f. the cube-node pipeline on scattered ids -------------------------------------------------------------------------------

def test_gpu_cube_pipeline_on_scattered_ids(oracle_lib, monkeypatch):
    """The mesh of test_gpu_cube_kernel_forms (more groups than resident waves, a ragged last group, a list long enough for
    locality_order), relabelled: a run of 16 list entries now reads rows from all over every table, every node has its own
    descriptor words.  Weights against the oracle; the list in node order, in the default order and in Morton order bit-identical;
    with and without the side stream bit-identical; the fused apply against the oracle's W . u."""
    mesh = M.hex_mesh(41, 37, 29, jitter=0.15, seed=6)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(1, 0.0), seed=3)
    r = M.relabel_mesh(mesh, seed=8)
    o = _oracle(oracle_lib, r)
    wo, no = o.prepare("gls", "u")
    Wo, _ = o.interpolate("u", "gls")
    u = np.concatenate(r.cell_data["u"])
    fields = np.stack([u, np.sin(3.0 * u)])
    got = {}
    for mode, side in (("off", True), (None, True), ("m", True), (None, False)):
        with monkeypatch.context() as mp:
            if mode:
                mp.setenv("NIN_GLS_LOCALITY_ORDER", mode)
            if not side:
                mp.setenv("NIN_GLS_NO_SIDE_STREAM", "1")
            I = _loaded(r)
            w, nw = I.prepare_interpolator("gls", "u", np.arange(I.grid.n_points))
            assert I.grid.gls_plan()["hex8"] == 40 * 36 * 28
            W, neu = I.interpolate("u", "gls")
            many, nws = I.apply("u", "gls", values=fields)
        got[mode, side] = (w, nw, W.indptr.copy(), W.indices.copy(), W.data.copy(), neu, many, nws)
        if (mode, side) == (None, True):
            assert util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data) <= util.WEIGHT_RTOL
    w, nw = got[None, True][:2]
    rs, ew = util.rowscaled_err(w, wo), util.elementwise_err(w, wo)
    print(f"relabelled hex 41x37x29, cube-node kernel: row-scaled {rs:.2e}, element-wise {ew:.2e}")
    assert rs <= util.WEIGHT_RTOL and ew <= util.elementwise_rtol("gls")
    assert util.rowscaled_err(nw, no) <= util.WEIGHT_RTOL
    interior = np.asarray(I.grid.boundary_points) == 0
    assert np.count_nonzero(w[interior]) > 8 * int(interior.sum()) - 10
    for key, res in got.items():
        for a, b in zip(got[None, True], res):
            assert np.array_equal(a, b), key
    many = got[None, True][6]
    for k in range(2):
        ref = Wo.dot(fields[k])
        assert np.abs(many[k] - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), k
    rng = np.random.default_rng(0)
    sub = rng.permutation(I.grid.n_points)[:1237].astype(np.int64)
    ws, nws = I.prepare_interpolator("gls", "u", sub)
    assert np.array_equal(ws, w[sub]) and np.array_equal(nws, nw[sub])


# ---- b. every kernel in one launch --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def H(oracle_lib):
    """the hybrid mesh of tests/test_gpu_composite.py built from RELABELLED parts, then relabelled once more as a whole (the
    parts' node ids interleave at random, their cells inside every block too)"""
    parts = TC._parts()
    for i, p in enumerate(parts):
        M.attach_fields(p, "u", perm="ALH", neumann_plane=(2, 0.0), seed=20 + i)
    parts = [M.relabel_mesh(p, seed=300 + i) for i, p in enumerate(parts)]
    mesh = M.relabel_mesh(M.composite_mesh(parts), seed=400)
    o = _oracle(oracle_lib, mesh)
    I = _loaded(mesh)
    return {"mesh": mesh, "P": mesh.points.shape[0], "oracle": {meth: o.prepare(meth, "u") for meth in METHODS},
            "oracle_csr": {meth: o.interpolate("u", meth)[0] for meth in METHODS}, "o": o, "I": I,
            "full": {meth: I.prepare_interpolator(meth, "u", np.arange(mesh.points.shape[0])) for meth in METHODS},
            "plan": I.grid.gls_plan()}


def test_hybrid_plan_still_holds_every_kernel(H):
    plan = H["plan"]
    print(f"plan relabelled hybrid: {dict((k, v) for k, v in plan.items() if v)}")
    for k in ("hex8", "quad4", "mfg_tiles", "scratch", "mfx_boundary"):
        assert plan[k] > 0, (k, plan)
    for fam in ("mfw_", "small", "block", "mfx_"):
        assert any(v > 0 for k, v in plan.items() if k.startswith(fam)), (fam, plan)
    assert sum(plan.values()) == H["P"]
    _assert_grid_is_oracles(H["I"], H["o"])


@pytest.mark.parametrize("meth", METHODS)
def test_hybrid_full_launch(H, meth):
    w, nw = H["full"][meth]
    wo, no = H["oracle"][meth]
    rs, ew = util.rowscaled_err(w, wo), util.elementwise_err(w, wo)
    print(f"relabelled hybrid {meth}: row-scaled {rs:.2e}, element-wise {ew:.2e}")
    assert rs <= _tol(meth) and ew <= util.elementwise_rtol(meth)
    assert util.rowscaled_err(nw, no) <= _tol(meth)


def test_hybrid_shuffled_target_list_hits_every_class(H):
    """A shuffled target list with nodes of every kernel of the plan (each kernel launched alone through NIN_GLS_ONLY tells
    which rows are its own): the full launch's rows bit for bit, and the oracle's within the bar."""
    I, plan = H["I"], H["plan"]
    rows, _ = TC._layout(I.grid)
    dp = I.device_plan("u", "gls")
    rng = np.random.default_rng(6)
    picks = []
    with pytest.MonkeyPatch.context() as mp:
        for k, name in enumerate(I.grid.PLAN_KERNELS):
            if not plan[name]:
                continue
            mp.setenv("NIN_GLS_ONLY", str(k))
            a, n = TC._host(TC._torch_launch(dp, np.nan))
            mine = np.flatnonzero(~np.isnan(n))
            assert len(mine) == plan[name], (name, len(mine), plan[name])
            picks.append(rng.choice(mine, min(48, len(mine)), replace=False))
    targets = rng.permutation(np.unique(np.concatenate(picks + [np.arange(2, H["P"], 11)]))).astype(np.int64)
    w, nw = H["full"]["gls"]
    wo, no = H["oracle"]["gls"]
    for _ in range(2):
        ws, nws = I.prepare_interpolator("gls", "u", targets)
        assert np.array_equal(ws, w[targets]) and np.array_equal(nws, nw[targets])
        assert util.rowscaled_err(ws, wo[targets]) <= util.WEIGHT_RTOL and util.rowscaled_err(nws, no[targets]) <= util.WEIGHT_RTOL


@pytest.mark.parametrize("meth", METHODS)
def test_hybrid_interpolate_in_pieces_equals_one_piece(H, meth):
    res = {}
    for mode in ("pieces", "one"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(*(("NIN_E2E_MIN_NODES", "0") if mode == "pieces" else ("NIN_E2E_NO_PIPELINE", "1")))
            I = _loaded(H["mesh"])
            W, nws = I.interpolate("u", meth)
        Wo = H["oracle_csr"][meth]
        assert util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data) <= _tol(meth), (mode, meth)
        assert util.csr_elementwise_err(W, Wo.indptr, Wo.indices, Wo.data) <= util.elementwise_rtol(meth), (mode, meth)
        assert util.rowscaled_err(nws, H["oracle"][meth][1]) <= _tol(meth), (mode, meth)
        res[mode] = (W.indptr.copy(), W.indices.copy(), W.data.copy(), np.array(nws))
    for a, b in zip(res["pieces"], res["one"]):
        assert np.array_equal(a, b, equal_nan=True), meth


def test_hybrid_apply_fused_and_unfused(H):
    Wo, nwo = H["oracle_csr"]["gls"], H["oracle"]["gls"][1]
    u = np.concatenate(H["mesh"].cell_data["u"])
    rng = np.random.default_rng(5)
    fields = np.stack([u, np.cos(2.0 * u), rng.uniform(-1.0, 1.0, len(u))])
    got = {}
    for fused in (True, False):
        with pytest.MonkeyPatch.context() as mp:
            if not fused:
                mp.setenv("NIN_APPLY_NO_FUSION", "1")
            I = _loaded(H["mesh"])
            vals, nws = I.apply("u", "gls")
            many, nws3 = I.apply("u", "gls", values=fields)
        assert util.rowscaled_err(nws, nwo) <= util.WEIGHT_RTOL
        np.testing.assert_array_equal(nws3, nws)
        np.testing.assert_array_equal(many[0], vals)
        for k in range(3):
            ref = Wo.dot(fields[k])
            assert np.abs(many[k] - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (fused, k)
        got[fused] = (many, nws)
    assert np.abs(got[True][0] - got[False][0]).max() <= 1e-13 * np.abs(got[False][0]).max()
    np.testing.assert_array_equal(got[True][1], got[False][1])


@pytest.mark.parametrize("meth", METHODS)
def test_hybrid_apply_transpose_against_scipy(H, meth):
    """apply_transpose(v) against scipy's W.T @ v of interpolate()'s W, with the bound of tests/test_gpu_transpose.py: the
    cell-major transpose index is built from a cell order and a node order that are random here."""
    import test_gpu_transpose as TT
    I = H["I"]
    W, _ = I.interpolate("u", meth)
    v = np.random.default_rng(11).uniform(-1.0, 1.0, H["P"])
    x = I.apply_transpose("u", meth, v)
    assert x.shape == (W.shape[1],) and x.dtype == np.float64
    ref = W.T @ v
    _, bad_cols, A = TT._finite(W)
    np.testing.assert_array_equal(x[bad_cols], ref[bad_cols])
    good = ~bad_cols
    bound = A.T @ np.abs(v)
    off = np.flatnonzero(good)[~(np.abs(x[good] - ref[good]) <= 1e-13 * bound[good])]
    assert len(off) == 0, (meth, off[:10], x[off[:10]], ref[off[:10]])
    assert np.count_nonzero(x[good]) > 0.9 * W.shape[1], meth


@pytest.mark.parametrize("grid_build", ("host", "device"))
def test_hybrid_update_points_equals_a_fresh_load(H, grid_build):
    """update_points() on the relabelled hybrid (points moved as in tests/test_gpu_update_points.py), after everything is
    resident: grid arrays, all three methods' CSR, apply and apply_transpose equal a fresh load_mesh() of the moved mesh bit for
    bit."""
    X1 = TU.moved(H["mesh"].points)
    F = _loaded(TU.with_points(H["mesh"], X1))
    I = _loaded(H["mesh"], grid_build=grid_build)
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-1.0, 1.0, int(F.grid.n_elems)), rng.uniform(-1.0, 1.0, H["P"])
    for meth in METHODS:
        I.interpolate("u", meth)
    I.apply_transpose("u", "idw", v)
    plan = dict(I.grid.gls_plan())
    I.update_points(X1)
    assert I.grid.geometry_updates == 1
    TU.assert_grid_same(I.grid, F.grid, grid_build)
    for meth in METHODS:
        TU.assert_csr_same(I.interpolate("u", meth), F.interpolate("u", meth), (grid_build, meth))
        got, ref = I.apply("u", meth, values=u), F.apply("u", meth, values=u)
        assert TU.same(got[0], ref[0]) and TU.same(got[1], ref[1]), meth
        assert TU.same(I.apply_transpose("u", meth, v), F.apply_transpose("u", meth, v)), meth
    assert dict(I.grid.gls_plan()) == plan == dict(F.grid.gls_plan())
    assert not TU.same(H["full"]["gls"][0], I.prepare_interpolator("gls", "u", np.arange(H["P"]))[0])
