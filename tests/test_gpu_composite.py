"""Every GLS kernel of the launch plan in ONE launch: a hybrid mesh (mesh.composite_mesh) whose parts are the single-family
meshes the rest of the suite tests one at a time.  In one launch the kernels share the grid's block of work counters and the
side stream; each route below (the full launch with and without the side stream, target lists, interpolate() in pieces and in
one piece, the fused and the unfused apply, DevicePlan launches, each kernel alone through NIN_GLS_ONLY, the device-built grid)
is held to the oracle on the union and, through the part maps, to each part computed alone on the GPU."""
import os

import numpy as np
import pytest

import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

TIGHT = 1e-14
METHODS = ("gls", "idw", "ls")


def _parts():
    return [M.hex_mesh(16, jitter=0.1, seed=1), M.delaunay_tet_mesh(10, seed=4, lattice="random"), M.delaunay_tet_mesh(8, seed=2),
            M.tet_mesh(6, jitter=0.1, seed=3), M.wedge_mesh(6, 5, 4, jitter=0.05, seed=5), M.mixed_mesh(10, 5, 5, jitter=0.1, seed=6),
            M.delaunay_wedge_mesh(12, 6, seed=7, lattice="random"), M.wedge_fan(30, 3), M.wedge_fan(50, 2)]


def _interp(**kw):
    import ninpol_amd
    return ninpol_amd.Interpolator(**kw)


def _loaded(mesh, **kw):
    I = _interp(**kw)
    I.load_mesh(mesh_obj=mesh)
    return I


_layout = util.esup_layout


def _dense(grid, csr):
    """weights in CSR position (esup layout, nnz_esup) -> the dense (n_points, MX_ELEMENTS_PER_POINT) table"""
    rows, local = _layout(grid)
    w = np.zeros((int(grid.n_points), int(grid.MX_ELEMENTS_PER_POINT)))
    w[rows, local] = csr
    return w


def _weights(I, meth, targets=()):
    """nin_weights_host: weights in CSR position for ALL nodes (0 outside `targets`) and neumann_ws, no Neumann term added"""
    from ninpol_amd.interpolator import _run_weights
    return _run_weights(I.grid, meth, I.cells_data, I.points_data, I.variable_to_index, "u", np.asarray(targets, dtype=np.int64), False)


def _tol(meth):
    return util.WEIGHT_RTOL if meth == "gls" else TIGHT


def _check(C, I, meth, w, nw, what):
    """a full dense table of the union against the oracle, and each part's rows against that part alone on the GPU"""
    wo, nwo = C["oracle"][meth]
    assert util.rowscaled_err(w, wo) <= _tol(meth), (what, meth)
    assert util.elementwise_err(w, wo) <= util.elementwise_rtol(meth), (what, meth)
    assert util.rowscaled_err(nw, nwo) <= _tol(meth), (what, meth)
    W = util.esup_csr(I.grid, w)
    for i, (pg, res) in enumerate(C["alone"]):
        wp, nwp = res[meth]
        mine = util.part_table(W, pg, C["mesh"].part_nodes[i], C["mesh"].part_cells[i])
        assert util.rowscaled_err(mine, wp) <= _tol(meth), (what, meth, i)
        assert util.elementwise_err(mine, wp) <= util.elementwise_rtol(meth), (what, meth, i)
        assert util.rowscaled_err(nw[C["mesh"].part_nodes[i]], nwp) <= _tol(meth), (what, meth, i)


@pytest.fixture(scope="module")
def C(oracle_lib):
    parts = _parts()
    for i, p in enumerate(parts):
        M.attach_fields(p, "u", perm="ALH", neumann_plane=(2, 0.0), seed=20 + i)
    mesh = M.composite_mesh(parts)
    o = oracle_lib.OracleInterpolator("port", threads=8)
    o.load_mesh(mesh)
    oracle = {meth: o.prepare(meth, "u") for meth in METHODS}
    oracle_csr = {meth: o.interpolate("u", meth)[0] for meth in METHODS}
    alone = []
    for p in parts:
        J = _loaded(p)
        res = {meth: J.prepare_interpolator(meth, "u", np.arange(J.grid.n_points)) for meth in METHODS}
        alone.append((J.grid, res))
    I = _loaded(mesh)
    full = {meth: _weights(I, meth) for meth in METHODS}
    return {"parts": parts, "mesh": mesh, "P": mesh.points.shape[0], "oracle": oracle, "oracle_csr": oracle_csr, "alone": alone,
            "I": I, "full": full, "plan": I.grid.gls_plan(), "part_plans": [g.gls_plan() for g, _ in alone]}


_torch_launch, _host = util.torch_launch, util.torch_to_host


@pytest.fixture(scope="module")
def owners(C):
    """NIN_GLS_ONLY=<k>: the rows each kernel of the plan writes (launched alone into NaN-filled buffers)"""
    csr, nws = C["full"]["gls"]
    assert not np.isnan(csr).any() and not np.isnan(nws).any()   # (a NaN in the owners' buffers means: not written)
    return util.gls_kernel_owners(C["I"], C["plan"])


def test_plan_holds_every_kernel_and_is_the_sum_of_the_parts(C):
    """The plan the routes below rely on (so that they cannot go vacuous): at least 8 cube-node workgroups in every quarter of
    interpolate()'s pipeline -- they take one work counter per XCD -- next to the tiles-in-global-memory kernel, the global-scratch
    class and a member of every family; and node classes are local: the union's plan is the sum of the parts' plans."""
    plan = C["plan"]
    assert plan["hex8"] >= 4 * 512, plan
    for k in ("mfg_tiles", "scratch", "quad4", "mfx_boundary"):
        assert plan[k] > 0, (k, plan)
    for fam in ("mfw_", "small", "block", "mfx_"):
        assert any(v > 0 for k, v in plan.items() if k.startswith(fam)), (fam, plan)
    assert sum(plan.values()) == C["P"]
    total = {k: sum(pp[k] for pp in C["part_plans"]) for k in plan}
    assert dict(plan) == total, (dict(plan), total)


@pytest.mark.parametrize("meth", METHODS)
def test_full_launch(C, meth):
    """Route 1: prepare_interpolator over every node (the side stream on, the default)."""
    w, nw = C["I"].prepare_interpolator(meth, "u", np.arange(C["P"]))
    _check(C, C["I"], meth, w, nw, "full launch")
    np.testing.assert_array_equal(w, _dense(C["I"].grid, C["full"][meth][0]))


def test_full_launch_without_side_stream(C, monkeypatch):
    """Route 2: the same with the global-scratch class and the tiles-in-global-memory kernel on the main stream, after the
    cube-node kernel; the rows are those of the default launch, bit for bit."""
    monkeypatch.setenv("NIN_GLS_NO_SIDE_STREAM", "1")
    csr, nws = _weights(C["I"], "gls")
    _check(C, C["I"], "gls", _dense(C["I"].grid, csr), nws, "no side stream")
    np.testing.assert_array_equal(csr, C["full"]["gls"][0])
    np.testing.assert_array_equal(nws, C["full"]["gls"][1])


@pytest.mark.parametrize("which", ["every_third", "cube_and_mfg"])
@pytest.mark.parametrize("meth", METHODS)
def test_target_lists(C, owners, meth, which):
    """Route 3: a target list -- every third node, or exactly the cube nodes and the tiles-in-global-memory kernel's nodes --
    gives the full launch's rows bit for bit on the targets and 0 everywhere else."""
    if which == "every_third":
        t = np.arange(1, C["P"], 3)
    else:
        t = np.sort(np.concatenate([owners["hex8"][0], owners["mfg_tiles"][0]]))
        assert len(t) == C["plan"]["hex8"] + C["plan"]["mfg_tiles"]
    csr, nws = _weights(C["I"], meth, t)
    rows, _ = _layout(C["I"].grid)
    on = np.zeros(C["P"], dtype=bool)
    on[t] = True
    fcsr, fnws = C["full"][meth]
    np.testing.assert_array_equal(csr[on[rows]], fcsr[on[rows]], err_msg=f"{meth} {which}: target rows")
    np.testing.assert_array_equal(nws[on], fnws[on])
    assert not csr[~on[rows]].any() and not nws[~on].any(), (meth, which, "rows outside the list")
    assert np.abs(np.nan_to_num(fcsr[on[rows]])).sum() > 0


@pytest.mark.parametrize("meth", METHODS)
def test_interpolate_in_pieces_and_in_one(C, meth):
    """Route 4: interpolate() cut into quarters of the node range (every piece runs the cube-node kernel on >= 8 workgroups
    next to the other kernels' sub-lists) and in one piece: both against the oracle's CSR, and identical to each other."""
    res = {}
    for mode in ("pieces", "one"):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv(*(("NIN_E2E_MIN_NODES", "0") if mode == "pieces" else ("NIN_E2E_NO_PIPELINE", "1")))
            I = _loaded(C["mesh"])
            W, nws = I.interpolate("u", meth)
        Wo = C["oracle_csr"][meth]
        assert util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data) <= _tol(meth), (mode, meth)
        assert util.csr_elementwise_err(W, Wo.indptr, Wo.indices, Wo.data) <= util.elementwise_rtol(meth), (mode, meth)
        assert util.rowscaled_err(nws, C["oracle"][meth][1]) <= _tol(meth), (mode, meth)
        res[mode] = (W.indptr.copy(), W.indices.copy(), W.data.copy(), np.array(nws))
    for a, b in zip(res["pieces"], res["one"]):
        assert np.array_equal(a, b, equal_nan=True), meth


def test_apply_fused_and_unfused(C):
    """Route 5: GLS apply -- the cube-node kernel forming W . u itself next to the other kernels (and the side stream), and the
    unfused path -- with one field and with three, against the oracle's W . u."""
    Wo, nwo = C["oracle_csr"]["gls"], C["oracle"]["gls"][1]
    u = np.concatenate(C["mesh"].cell_data["u"])
    rng = np.random.default_rng(5)
    fields = np.stack([u, np.cos(2.0 * u), rng.uniform(-1.0, 1.0, len(u))])
    got = {}
    for fused in (True, False):
        with pytest.MonkeyPatch.context() as mp:
            if not fused:
                mp.setenv("NIN_APPLY_NO_FUSION", "1")
            I = _loaded(C["mesh"])
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


def test_device_plan_launches(C, oracle_lib):
    """Route 6: DevicePlan.launch into torch buffers.  Every entry of csr_data and neumann_ws is written (include/ninpol_amd.h:
    skipped nodes get 0): NaN-filled and zero-filled buffers end up equal; two launches back to back on one stream, no sync
    between them, agree; after a Neumann-flag edit and refresh(), a launch into the SAME buffers equals a fresh computation."""
    I = _loaded(C["mesh"])
    dp = I.device_plan("u", "gls")
    ref = C["full"]["gls"]
    for fill in (np.nan, 0.0):
        a, n = _host(_torch_launch(dp, fill))
        np.testing.assert_array_equal(a, ref[0], err_msg=f"fill {fill}")
        np.testing.assert_array_equal(n, ref[1], err_msg=f"fill {fill}")
    x, y = _torch_launch(dp, np.nan), _torch_launch(dp, np.nan)
    (xa, xn), (ya, yn) = _host(x), _host(y)
    np.testing.assert_array_equal(xa, ref[0])
    np.testing.assert_array_equal(ya, ref[0])
    np.testing.assert_array_equal(xn, yn)
    rows, _ = _layout(I.grid)
    an, nn = _host(_torch_launch(dp, np.nan, add_neumann=True))
    np.testing.assert_array_equal(an, ref[0] + ref[1][rows])
    # the flags, edited in place: half of the Neumann nodes become Dirichlet, some Dirichlet boundary nodes become Neumann
    flag_row = I.points_data[I.variable_to_index["points"]["neumann_flag_u"]]
    P = C["P"]
    old = flag_row[:P].copy()
    neu = np.flatnonzero(old != 0)
    dirichlet = np.flatnonzero((old == 0) & (np.asarray(I.grid.boundary_points) != 0))
    flag_row[neu[::2]] = 0.0
    flag_row[dirichlet[::5]] = 1.0
    assert len(neu[::2]) > 0 and len(dirichlet[::5]) > 0
    dp.refresh()
    ea, en = _host(_torch_launch(dp, None, out=x))
    J = _loaded(C["mesh"])
    J.points_data[:] = I.points_data
    fa, fn = _weights(J, "gls")
    np.testing.assert_array_equal(ea, fa)
    np.testing.assert_array_equal(en, fn)
    assert not np.array_equal(fa, ref[0])
    edited = M.Mesh(C["mesh"].points, C["mesh"].cells, cell_data=C["mesh"].cell_data,
                    point_data=dict(C["mesh"].point_data, neumann_flag_u=np.asarray(flag_row[:P]).copy()))
    o = oracle_lib.OracleInterpolator("port", threads=8)
    o.load_mesh(edited)
    wo, nwo = o.prepare("gls", "u")
    assert util.rowscaled_err(_dense(J.grid, fa), wo) <= util.WEIGHT_RTOL
    assert util.rowscaled_err(fn, nwo) <= util.WEIGHT_RTOL


def test_each_kernel_owns_its_rows(C, owners):
    """Route 7: each kernel launched alone (NIN_GLS_ONLY) writes exactly as many rows as the plan gives it, those rows are the
    full launch's bit for bit, no row is written by two kernels, and together they write every row."""
    rows, _ = _layout(C["I"].grid)
    fcsr, fnws = C["full"]["gls"]
    seen = np.zeros(C["P"], dtype=np.int64)
    for name, (mine, vals, nws) in owners.items():
        assert len(mine) == C["plan"][name], name
        on = np.zeros(C["P"], dtype=bool)
        on[mine] = True
        np.testing.assert_array_equal(vals, fcsr[on[rows]], err_msg=name)
        np.testing.assert_array_equal(nws, fnws[mine], err_msg=name)
        seen[mine] += 1
    assert seen.max() == 1, "a row written by two kernels"
    assert seen.min() == 1, "a row no kernel writes"     # (every node is in one list: Dirichlet nodes get their 0 row there)


def test_device_built_grid(C):
    """Route 8: the same union with the grid built on the device."""
    I = _loaded(C["mesh"], grid_build="device")
    for meth in METHODS:
        w, nw = I.prepare_interpolator(meth, "u", np.arange(C["P"]))
        _check(C, I, meth, w, nw, "device grid")
    assert dict(I.grid.gls_plan()) == dict(C["plan"])
