"""The GLS derivative and gradient operations on grids BUILT ON THE DEVICE (Interpolator(grid_build="device"), csrc/grid_device.hip,
DESIGN.md 4.5), in the states of the device-built grid's host mirror (tests/device_grid_twins.py: STATES): the permeability adjoint
and tangent, the kept Jacobians in K (full and reduced) and their dirty relinearisation, the shape adjoint, the shape tangent, the kept
shape Jacobian, its block-CSR assembly and its dirty relinearisation, the corner gradients, and the Python wrappers that read grid
arrays on the host.

Every test loads one mesh into two Interpolators, grid_build="host" and grid_build="device", drives both through the same calls with
the same inputs and compares every output by bytes; a dirty relinearisation is compared with a fresh full linearisation on the
device-built grid too.  There is no tolerance in this module: tests/test_gpu_gls_*.py hold the host-built path to the 80-bit models,
and byte equality carries that over.

The shape operations read inpoel / inpofa on the device through ensure_update_inputs without any geometry update having run: on a
device-built grid they borrow the mirror's buffers and nothing refreshes them ("borrow without update"); release_scratch() and a lazy
read of inpoel, inpofa and faces_areas follow.

The mesh is mixed_mesh(4, 3, 3) with jitter, the ALH tensor and the Neumann plane z = 0 (tests/test_gpu_gls_shape_adjoint.py's); the
random-cloud Delaunay mesh, which populates every bin of the adjoint kernel, runs the shape adjoint and the corner gradients once."""
import numpy as np
import pytest

import device_grid_twins as TW
import test_gpu_gls_corner_gradients as CG
import test_gpu_gls_jacobian_dirty as JD
import test_gpu_gls_shape_adjoint as SA
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

N_DIR = JD.N_DIR


def _torch():
    import torch
    return torch


def _mesh(name):
    return M.attach_fields(SA.MESHES[name](), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)


class Side(JD.Case):
    """One twin behind the interface of test_gpu_gls_jacobian_dirty.Case (fresh / redo / buffers / products / assembled).  Nothing is
    read from the grid's host arrays here: the connectivity the helpers need comes from `conn`, read from a third, host-built load."""

    def __init__(self, I, name, mesh, conn):
        torch = _torch()
        self.name, self.I = name, I
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        self.dev = torch.device("cuda", int(I.device))
        perm, _ = I._perm_rows()
        self.K0 = np.array(perm).reshape(self.E, 9)
        self.X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64)).reshape(self.P, 3)
        self.flag0 = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        self.inpoel, self.boundary, self.node_of_esup, self.node_of_fsup = conn
        rng = np.random.default_rng(71)
        self.u0, self.b0 = rng.uniform(-1.0, 1.0, self.E), rng.uniform(-1.0, 1.0, self.P)
        self.u2 = self.u0 + rng.uniform(0.5, 1.0, self.E)
        self.basis6 = self.to_dev(rng.uniform(-1.0, 1.0, (self.E, 6, 9)))
        self.d = {"K": rng.uniform(-1.0, 1.0, (N_DIR, self.E, 9)), "R1": rng.uniform(-1.0, 1.0, (N_DIR, self.E, 1)),
                  "R6": rng.uniform(-1.0, 1.0, (N_DIR, self.E, 6)), "X": rng.uniform(-1.0, 1.0, (N_DIR, self.P, 3))}
        self.vs = rng.uniform(-1.0, 1.0, (N_DIR, self.P))
        self.ghat, self.gnws = rng.uniform(-1.0, 1.0, self.nnz), rng.uniform(-1.0, 1.0, self.P)
        self.gdm = rng.uniform(-1.0, 1.0, self.E)
        self.fields = rng.uniform(-1.0, 1.0, (CG.N_FIELDS, self.E))

    def make_plan(self):
        from ninpol_amd.interpolator import DevicePlan
        self.plan = DevicePlan(self.I, "u", "gls")

    def nan(self, *shape):
        return _torch().full(shape, float("nan"), dtype=_torch().float64, device=self.dev)

    def host(self, *tensors):
        self.sync()
        return [t.cpu().numpy() for t in tensors]


_CONN = {}


def conn_of(name):
    """(inpoel, boundary nodes, the node of every esup row, of every fsup row) of a host-built load of the mesh"""
    if name not in _CONN:
        g = TW.load(_mesh(name), "host").grid
        P = int(g.n_points)
        _CONN[name] = (np.array(g.inpoel).astype(np.int64), np.asarray(g.boundary_points).astype(np.int64) != 0,
                       np.repeat(np.arange(P), np.diff(np.asarray(g.esup_ptr).astype(np.int64))),
                       np.repeat(np.arange(P), np.diff(np.asarray(g.fsup_ptr).astype(np.int64))))
    return _CONN[name]


def sides(name, state, **kw):
    """the twins of mesh `name`, the device-built one in `state`, each with its GLS plan; the dirty sets cleared"""
    mesh = _mesh(name)
    H, D = TW.twins(mesh, **kw)
    TW.enter(H, D, state)
    h, d = Side(H, name + "/host", mesh, conn_of(name)), Side(D, name + "/device", mesh, conn_of(name))
    for s in (h, d):
        s.make_plan()
        s.grid.clear_dirty(s.stream())
        s.sync()
        assert s.grid.dirty_nodes == 0
    return h, d


def equal(what, a, b, zero_ok=False):
    """two lists of arrays, the host-built twin's and the device-built twin's: the same bytes, finite, not all zero"""
    assert len(a) == len(b) and len(a) > 0, what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, i, int(np.count_nonzero(x != y)))
        assert np.all(np.isfinite(x)), (what, i)
        assert zero_ok or np.count_nonzero(x) > 0, (what, i, "all zero")


def compare_kept(h, d, Jh, Jd, kind, what, products=True):
    equal((what, kind, "records"), [a for _, a, _ in h.buffers(Jh, kind)], [a for _, a, _ in d.buffers(Jd, kind)])
    if products:
        equal((what, kind, "products"), h.products(Jh, kind), d.products(Jd, kind))
    assert Jh.is_current() and Jd.is_current() and Jh.stamp == Jd.stamp, (what, kind)


# ---- 1. the permeability: adjoint, tangent, the kept Jacobians and their dirty relinearisation -----------------------------------------

def k_derivatives(s):
    """launch_weights_backward (both ways of treating diff_mag and neumann_ws) and launch_weights_tangent for two directions"""
    out = []
    g, gn, gdm = s.to_dev(s.ghat), s.to_dev(s.gnws), s.to_dev(s.gdm)
    gp, gd = s.nan(s.E, 9), s.nan(s.E)
    s.plan.launch_weights_backward(g.data_ptr(), gp.data_ptr(), 0, gn.data_ptr(), s.stream(), add_neumann=True)
    out += s.host(gp)
    gp = s.nan(s.E, 9)
    s.plan.launch_weights_backward(g.data_ptr(), gp.data_ptr(), gd.data_ptr(), 0, s.stream(), add_neumann=False)
    out += s.host(gp, gd)
    tp, tdm = s.to_dev(s.d["K"][:2]), s.to_dev(np.stack([s.gdm, -s.gdm]))
    tc, tn = s.nan(2, s.nnz), s.nan(2, s.P)
    s.plan.launch_weights_tangent(tp.data_ptr(), tc.data_ptr(), 2, 0, tn.data_ptr(), s.stream(), add_neumann=True)
    out += s.host(tc, tn)
    tc = s.nan(2, s.nnz)
    s.plan.launch_weights_tangent(tp.data_ptr(), tc.data_ptr(), 2, tdm.data_ptr(), 0, s.stream(), add_neumann=False)
    out += s.host(tc)
    return out


@pytest.mark.parametrize("state", ("cold", "full", "lent_released"))
def test_permeability_derivatives(state):
    h, d = sides("mixed", state)
    what = ("K", state)
    equal((what, "adjoint and tangent"), k_derivatives(h), k_derivatives(d))
    kinds = ("K", "R1", "R6")
    J = {s: {k: s.fresh(k, s.u0, s.b0) for k in kinds} for s in (h, d)}
    for k in kinds:
        compare_kept(h, d, J[h][k], J[d][k], k, (what, "linearize"))
    before = {k: [a.copy() for _, a, _ in d.buffers(J[d][k], k)] for k in kinds}
    # a local permeability update, then only the dirty rows: against the host-built twin and against a fresh full linearisation
    ids, rows, u1 = h.some_cells()
    marked = h.vertices(ids)
    for s in (h, d):
        s.update_cells(ids, rows)
        assert s.grid.dirty_nodes == len(marked) and 0 < len(marked) < s.P
        for i, k in enumerate(kinds):
            assert not J[s][k].is_current()
            assert s.redo(J[s][k], k, u1, s.b0, clear=(i == len(kinds) - 1)) == len(marked), (what, k)
        assert s.grid.dirty_nodes == 0
    for k in kinds:
        compare_kept(h, d, J[h][k], J[d][k], k, (what, "relinearize_dirty"))
        d.same(J[d][k], k, d.fresh(k, u1, d.b0), (what, "relinearize_dirty against a fresh linearisation"))
        assert any(a.tobytes() != b.tobytes() for a, (_, b, _) in zip(before[k], d.buffers(J[d][k], k))), (what, k, "the update changed nothing")
    (ph, dh), (pd, dd) = h.grid.fetch_permeability(), d.grid.fetch_permeability()
    assert pd.tobytes() == ph.tobytes() and dd.tobytes() == dh.tobytes() and pd[ids].tobytes() == rows.tobytes()
    TW.assert_lazy_arrays_same(h.I, d.I, what)


# ---- 2. the node coordinates: shape adjoint, shape tangent, the kept shape Jacobian, its assembly, its dirty relinearisation ----------

def x_derivatives(s):
    """launch_weights_backward_points for both add_neumann values, with and without grad_neumann_ws; launch_weights_tangent_points"""
    out = []
    g, gn = s.to_dev(s.ghat), s.to_dev(s.gnws)
    for add_neumann in (True, False):
        for with_nws in (True, False):
            gx = s.nan(s.P, 3)
            s.plan.launch_weights_backward_points(g.data_ptr(), gx.data_ptr(), gn.data_ptr() if with_nws else 0, s.stream(), add_neumann=add_neumann)
            out += s.host(gx)
    assert out[0].tobytes() != out[3].tobytes()          # both terms really enter: the variants answer differently
    dX = s.to_dev(s.d["X"][:2])
    for add_neumann in (True, False):
        tc, tn = s.nan(2, s.nnz), s.nan(2, s.P)
        s.plan.launch_weights_tangent_points(dX.data_ptr(), tc.data_ptr(), 2, tn.data_ptr(), s.stream(), add_neumann=add_neumann)
        out += s.host(tc, tn)
    return out


def assembled(s, J):
    block_ptr, block_col = J.fetch_pattern()
    return [block_ptr, block_col, s.assembled(J)]


@pytest.mark.parametrize("state", ("cold", "partial", "full", "lent_released"))
def test_shape_derivatives(state):
    h, d = sides("mixed", state)
    what = ("X", state)
    equal((what, "adjoint and tangent"), x_derivatives(h), x_derivatives(d))
    J = {s: s.fresh("X", s.u0, s.b0) for s in (h, d)}
    compare_kept(h, d, J[h], J[d], "X", (what, "linearize"))
    equal((what, "assembled"), assembled(h, J[h]), assembled(d, J[d]))
    pattern = [a.copy() for a in J[d].fetch_pattern()]
    products = d.products(J[d], "X")
    # the borrowed connectivity across release_scratch(), read lazily, and the kept object's launches behind it
    for s in (h, d):
        s.grid.release_scratch()
    for k in ("inpoel", "inpofa", "faces_areas"):
        assert TW.same(getattr(h.grid, k), getattr(d.grid, k)) and np.count_nonzero(getattr(d.grid, k)) > 0, (what, k)
    equal((what, "products after release_scratch"), products, d.products(J[d], "X"))
    equal((what, "adjoint and tangent after release_scratch"), x_derivatives(h), x_derivatives(d))
    # a local move, then only the dirty rows
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(h.P, max(2, h.P // 40), replace=False))
    rows = h.X0[ids] + rng.uniform(-0.01, 0.01, (len(ids), 3))
    marked = h.around(ids)
    before = [a.copy() for _, a, _ in d.buffers(J[d], "X")]
    from ninpol_amd import _lib
    for s in (h, d):
        s.I.update_points(s.to_dev(rows), nodes=s.to_dev(ids, np.int64))
        with pytest.raises(_lib.NinpolError):          # the records are applied through the resident geometry: refused until relinearised
            s.products(J[s], "X")
        assert s.redo(J[s], "X", s.u0, s.b0) == len(marked) and 0 < len(marked) < s.P, (what, s.name)
        assert s.grid.dirty_nodes == 0
    compare_kept(h, d, J[h], J[d], "X", (what, "relinearize_dirty"))
    F = d.fresh("X", d.u0, d.b0)
    d.same(J[d], "X", F, (what, "relinearize_dirty against a fresh linearisation"))
    assert any(a.tobytes() != b.tobytes() for a, (_, b, _) in zip(before, d.buffers(J[d], "X"))), (what, "the move changed nothing")
    equal((what, "assembled after the move"), assembled(h, J[h]), assembled(d, J[d]))
    equal((what, "assembled against a fresh linearisation"), assembled(d, F), assembled(d, J[d]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pattern, J[d].fetch_pattern()))
    for k in TW.GEOMETRY:
        assert TW.same(getattr(h.grid, k), getattr(d.grid, k)), (what, k)
    X1 = h.X0.copy()
    X1[ids] = rows
    assert np.array_equal(d.grid.point_coords, X1)
    TW.assert_lazy_arrays_same(h.I, d.I, what)


# ---- 3. the corner gradients ------------------------------------------------------------------------------------------------------------

def corner_gradients(s):
    torch = _torch()
    k = CG.N_FIELDS
    bufs = [s.nan(k, s.nnz, 3), s.nan(k, s.P), s.nan(k, s.nnz, 3), s.nan(k, s.P, 3)]          # grad, node_values, flux, node_gradient
    ud = s.to_dev(s.fields)
    s.plan.launch_corner_gradients(ud.data_ptr(), bufs[0].data_ptr(), k, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), s.stream())
    out = s.host(*bufs)
    torch.cuda.synchronize()
    grad, flux = s.I.corner_gradients("u", s.fields, flux=True)
    return out + [grad, flux, s.I.node_gradient("u", s.fields), s.I.corner_gradients("u")]


@pytest.mark.parametrize("state", ("cold", "full", "lent_released"))
def test_corner_gradients(state):
    h, d = sides("mixed", state)
    a, b = corner_gradients(h), corner_gradients(d)
    equal(("corner gradients", state), a, b)
    assert b[4].tobytes() == b[0].tobytes() and b[5].tobytes() == b[2].tobytes() and b[6].tobytes() == b[3].tobytes()      # the wrappers are the launch
    TW.assert_lazy_arrays_same(h.I, d.I, ("corner gradients", state))


# ---- 4. every bin of the adjoint kernel, once ----------------------------------------------------------------------------------------------

def test_every_adjoint_bin_on_the_delaunay_mesh():
    h, d = sides("delaunay", "cold")
    plans = [s.grid.gls_adjoint_plan() for s in (h, d)]
    assert plans[0] == plans[1] and list(plans[1]) == ["lds1", "lds2", "lds4", "global"], plans
    assert all(v > 0 for v in plans[1].values()) and sum(plans[1].values()) == d.P, plans
    equal("delaunay, shape adjoint and tangent", x_derivatives(h), x_derivatives(d))
    equal("delaunay, corner gradients", corner_gradients(h), corner_gradients(d))
    TW.assert_lazy_arrays_same(h.I, d.I, "delaunay")


# ---- 5. the Python wrappers that read grid arrays on the host -----------------------------------------------------------------------------

def wrappers(s, ids, rows, nodes, moved):
    """the host-synchronous entry points and the scipy operators (to_scipy() reads esup and esup_ptr from the grid on the host), their
    update() after a local permeability update and after a local move"""
    I = s.I
    out = [I.permeability_gradient("u", s.vs[:2], np.stack([s.u0, s.u2])), I.points_gradient("u", s.vs[:2], np.stack([s.u0, s.u2]))]
    out += list(I.permeability_tangent("u", s.d["K"][:2].reshape(2, s.E, 3, 3))) + list(I.points_tangent("u", s.d["X"][:2]))
    JK = I.permeability_jacobian("u", s.u0, s.b0)
    JR = I.permeability_jacobian("u", s.u0, s.b0, basis="symmetric")
    JX = I.points_jacobian("u", s.u0, s.b0)

    def explicit():
        A, R, X = JK.to_scipy(), JR.to_scipy(), JX.assemble()
        return [A.data, A.indices, A.indptr, R.data, R.indices, R.indptr, X.data, X.indices, X.indptr,
                JK.matvec(s.d["K"][0].reshape(-1)), JK.rmatvec(s.vs[0]), JX.matvec(s.d["X"][0].reshape(-1)), JX.rmatvec(s.vs[0])]
    out += explicit()
    s.grid.clear_dirty()
    I.update_permeability(s.to_dev(rows), cells=s.to_dev(ids, np.int64))
    I.update_points(s.to_dev(moved), nodes=s.to_dev(nodes, np.int64))
    s.sync()
    n = [JK.update(s.u0, s.b0, clear=False), JR.update(s.u0, s.b0, clear=False), JX.update(s.u0, s.b0)]
    assert n[0] == n[1] == n[2] > 0 and s.grid.dirty_nodes == 0
    after = explicit()
    assert after[0].tobytes() != out[-13].tobytes() and after[6].tobytes() != out[-7].tobytes()          # the updates moved both Jacobians
    return out + [np.array(n)] + after


@pytest.mark.parametrize("state", ("cold", "full"))
def test_host_wrappers_and_scipy_operators(state):
    h, d = sides("mixed", state)
    ids, rows, _ = h.some_cells(seed=1)
    nodes = np.sort(np.random.default_rng(8).choice(h.P, max(2, h.P // 40), replace=False))
    moved = h.X0[nodes] + np.random.default_rng(9).uniform(-0.01, 0.01, (len(nodes), 3))
    equal(("wrappers", state), wrappers(h, ids, rows, nodes, moved), wrappers(d, ids, rows, nodes, moved), zero_ok=True)
    TW.assert_lazy_arrays_same(h.I, d.I, ("wrappers", state))
