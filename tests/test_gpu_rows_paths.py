"""The IDW / LS row kernels (csrc/kernels_idw_ls.hip) and the row kernels behind interpolate() and apply() (csrc/kernels_csr.hip) on the
paths that no mesh of the GLS parity set reaches: a tile too long for LDS (rows straight from / to HBM), tiles of 32 nodes in the pieces
of interpolate()'s pipeline, IDW's node-on-a-centroid branch, LS's D == 0.0 fallback on rows of more than 8 cells, the padded centroid
records (NIN_ROWS_PAD4), and apply() held to a per-row rounding bound.  The meshes are tests/rows_paths.py's; tests/test_rows_paths.py
pins, with the oracle alone, that they do reach those paths.

Bars: IDW and LS against the oracle at TIGHT = 1e-14 row-scaled (util.rowscaled_err: NaN and inf patterns equal), element-wise <= 1e-14,
the CSR pattern exact (util.csr_rowscaled_err); identities between two GPU runs by np.array_equal(..., equal_nan=True).  Every weight test
first asserts that grid.centroids and grid.point_coords are the oracle's bit for bit: a failure then points at the kernel."""
import copy

import numpy as np
import pytest

import rows_paths as R
import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

TIGHT = 1e-14
METHODS = ("idw", "ls")

MESHES = {
    "fan0": lambda: R.fan_fields(R.fan_axis_first(60, 16, 0)),
    "fan70": lambda: R.fan_fields(R.fan_axis_first(60, 16, 70)),
    "delaunay": lambda: M.attach_fields(R.delaunay_small(), "u", perm="LIN", neumann_plane=(2, 0.0), seed=3),
    "tiny": lambda: R.tiny_tet(),
    "tiny343": lambda: R.tiny_tet(n=6),
    "flat_tet_x": lambda: R.flat_on_axis("tet", 5, 0),
    "flat_wedge_y": lambda: R.flat_on_axis("wedge", 5, 1),
    "flat_tet_z": lambda: R.flat_on_axis("tet", 5, 2),
    "mixed": lambda: M.attach_fields(M.mixed_mesh(9, 5, 5, jitter=0.1, seed=2), "u", perm="ALH", neumann_plane=(2, 0.0), seed=4),
}
FAN_AT = {"fan0": 0, "fan70": 70}


class Case:
    """one mesh and the oracle's answers on it (computed once, shared, never written to)"""

    def __init__(self, name, oracle_lib):
        self.name = name
        self.mesh = MESHES[name]()
        self.o = o = oracle_lib.OracleInterpolator("port", threads=8)
        o.load_mesh(self.mesh)
        self.P, self.E = int(o.grid.n_points), int(o.grid.n_elems)
        self._w, self._W = {}, {}

    def weights(self, meth):
        if meth not in self._w:
            self._w[meth] = self.o.prepare(meth, "u")
            for a in self._w[meth]:
                a.setflags(write=False)
        return self._w[meth]

    def csr(self, meth):
        if meth not in self._W:
            self._W[meth] = self.o.interpolate("u", meth)
        return self._W[meth]

    def loaded(self):
        import ninpol_amd
        I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=self.mesh)
        # the grid is the oracle's bit for bit: what differs below is the kernel's
        assert np.array_equal(np.asarray(I.grid.centroids), self.o.grid.centroids), "centroids"
        assert np.array_equal(np.asarray(I.grid.point_coords), self.o.grid.point_coords), "point_coords"
        assert np.array_equal(np.asarray(I.grid.esup_ptr), self.o.grid.esup_ptr) and np.array_equal(np.asarray(I.grid.esup), self.o.grid.esup)
        return I


_CASES = {}


@pytest.fixture
def case(oracle_lib):
    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(name, oracle_lib)
        return _CASES[name]
    return get


def all_nodes(c):
    return np.arange(c.P)


def assert_weights(c, meth, w, nw, nodes=None, groups=None):
    """dense rows (of `nodes`, default all) against the oracle's; `groups` {name: positions in w}: compared on their own first"""
    wo, no = c.weights(meth)
    if nodes is not None:
        wo, no = wo[nodes], no[nodes]
    for name, sel in (groups or {}).items():
        err = util.rowscaled_err(w[sel], wo[sel])
        assert err <= TIGHT, (c.name, meth, name, err)
    err, el = util.rowscaled_err(w, wo), util.elementwise_err(w, wo)
    print(f"{c.name} {meth}: row-scaled {err:.2e}, element-wise {el:.2e}")
    assert err <= TIGHT, (c.name, meth, err)
    assert el <= 1e-14, (c.name, meth, el)
    assert util.rowscaled_err(nw, no) <= TIGHT, (c.name, meth, "neumann_ws")


def assert_csr(c, meth, W, nws):
    Wo, nwo = c.csr(meth)
    assert W.shape == (c.P, c.E)
    err = util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data)
    el = util.csr_elementwise_err(W, Wo.indptr, Wo.indices, Wo.data)
    assert err <= TIGHT, (c.name, meth, err)
    assert el <= 1e-14, (c.name, meth, el)
    assert util.rowscaled_err(nws, nwo) <= TIGHT, (c.name, meth, "neumann_ws")


def csr_arrays(W, nws):
    return W.indptr.copy(), W.indices.copy(), W.data.copy(), np.array(nws)


def same_arrays(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def interpolate_in(c, monkeypatch, mode, methods=METHODS):
    """interpolate() of a fresh Interpolator in one piece or in the pieces of the pipeline: {meth: (indptr, indices, data, neumann_ws)}"""
    with monkeypatch.context() as mp:
        mp.setenv(*(("NIN_E2E_MIN_NODES", "0") if mode == "pieces" else ("NIN_E2E_NO_PIPELINE", "1")))
        I = c.loaded()
        assert c.P >= 256, "the pipeline needs four pieces of 64 nodes"
        out = {}
        for meth in methods:
            W, nws = I.interpolate("u", meth)
            out[meth] = csr_arrays(W, nws)
            assert_csr(c, meth, W, nws)
    return out


def fan_groups(c):
    """the nodes of the tile past the cap and of the tiles on either side of it"""
    cap, tn, runs = R.rows_tiling(c.o.grid.esup_ptr)
    (t,) = np.flatnonzero(runs > cap)
    g = {"the tile straight from HBM": R.nodes_of_tiles([t], tn, c.P), "the staged tile after it": R.nodes_of_tiles([t + 1], tn, c.P)}
    if t > 0:
        g["the staged tile before it"] = R.nodes_of_tiles([t - 1], tn, c.P)
    return g


# ---- 1. the tile too long for LDS: weights and CSR ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("name", sorted(FAN_AT))
def test_long_tile_weights_and_csr(case, name, meth):
    c = case(name)
    I = c.loaded()
    groups = fan_groups(c)
    w, nw = I.prepare_interpolator(meth, "u", all_nodes(c))
    assert_weights(c, meth, w, nw, groups=groups)
    W, nws = I.interpolate("u", meth)
    # the rows of the three tiles as matrices of their own, then everything
    Wo, _ = c.csr(meth)
    for gname, nodes in groups.items():
        a, b = W[nodes], Wo[nodes]
        assert util.csr_rowscaled_err(a, b.indptr, b.indices, b.data) <= TIGHT, (name, meth, gname)
    assert_csr(c, meth, W, nws)
    # skipped rows (Dirichlet boundary nodes) in the long tile are written as zeros, computed rows are full
    long_tile = groups["the tile straight from HBM"]
    n = np.diff(c.o.grid.esup_ptr)[long_tile]
    stored = np.diff(W.indptr)[long_tile]
    assert np.count_nonzero(stored == 0) >= 5 and np.count_nonzero(stored == n) >= 30


# ---- 2. the long tile: the routes agree ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("name", sorted(FAN_AT))
def test_long_tile_target_list_equals_full_launch(case, name, meth):
    c = case(name)
    I = c.loaded()
    w, nw = I.prepare_interpolator(meth, "u", all_nodes(c))
    axis = R.fan_axis_nodes(16, FAN_AT[name])
    rng = np.random.default_rng(11)
    others = rng.choice(np.setdiff1d(np.arange(c.P - 1), axis), size=40, replace=False)
    targets = rng.permutation(np.concatenate([axis, others, [c.P - 1]])).astype(np.int64)
    wt, nwt = I.prepare_interpolator(meth, "u", targets)
    assert np.array_equal(wt, w[targets], equal_nan=True) and np.array_equal(nwt, nw[targets], equal_nan=True)
    assert_weights(c, meth, wt, nwt, nodes=targets)


@pytest.mark.parametrize("name", sorted(FAN_AT))
def test_long_tile_pieces_equal_one_piece(case, monkeypatch, name):
    c = case(name)
    one, pieces = interpolate_in(c, monkeypatch, "one"), interpolate_in(c, monkeypatch, "pieces")
    for meth in METHODS:
        assert same_arrays(one[meth], pieces[meth]), (name, meth)


@pytest.mark.parametrize("meth", METHODS)
def test_long_tile_host_matrix_follows_dirty_axis_nodes(case, meth):
    """a host matrix (tests/test_gpu_hostmatrix.py) after the axis nodes were marked dirty: their rows -- 120 entries each, overwritten on
    the host first -- come back as a fresh interpolate() has them"""
    c = case("fan70")
    I = c.loaded()
    Mx = I.device_plan("u", meth).host_matrix()
    axis = R.fan_axis_nodes(16, 70)
    I.grid.mark_dirty(nodes=axis.astype(np.int64))
    assert I.grid.dirty_nodes == len(axis)
    indptr = Mx.W.indptr
    for p in axis:
        Mx.W.data[indptr[p]:indptr[p + 1]] = -7.0
        Mx.W.indices[indptr[p]:indptr[p + 1]] = -1
        Mx.neumann[p] = -7.0
    assert Mx.update() == len(axis) and Mx.structure_changed is False
    W, nws = c.loaded().interpolate("u", meth)
    assert same_arrays((Mx.W.indptr, Mx.W.indices, Mx.W.data, Mx.neumann), (W.indptr, W.indices, W.data, nws)), meth
    assert_csr(c, meth, Mx.W, Mx.neumann)
    Mx.release()


# ---- 3. apply() on the long tile and on tiles of 32 nodes -----------------------------------------------------------------------------------
N_FIELDS = (1, 2, 3, 5, 6)      # NF = 1, 2, 4 and the guarded tails 4 + 1, 4 + 2


def cell_fields(c):
    u = np.concatenate(c.mesh.cell_data["u"])
    rng = np.random.default_rng(5)
    return np.ascontiguousarray(np.stack([u, np.sin(3.0 * u)] + [rng.uniform(-1.0, 1.0, len(u)) for _ in range(max(N_FIELDS) - 2)]))


@pytest.mark.parametrize("meth", METHODS)
@pytest.mark.parametrize("name", ["fan70", "delaunay"])
def test_apply_within_the_rounding_bound_of_its_rows(case, name, meth):
    """apply() against the row sums of ITS OWN weights (prepare_interpolator, in esup layout) in 80-bit arithmetic: every finite row
    within rows_paths.apply_model's bound -- (n_p + 1) * 2**-53 * sum |w_j u_j|: a dropped or doubled entry is outside it -- rows with
    a non-finite weight non-finite and no others; a batch of k fields equals k single calls byte for byte"""
    c = case(name)
    I = c.loaded()
    g = c.o.grid
    cap, tn, runs = R.rows_tiling(g.esup_ptr)
    assert tn == (64 if name == "fan70" else 32) and np.count_nonzero(runs > cap) == (1 if name == "fan70" else 0)
    w, nw = I.prepare_interpolator(meth, "u", all_nodes(c))
    assert_weights(c, meth, w, nw)
    data = R.esup_data(g, w, nw)
    rows, _ = util.esup_layout(g)
    bad = np.zeros(c.P, dtype=bool)
    np.logical_or.at(bad, rows, ~np.isfinite(data))
    F = cell_fields(c)
    singles = np.stack([I.apply("u", meth, values=F[f])[0] for f in range(len(F))])
    worst = 0.0
    for f in range(len(F)):
        ref, bound = R.apply_model(g.esup_ptr, g.esup, data, F[f])
        assert np.array_equal(~np.isfinite(singles[f]), bad), (name, meth, f, "non-finite rows")
        ok = ~bad
        d = np.abs(singles[f][ok] - ref[ok])
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound[ok] > 0, d / bound[ok], 0.0))))
        assert np.all(d <= bound[ok]), (name, meth, f, float((d - bound[ok]).max()))
    print(f"{name} {meth}: apply() at most {worst:.3f} of the bound")
    assert np.count_nonzero(singles[0]) >= (c.P - bad.sum()) // 2
    for k in N_FIELDS:
        many, nws = I.apply("u", meth, values=F[:k])
        assert many.shape == (k, c.P)
        assert np.array_equal(many, singles[:k], equal_nan=True), (name, meth, k)
        assert util.rowscaled_err(nws, c.weights(meth)[1]) <= TIGHT


# ---- 4. tiles of 32 nodes in the pieces of the pipeline -----------------------------------------------------------------------------------
def test_tiles_of_32_pieces_equal_one_piece(case, monkeypatch):
    c = case("delaunay")
    cap, tn, runs = R.rows_tiling(c.o.grid.esup_ptr)
    assert tn == 32
    one, pieces = interpolate_in(c, monkeypatch, "one"), interpolate_in(c, monkeypatch, "pieces")     # (both against the oracle there)
    for meth in METHODS:
        assert same_arrays(one[meth], pieces[meth]), meth
    I = c.loaded()
    for meth in METHODS:
        w, nw = I.prepare_interpolator(meth, "u", all_nodes(c))
        assert_weights(c, meth, w, nw)


# ---- 5. IDW's node-on-a-centroid branch ---------------------------------------------------------------------------------------------------
def assert_unit_rows(c, w, indptr, indices, data):
    nodes_o, j_o = R.unit_rows(c.o.grid, c.weights("idw")[0])
    nodes, j = R.unit_rows(c.o.grid, w)
    assert np.array_equal(nodes, nodes_o) and np.array_equal(j, j_o), "the device's unit rows are the oracle's: same node, same j"
    assert np.count_nonzero(j >= 8) >= 10 and np.count_nonzero(j >= 16) >= 3
    ptr, esup = c.o.grid.esup_ptr, c.o.grid.esup
    assert np.all(np.diff(indptr)[nodes] == 1), "a unit row has exactly one stored entry"
    assert np.array_equal(indices[indptr[nodes]], esup[ptr[nodes] + j]) and np.all(data[indptr[nodes]] == 1.0)


def test_idw_epsilon_rows(case):
    """tiny_tet(): 216 nodes -- interpolate() is never cut into pieces below 256 nodes, so this mesh runs in one piece"""
    c = case("tiny")
    I = c.loaded()
    w, nw = I.prepare_interpolator("idw", "u", all_nodes(c))
    assert_weights(c, "idw", w, nw)
    W, nws = I.interpolate("u", "idw")
    assert_csr(c, "idw", W, nws)
    assert_unit_rows(c, w, W.indptr, W.indices, W.data)
    targets = np.arange(1, c.P, 3)
    wt, nwt = I.prepare_interpolator("idw", "u", targets)
    assert np.array_equal(wt, w[targets]) and np.array_equal(nwt, nw[targets])
    wl, nwl = I.prepare_interpolator("ls", "u", all_nodes(c))         # LS on the same mesh: no epsilon there
    assert_weights(c, "ls", wl, nwl)


def test_idw_epsilon_rows_in_pieces(case, monkeypatch):
    """the same cells, 343 nodes: in one piece and in the four pieces of the pipeline (unit rows in every piece)"""
    c = case("tiny343")
    I = c.loaded()
    w, nw = I.prepare_interpolator("idw", "u", all_nodes(c))
    assert_weights(c, "idw", w, nw)
    res = {}
    for mode in ("one", "pieces"):
        res[mode] = interpolate_in(c, monkeypatch, mode, methods=("idw",))["idw"]
        assert_unit_rows(c, w, *res[mode][:3])
    assert same_arrays(res["one"], res["pieces"])


# ---- 6. LS's D == 0.0 fallback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat_tet_x", "flat_wedge_y", "flat_tet_z"])
def test_ls_fallback_on_flat_meshes(case, name):
    c = case(name)
    I = c.loaded()
    n = np.diff(c.o.grid.esup_ptr)
    for meth in ("ls", "idw"):
        w, nw = I.prepare_interpolator(meth, "u", all_nodes(c))
        assert_weights(c, meth, w, nw, groups={"rows of more than 8 cells": np.flatnonzero(n > 8), "rows of at most 8": np.flatnonzero(n <= 8)})
        if meth == "ls":
            fb = R.fallback_rows(c.o.grid, w)
            assert (not fb.any()) if name == "flat_tet_z" else (fb.all() and np.count_nonzero(n > 8) >= 40), name
        targets = np.arange(0, c.P, 3)
        wt, nwt = I.prepare_interpolator(meth, "u", targets)
        assert np.array_equal(wt, w[targets], equal_nan=True) and np.array_equal(nwt, nw[targets], equal_nan=True), (name, meth)
        assert_weights(c, meth, wt, nwt, nodes=targets)
        W, nws = I.interpolate("u", meth)
        assert_csr(c, meth, W, nws)


# ---- 7. padded centroid records -------------------------------------------------------------------------------------------------------------
def run_both(I, P):
    out = []
    for meth in METHODS:
        out += list(I.prepare_interpolator(meth, "u", np.arange(P)))
        out += list(csr_arrays(*I.interpolate("u", meth)))
    return out


@pytest.mark.parametrize("name", ["tiny", "flat_tet_x", "fan70", "mixed"])
def test_padded_centroids_are_bit_identical(case, monkeypatch, name):
    """NIN_ROWS_PAD4 (read when the grid goes to the device): IDW and LS gather (x, y, z, 0) records; the same bytes out.  On the mixed
    mesh then a local update_points(nodes=) (tests/test_gpu_update_points_local.py), which rewrites the padded records of the cells
    around the moved nodes: both builds equal a fresh Interpolator loaded with the moved mesh."""
    import ninpol_amd
    import torch
    c = case(name)
    got = {}
    for pad in (False, True):
        with monkeypatch.context() as mp:
            if pad:
                mp.setenv("NIN_ROWS_PAD4", "1")
            else:
                mp.delenv("NIN_ROWS_PAD4", raising=False)
            I = c.loaded()
            got[pad] = (I, run_both(I, c.P))
    assert same_arrays(got[False][1], got[True][1]), name
    for meth, k in zip(METHODS, (0, 6)):
        assert_weights(c, meth, got[True][1][k], got[True][1][k + 1])
    if name != "mixed":
        return
    X = np.ascontiguousarray(np.asarray(c.mesh.points, dtype=np.float64)).copy()
    rng = np.random.default_rng(17)
    nodes = rng.choice(c.P, size=30, replace=False).astype(np.int64)
    X[nodes] += rng.uniform(-0.004, 0.004, (30, 3))
    moved = copy.copy(c.mesh)
    moved.points = X
    F = ninpol_amd.Interpolator()
    F.load_mesh(mesh_obj=moved)
    fresh = run_both(F, c.P)
    assert not same_arrays(fresh, got[False][1]), "the move changes the weights"
    for pad in (False, True):
        I = got[pad][0]
        I.update_points(torch.from_numpy(X[nodes]).cuda(), nodes=torch.from_numpy(nodes).cuda())
        torch.cuda.current_stream().synchronize()
        assert same_arrays(run_both(I, c.P), fresh), ("after update_points(nodes=)", pad)
