"""The numpy model of the GLS shape adjoint (tests/gls_shape_model.py) pinned on the CPU, on jittered hexahedra, tetrahedra, a mixed
mesh and a random-cloud Delaunay mesh, ALH tensor, Neumann plane z = 0:

  (a) against central differences of the model's own forward with the geometry recomputed from the moved coordinates in float64
      (centroid, face centre, unit normal of the first three points): h = 1e-6, 40 sampled coordinates, FD_RTOL of max |grad|;
  (b) against central differences of the oracle itself, the mesh loaded again with the moved points so that the float32 normals are
      in: h = 1e-3, 12 coordinates, 1e-4 of max |grad| -- what stands between (a) and (b) is the float32 noise of the normals;
  (c) three one-line mutants of the model each miss bar (a) on a named mesh;
  (d) translating every point leaves every weight alone: per axis the gradient sums to zero on the scale of its contributions."""
import numpy as np
import pytest

import gls_shape_model as SM
from ninpol_amd import mesh as M
from gls_shape_model import ADJOINT_RTOL
from test_gls_adjoint_model import FD_RTOL, MESHES, oracle_case, stored

H_SMOOTH, N_SMOOTH = 1e-6, 40
H_ORACLE, N_ORACLE = 1e-3, 12
# ten times the 9.0e-6 measured at this step (hex; 8.9e-6 tet, 1.3e-6 mixed): the truncation error of the step on one side, the float32
# noise of the reloaded normals on the other (it reaches 2e-5 at h = 1e-4)
ORACLE_RTOL = 1e-4
MUTANT_MESH = {"quad_fourth_vertex": "hex", "normal_projection": "tet", "dtau": "mixed"}


def around(grid, v):
    """the nodes whose rows can move with point v: the points of the cells around it"""
    ptr, esup = np.asarray(grid.esup_ptr), np.asarray(grid.esup)
    inpoel = np.asarray(grid.inpoel)
    rows = inpoel[esup[ptr[v]:ptr[v + 1]]]
    return np.unique(rows[rows >= 0]).astype(np.int64)


class Case:
    def __init__(self, name, oracle_lib):
        self.name, self.lib = name, oracle_lib
        self.make = MESHES[name][0]
        self.o, self.perm, self.dmag, self.flag, self.rows = oracle_case(oracle_lib, self.make)
        g = self.grid = self.o.grid
        self.coords = np.array(g.point_coords, dtype=np.float64).reshape(-1, 3)
        self.P = len(self.coords)
        rng = np.random.default_rng(17)
        self.ghat, self.gnws = rng.uniform(-1.0, 1.0, len(g.esup)), rng.uniform(-1.0, 1.0, self.P)
        self._smooth = None

    def model(self, grid, **kw):
        return SM.shape_adjoint(grid, self.perm, self.dmag, self.flag, self.grid.inpoel, self.grid.inpofa, self.ghat, self.gnws,
                                add_neumann=True, dtype=np.float64, **kw)

    def smooth(self):
        """(the smooth bag, [(point, axis, central difference of the smooth forward)])"""
        if self._smooth is None:
            g = self.grid
            bag = SM.smooth_bag(g, self.coords, g.inpoel, g.inpofa)
            picks = np.random.default_rng(5).choice(self.P * 3, size=N_SMOOTH, replace=False)
            fd = []
            for idx in picks:
                v, k = divmod(int(idx), 3)
                nodes = around(g, v)
                vals = []
                for sgn in (+1, -1):
                    X = self.coords.copy()
                    X[v, k] += sgn * H_SMOOTH
                    vals.append(SM.loss(SM.smooth_bag(g, X, g.inpoel, g.inpofa), self.perm, self.dmag, self.flag, self.ghat, self.gnws, True, nodes))
                fd.append((v, k, (vals[0] - vals[1]) / (2 * H_SMOOTH)))
            self._smooth = (bag, fd)
        return self._smooth

    def smooth_err(self, mutant=None):
        bag, fd = self.smooth()
        grad = self.model(bag, mutant=mutant)["grad_points"]
        scale = np.abs(self.model(bag)["grad_points"]).max() if mutant else np.abs(grad).max()
        return max(abs(d - grad[v, k]) for v, k, d in fd) / scale, scale


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()          # (the oracle's grids go while its library is still loaded)


@pytest.fixture(params=sorted(MESHES))
def case(request, oracle_lib):
    return get(request.param, oracle_lib)


def get(name, oracle_lib):
    if name not in _CASES:
        _CASES[name] = Case(name, oracle_lib)
    return _CASES[name]


def test_smooth_normals_are_the_resident_ones(case):
    """the float64 normals of the smooth forward against the resident float32 ones: the same orientation, float32 apart"""
    bag, _ = case.smooth()
    d = np.abs(bag.normal_faces - np.asarray(case.grid.normal_faces).reshape(-1, 3)).max()
    print(f"{case.name}: float64 normals against the resident ones {d:.2e}")
    assert d <= 4e-7
    assert np.abs(bag.centroids - np.asarray(case.grid.centroids).reshape(-1, 3)).max() <= 1e-15
    assert np.abs(bag.faces_centers - np.asarray(case.grid.faces_centers).reshape(-1, 3)).max() <= 1e-15


def test_gradient_is_the_central_difference_of_the_smooth_forward(case):
    worst, scale = case.smooth_err()
    m = case.model(case.smooth()[0])
    dirichlet = (np.asarray(case.grid.boundary_points).astype(np.int64) != 0) & (case.flag == 0)
    assert dirichlet.any() and not m["computed"][dirichlet].any() and np.abs(m["grad_points"][dirichlet]).max() > 0
    print(f"{case.name}: worst |FD - model| / max|grad| = {worst:.2e} over {N_SMOOTH} coordinates (max|grad| = {scale:.3e})")
    assert worst <= FD_RTOL


def test_gradient_is_the_central_difference_of_the_oracle(case):
    o, g = case.o, case.grid
    grad = case.model(g)["grad_points"]
    scale = np.abs(grad).max()
    perm_row, dmag_row = case.rows
    E = len(case.perm)
    picks = np.random.default_rng(7).choice(case.P * 3, size=N_ORACLE, replace=False)
    worst = 0.0
    for idx in picks:
        v, k = divmod(int(idx), 3)
        nodes = around(g, v)
        vals = []
        for sgn in (+1, -1):
            mesh = M.attach_fields(case.make(), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
            mesh.points = np.ascontiguousarray(case.coords.copy())
            mesh.points[v, k] += sgn * H_ORACLE
            o2 = case.lib.OracleInterpolator("port", threads=2)
            o2.load_mesh(mesh)
            assert np.array_equal(o2.grid.esup, g.esup) and np.array_equal(o2.grid.inpofa, g.inpofa)
            o2.cells_data[perm_row][:E * 9] = case.perm.reshape(-1)       # the fields of the unmoved mesh
            o2.cells_data[dmag_row][:E] = case.dmag
            assert np.array_equal(np.asarray(o2.points_data[o2.variable_to_index["points"]["neumann_flag_u"]][:case.P]).astype(np.int64), case.flag)
            d, nws = stored(o2, nodes)
            vals.append(float(case.ghat @ d + case.gnws @ nws))
        fd = (vals[0] - vals[1]) / (2 * H_ORACLE)
        worst = max(worst, abs(fd - grad[v, k]) / scale)
    print(f"{case.name}: oracle, worst |FD - model| / max|grad| = {worst:.2e} over {N_ORACLE} coordinates, h = {H_ORACLE}")
    assert worst <= ORACLE_RTOL


@pytest.mark.parametrize("mutant", SM.MUTANTS)
def test_a_mutant_misses_the_bar(mutant, oracle_lib):
    c = get(MUTANT_MESH[mutant], oracle_lib)
    worst, _ = c.smooth_err(mutant)
    print(f"{c.name}: mutant {mutant}: worst |FD - model| / max|grad| = {worst:.2e}")
    assert worst > FD_RTOL


def test_translation_invariance(case):
    m = case.model(case.grid)
    total, room = np.abs(m["grad_points"].sum(axis=0)), m["scale"].sum(axis=0)
    print(f"{case.name}: |sum_p grad_points[p]| / sum_p scale[p] per axis: " + ", ".join(f"{t / r:.2e}" for t, r in zip(total, room)))
    assert np.all(room > 0) and np.all(total <= ADJOINT_RTOL * room)
