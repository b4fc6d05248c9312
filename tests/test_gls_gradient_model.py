"""The numpy model of the GLS corner gradients (tests/gls_gradient_model.py) pinned on the CPU, on the jittered hexahedra, tetrahedra,
mixed and random-cloud Delaunay meshes of tests/test_gls_adjoint_model.py (ALH tensor, Neumann plane z = 0):

  (a) its node value u_p is W u of the oracle's weights without the `+ neumann_ws` term, to the parity bar of tests/util.py: an entry
      of a row may be WEIGHT_RTOL of the row's largest weight away, so the product may be that times sum_i |u_i|;
  (b) (g, u_p) satisfies the normal equations of [A | c] in 80 bits: the defect, on the scale of its own terms, is a few units of the
      80-bit roundoff times the growth of the solve -- held under 2^-40, nine orders below anything a wrong right-hand side leaves;
  (c) two mutants of the model -- a nonzero b on a face row, a missing c u_p term -- are told apart from it on every mesh, by the
      normal equations and by the distance between the answers;
  (d) linear exactness on one block of one anisotropic tensor with an all-Dirichlet boundary: u = a + beta . x at the centroids meets
      every row of every interior node's system with zero residual, so g_i = beta and u_p = a + beta . x_p whatever the weighting.
      The yardstick is what the float64 rounding of the cell values may move the 80-bit answer by (the model's `room`, propagated
      through |A+|), not a fixed tolerance: the 80-bit solve itself loses 2^-11 of that."""
import numpy as np
import pytest

import gls_derivative_exact as D
import gls_gradient_model as GG
import util
from gls_exact import LD
from ninpol_amd import mesh as M
from test_gls_adjoint_model import MESHES, oracle_case

NORMAL_EQUATIONS_CAP = 2.0 ** -40
A0, BETA = 0.3, (1.0, -2.0, 0.5)
LINEAR_MESHES = {
    "hex": lambda: M.hex_mesh(4, jitter=0.1),
    "delaunay": lambda: M.delaunay_tet_mesh(6, lattice="random"),
}

_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()          # (the oracle's grids go while its library is still loaded)


class Case:
    def __init__(self, name, oracle_lib):
        self.name = name
        self.o, self.perm, self.dmag, self.flag, _ = oracle_case(oracle_lib, MESHES[name][0])
        self.grid = self.o.grid
        self.u = np.random.default_rng(23).uniform(-1.0, 1.0, self.grid.n_elems)
        self._m = {}

    def model(self, dtype=LD, mutant=None):
        if (dtype, mutant) not in self._m:
            self._m[(dtype, mutant)] = GG.corner_gradients(self.grid, self.perm, self.dmag, self.flag, self.u, dtype, mutant)
        return self._m[(dtype, mutant)]

    def defect(self, model):
        return GG.normal_equation_defect(self.grid, self.perm, self.dmag, self.flag, self.u, model)


@pytest.fixture(params=sorted(MESHES))
def case(request, oracle_lib):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param, oracle_lib)
    return _CASES[request.param]


def test_node_value_is_the_oracles_weights_applied(case):
    g = case.grid
    w, _ = case.o.prepare("gls", "u", None)                        # [P][mx]: the weights without `+ neumann_ws`
    ptr, esup = np.asarray(g.esup_ptr), np.asarray(g.esup)
    m = case.model()
    worst = 0.0
    for p in range(g.n_points):
        cells = esup[ptr[p]:ptr[p + 1]]
        row = w[p, :len(cells)]
        assert bool(np.any(row != 0)) == bool(m["computed"][p]), p
        if not m["computed"][p]:
            assert m["node_values"][0, p] == 0 and not m["grad"][0, ptr[p]:ptr[p + 1]].any()
            continue
        room = np.abs(row).max() * np.abs(case.u[cells]).sum()
        worst = max(worst, abs(float(m["node_values"][0, p]) - float(row @ case.u[cells])) / room)
    print(f"{case.name}: |u_p - W u| / (max |w| sum |u|) {worst:.2e}")
    assert 0 < m["computed"].sum() < g.n_points and worst <= util.WEIGHT_RTOL


def test_normal_equations_in_80_bits(case):
    m = case.model()
    d = case.defect(m)
    print(f"{case.name}: normal-equation defect of the 80-bit model {d:.2e}")
    assert d <= NORMAL_EQUATIONS_CAP
    assert np.count_nonzero(m["grad"]) > 0 and np.all(m["scale"][0][np.repeat(m["computed"], np.diff(np.asarray(case.grid.esup_ptr)))] > 0)


def test_restatement_is_near_the_80_bit_model(case):
    ex, re = case.model(), case.model(np.float64)
    dg, dn = D.dist(re["grad"][0], ex["grad"][0], ex["scale"][0]), D.dist(re["node_values"][0], ex["node_values"][0], ex["scale_node"][0])
    print(f"{case.name}: float64 restatement from the 80-bit model: grad {dg:.2e}, node values {dn:.2e}")
    assert dg <= D.CASE_CAP and dn <= D.CASE_CAP


@pytest.mark.parametrize("mutant", GG.MUTANTS)
def test_mutants_are_told_apart(case, mutant):
    ex, mu = case.model(), case.model(LD, mutant)
    d = D.dist(mu["grad"][0], ex["grad"][0], ex["scale"][0])
    defect = case.defect(mu)
    print(f"{case.name}, {mutant}: distance from the model {d:.2e} of the scale, normal-equation defect {defect:.2e}")
    assert d > 1e-3 and defect > 1e3 * NORMAL_EQUATIONS_CAP


@pytest.mark.parametrize("name", sorted(LINEAR_MESHES))
def test_linear_exactness(name, oracle_lib):
    o, perm, dmag, flag, beta, u, room = linear_case(oracle_lib, name)
    g = o.grid
    ex = GG.corner_gradients(g, perm, dmag, flag, u, LD, room=room)
    re = GG.corner_gradients(g, perm, dmag, flag, u, np.float64)
    err_g, err_n, allowed_g, allowed_n = linear_errors(g, ex, ex, beta)
    computed = ex["computed"]
    interior = np.asarray(g.boundary_points).astype(np.int64) == 0
    assert computed.any() and np.array_equal(computed, interior)
    print(f"{name}: 80-bit model from beta: {float((err_g / allowed_g).max()):.2e} of the inputs' room; node values {float((err_n / allowed_n).max()):.2e}")
    assert np.all(err_g <= allowed_g) and np.all(err_n <= allowed_n)
    # the restatement: the room of the inputs plus its own distance from the 80-bit model, which the cap bounds
    d = D.dist(re["grad"][0], ex["grad"][0], ex["scale"][0])
    err_r = linear_errors(g, re, ex, beta)[0]
    assert d <= D.CASE_CAP and np.all(err_r <= allowed_g + d * ex["scale"][0][np.repeat(computed, np.diff(np.asarray(g.esup_ptr)))])


def linear_case(oracle_lib, name):
    """one block of the LIN tensor (homogeneous, anisotropic), every boundary node Dirichlet, u = A0 + BETA . x at the centroids"""
    mesh = M.attach_fields(LINEAR_MESHES[name](), "u", perm="LIN", neumann_plane=None, seed=3)
    o = oracle_lib.OracleInterpolator("port", threads=2)
    o.load_mesh(mesh)
    v2i = o.variable_to_index
    E, P = o.grid.n_elems, o.grid.n_points
    perm = np.array(o.cells_data[v2i["cells"]["permeability"]][:E * 9]).reshape(E, 9)
    dmag = np.array(o.cells_data[v2i["cells"]["diff_mag"]][:E])
    flag = np.array(o.points_data[v2i["points"]["neumann_flag_u"]][:P]).astype(np.int64)
    assert not flag.any() and np.all(perm == perm[0]) and not np.allclose(perm[0].reshape(3, 3), np.eye(3) * perm[0, 0])
    u, room = GG.linear_field(o.grid, A0, BETA)
    return o, perm, dmag, flag, np.array(BETA, dtype=LD), u, room


def linear_errors(grid, got, exact, beta):
    """(|g - beta| per entry of the computed rows, |u_p - (A0 + beta . x_p)| per computed node, and what the inputs' rounding allows
    for each: twice the propagated room of the cell values (7 eps64 of |a| + sum |beta_k x_k| per cell) -- the second share covers
    the one rounding the system itself carries, fl(x_c - x_p) in A's cell rows: half a unit of |beta| . |x_c - x_p|, which is below
    half a unit of sum |beta_k| (|x_c| + |x_p|)_k, a seventh of the room of two neighbouring cells)"""
    ptr = np.asarray(grid.esup_ptr)
    on = np.repeat(exact["computed"], np.diff(ptr))
    X = np.asarray(grid.point_coords, dtype=np.float64).reshape(-1, 3).astype(LD)
    want = LD(A0) + X @ beta
    err_g = np.abs(np.asarray(got["grad"][0], dtype=LD) - beta)[on]
    err_n = np.abs(np.asarray(got["node_values"][0], dtype=LD) - want)[exact["computed"]]
    return err_g, err_n, 2 * exact["room_grad"][0][on], 2 * exact["room_node"][0][exact["computed"]]
