"""The numpy model of the GLS shape tangent (tests/gls_shape_tangent_model.py) pinned on the CPU, on the four meshes of
tests/test_gls_shape_model.py (jittered hexahedra, tetrahedra, a mixed mesh and a random-cloud Delaunay mesh), ALH tensor, Neumann
plane z = 0:

  (a) against central differences of the model's own smooth forward (SM.smooth_bag: the geometry recomputed in float64 from
      X +- h dX, h = 1e-6, the difference's own h^2 term taken out with the step 2h) along a random dX: FD_RTOL of max |dW|;
  (b) against the shape adjoint of tests/gls_shape_model.py in 80 bits, both add_neumann values, with and without ghat_nws:
      |<ghat, dd> + <ghat_nws, dnws> - <Xbar, dX>| <= DUALITY_RTOL sum |Xbar . dX| -- the two derivations share the assembly and the
      QR, and nothing after it;
  (c) four one-line mutants of the model each miss (a) or (b) on a named mesh;
  (d) a rigid translation moves no weight;
  (e) a direction supported on Dirichlet boundary nodes alone moves the rows of their neighbours;
  (f) the float64 restatement is within D.CASE_CAP of the 80-bit model on all four meshes."""
import numpy as np
import pytest

import gls_adjoint_model as GM
import gls_derivative_exact as D
import gls_shape_model as SM
import gls_shape_tangent_model as STM
from test_gls_adjoint_model import FD_RTOL, MESHES, oracle_case
from test_gls_tangent_model import DUALITY_RTOL

H_SMOOTH = 1e-6
TRANSLATION_RTOL = 1e-12
VARIANTS = ((True, True), (True, False), (False, True), (False, False))          # (add_neumann, with ghat_nws)
# where each mutant is seen, and by which check
MUTANT_MESH = {"quad_fourth_vertex": ("hex", "duality"), "normal_projection": ("tet", "duality"), "dtau": ("mixed", "fd"),
               "own_point": ("delaunay", "fd")}
assert sorted(MUTANT_MESH) == sorted(STM.MUTANTS)


class Case:
    """one mesh: the oracle's grid and tables, the directions -- random, one constant vector, random on the Dirichlet nodes alone --
    and the models' answers, one pass over the nodes per format and per grid"""

    def __init__(self, name, oracle_lib):
        self.name = name
        self.o, self.perm, self.dmag, self.flag, _ = oracle_case(oracle_lib, MESHES[name][0])
        g = self.grid = self.o.grid
        self.coords = np.array(g.point_coords, dtype=np.float64).reshape(-1, 3)
        self.P, self.nnz = len(self.coords), len(g.esup)
        self.dirichlet = (np.asarray(g.boundary_points).astype(np.int64) != 0) & (self.flag == 0)
        self.dX = np.random.default_rng(29).uniform(-1.0, 1.0, (self.P, 3))
        self.shift = np.broadcast_to(np.array([1.0, -0.5, 0.25]), (self.P, 3)).copy()
        self.dXd = np.where(self.dirichlet[:, None], np.random.default_rng(31).uniform(-1.0, 1.0, (self.P, 3)), 0.0)
        rng = np.random.default_rng(17)
        self.ghat, self.gnws = rng.uniform(-1.0, 1.0, self.nnz), rng.uniform(-1.0, 1.0, self.P)
        self.bag = SM.smooth_bag(g, self.coords, g.inpoel, g.inpofa)
        self._runs = {}
        self._fd = None

    def tangents(self, dtype, grid=None, mutant=None):
        """[random, translation, Dirichlet] (a mutant: the random direction alone) on the oracle's grid, or on `grid`"""
        key = (dtype, grid is None, mutant)
        if key not in self._runs:
            dirs = [self.dX] if mutant else [self.dX, self.shift, self.dXd]
            self._runs[key] = STM.shape_tangents(grid or self.grid, self.perm, self.dmag, self.flag, self.grid.inpoel, self.grid.inpofa, dirs,
                                                 True, dtype, mutant)
        return self._runs[key]

    def fd(self):
        """{"plain", "extrapolated"}: (d stored weights, d neumann_ws) by central differences of the smooth forward along the random
        direction -- D(h) at h = H_SMOOTH, and (4 D(h) - D(2h)) / 3"""
        if self._fd is None:
            g = self.grid

            def central(h):
                got = []
                for sgn in (+1, -1):
                    m = GM.gls_adjoint_model(SM.smooth_bag(g, self.coords + sgn * h * self.dX, g.inpoel, g.inpofa), self.perm, self.dmag, self.flag)
                    got.append((m["weights"], m["neumann_ws"], m["computed"]))
                assert np.array_equal(got[0][2], got[1][2])
                return (got[0][0] - got[1][0]) / (2 * h), (got[0][1] - got[1][1]) / (2 * h)

            d1, d2 = central(H_SMOOTH), central(2 * H_SMOOTH)
            self._fd = {"plain": d1, "extrapolated": tuple((4 * a - b) / 3 for a, b in zip(d1, d2))}
        return self._fd

    def fd_err(self, mutant=None, which="extrapolated"):
        """max |FD - model| / max |dW| of the float64 model on the smooth bag"""
        fd_w, fd_n = self.fd()[which]
        scale = np.abs(self.tangents(np.float64, self.bag)[0]["tangent"]).max()
        m = self.tangents(np.float64, self.bag, mutant)[0]
        return np.abs(fd_w - m["tangent"]).max() / scale, np.abs(fd_n - m["tangent_neumann_ws"]).max() / scale, scale

    def adjoints(self):
        """the 80-bit shape adjoints of VARIANTS"""
        if "adj" not in self._runs:
            cots = [(self.ghat, self.gnws if nws else None, an) for an, nws in VARIANTS]
            self._runs["adj"] = SM.shape_adjoints(self.grid, self.perm, self.dmag, self.flag, self.grid.inpoel, self.grid.inpofa, cots, D.LD)
        return self._runs["adj"]

    def duality_gaps(self, mutant=None):
        """per variant |<ghat, dd> + <ghat_nws, dnws> - <Xbar, dX>| / sum |Xbar . dX|, in 80 bits"""
        t = self.tangents(D.LD, mutant=mutant)[0]
        gaps = []
        for (an, nws), adj in zip(VARIANTS, self.adjoints()):
            lhs = self.ghat.astype(D.LD) @ (t["tangent"] if an else t["tangent_plain"])
            if nws:
                lhs = lhs + self.gnws.astype(D.LD) @ t["tangent_neumann_ws"]
            terms = adj["grad_points"] * self.dX.astype(D.LD)
            room = np.abs(terms).sum()
            assert room > 0
            gaps.append(float(abs(lhs - terms.sum()) / room))
        return gaps


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()          # (the oracle's grids go while its library is still loaded)


def get(name, oracle_lib):
    if name not in _CASES:
        _CASES[name] = Case(name, oracle_lib)
    return _CASES[name]


@pytest.fixture(params=sorted(MESHES))
def case(request, oracle_lib):
    return get(request.param, oracle_lib)


def test_tangent_is_the_central_difference_of_the_smooth_forward(case):
    """The bar is FD_RTOL of max |dW|.  The reference is the central difference D(h) of the smooth forward at X +- h dX, h = 1e-6, with
    its own h^2 term taken out by the same difference at 2h: (4 D(h) - D(2h)) / 3.  The plain D(h) is printed beside it.  A random dX
    moves every vertex of every cell at once, and on the random-cloud Delaunay mesh the truncation error of the plain difference alone
    is over the bar: 3.70e-7, 9.24e-8, 2.32e-8, 5.81e-9, 1.60e-9 of max |dW| at h = 4e-6, 2e-6, 1e-6, 5e-7, 2.5e-7 -- a factor of four
    per halving, at one and the same entry -- while the extrapolated difference is 1.8e-10 from the model at h = 1e-6.  (The three
    other meshes are under the bar with the plain difference too.)"""
    p_w, p_n, _ = case.fd_err(which="plain")
    e_w, e_n, scale = case.fd_err()
    print(f"{case.name}: max|FD - model| / max|dW| = {e_w:.2e} (weights), {e_n:.2e} (neumann_ws); the plain difference at h = {H_SMOOTH}: "
          f"{p_w:.2e}, {p_n:.2e}; max|dW| = {scale:.3e}")
    assert scale > 0 and e_w <= FD_RTOL and e_n <= FD_RTOL


def test_duality_with_the_shape_adjoint(case):
    gaps = case.duality_gaps()
    print(f"{case.name}: 80-bit duality gaps of sum|Xbar . dX|: " + ", ".join(f"{g:.2e}" for g in gaps))
    assert all(g <= DUALITY_RTOL for g in gaps)
    # the variants really differ: ghat_nws and add_neumann both enter
    a = case.adjoints()
    assert np.abs(a[0]["grad_points"] - a[1]["grad_points"]).max() > 0 and np.abs(a[0]["grad_points"] - a[2]["grad_points"]).max() > 0


@pytest.mark.parametrize("mutant", STM.MUTANTS)
def test_a_mutant_misses_the_bar(mutant, oracle_lib):
    name, check = MUTANT_MESH[mutant]
    c = get(name, oracle_lib)
    if check == "fd":
        e_w, e_n, _ = c.fd_err(mutant)
        print(f"{c.name}: mutant {mutant}: max|FD - model| / max|dW| = {e_w:.2e} (weights), {e_n:.2e} (neumann_ws)")
        assert max(e_w, e_n) > FD_RTOL
    else:
        gaps = c.duality_gaps(mutant)
        print(f"{c.name}: mutant {mutant}: 80-bit duality gaps " + ", ".join(f"{g:.2e}" for g in gaps))
        assert max(gaps) > DUALITY_RTOL


def test_rigid_translation(case):
    """dX = one constant vector: every dv1, dv2 and dT is exactly 0, dC_e - dx_p is 0 up to the rounding of (sum dx) / n_e (it does
    not round-trip on the six points of a wedge), so the tangent is 0 up to that.  Measured on the row scale of the random direction,
    whose entries are as large (|dX| <= 1): the translation's own scale is a scale of rounding errors and measures nothing; a row
    whose own scale is 0 must be exactly 0."""
    for dtype in (np.float64, D.LD):
        rnd, tr, _ = case.tangents(dtype)
        rows = D._rows(case.grid)[2]
        scale = rnd["scale"]
        assert np.all(scale[rnd["computed"]] > 0)
        worst = 0.0
        for key, per in (("tangent", rows), ("tangent_plain", rows), ("tangent_neumann_ws", np.arange(case.P))):
            t = np.abs(tr[key])
            assert not t[tr["scale"][per] == 0].any() and not t[scale[per] == 0].any()
            on = scale[per] > 0
            worst = max(worst, float((t[on] / scale[per][on]).max()))
        print(f"{case.name}: rigid translation, {np.dtype(dtype).name}: max|tangent| / scale = {worst:.2e}")
        assert worst <= TRANSLATION_RTOL


def test_dirichlet_nodes_move_their_neighbours(case):
    """a Dirichlet node has the zero row, but it is a vertex of cells and faces of nodes that have not"""
    m = case.tangents(D.LD)[2]
    assert case.dirichlet.any() and not m["computed"][case.dirichlet].any() and not case.dXd[~case.dirichlet].any()
    ptr = np.asarray(case.grid.esup_ptr)
    moved = [p for p in range(case.P) if np.abs(m["tangent"][ptr[p]:ptr[p + 1]]).max(initial=0) > 0]
    assert moved and m["computed"][moved].all() and not case.dirichlet[moved].any()
    assert np.count_nonzero(m["tangent_neumann_ws"]) > 0
    # the zero rows stay zero, on every direction
    for t in case.tangents(D.LD):
        zero = ~t["computed"]
        assert zero.any() and not t["scale"][zero].any() and not t["tangent"][np.repeat(zero, np.diff(ptr))].any()


def test_restatement_is_within_the_case_cap(case):
    exact, restated = case.tangents(D.LD), case.tangents(np.float64)
    for tag, ex, re in zip(("random", "translation", "dirichlet"), exact, restated):
        if tag == "translation":
            continue                                    # (its scale is one of rounding errors: test_rigid_translation)
        for an in (True, False):
            key = "tangent" if an else "tangent_plain"
            d = D.tangent_dist(case.grid, re[key], re["tangent_neumann_ws"], dict(ex, tangent=ex[key]))
            print(f"{case.name}: {tag} direction, add_neumann={an}: float64 restatement {d:.2e} from the 80-bit model")
            assert d <= D.CASE_CAP
