"""The numpy model of the GLS Jacobian in the node coordinates (tests/gls_shape_jacobian_model.py) pinned on the CPU, on the four meshes
of tests/test_gls_shape_tangent_model.py (jittered hexahedra, tetrahedra, a mixed mesh and a random-cloud Delaunay mesh), ALH tensor,
Neumann plane z = 0, a random cell field u and random node values b:

  (a) J . dX against the central difference of the smooth forward's  W u + nws . b  (SM.smooth_bag: the geometry recomputed in float64
      from X +- h dX, h = 1e-6, the difference's own h^2 term taken out with the step 2h: (4 D(h) - D(2h)) / 3) along a random dX:
      FD_RTOL = 1e-8 of max |J . dX| -- the bar and the method of the shape tangent's check (a);
  (b) <v, J . dX> = <J^T v, dX> in 80 bits, with and without b: DUALITY_RTOL = 1e-12 of sum |J^T v . dX| -- the two products come from
      two derivations that share the assembly and the QR, and nothing after it;
  (c) the zero rows of the forward are zero rows of J, and a Dirichlet node has a non-zero column: it moves the rows of its neighbours.

Measured: DESIGN.md 4.18."""
import numpy as np
import pytest

import gls_derivative_exact as D
import gls_shape_jacobian_model as JM
import test_gls_shape_tangent_model as STT
from test_gls_adjoint_model import FD_RTOL, MESHES
from test_gls_tangent_model import DUALITY_RTOL

assert FD_RTOL == 1e-8 and DUALITY_RTOL == 1e-12          # the two bars the shape tangent's checks (a) and (b) use


class Case(STT.Case):
    """STT.Case (the oracle's grid and tables, the random direction dX, the smooth bag and its central differences) with a cell field,
    node values and a node field"""

    def __init__(self, name, oracle_lib):
        super().__init__(name, oracle_lib)
        rng = np.random.default_rng(41)
        E = len(np.asarray(self.grid.centroids).reshape(-1, 3))
        self.u, self.b, self.v = rng.uniform(-1.0, 1.0, E), rng.uniform(-1.0, 1.0, self.P), rng.uniform(-1.0, 1.0, self.P)

    def args(self, grid=None):
        g = self.grid
        return (grid or g, self.perm, self.dmag, self.flag, g.inpoel, g.inpofa)


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()          # (the oracle's grids go while its library is still loaded)


@pytest.fixture(params=sorted(MESHES))
def case(request, oracle_lib):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param, oracle_lib)
    return _CASES[request.param]


def test_jvp_is_the_central_difference_of_the_smooth_forward(case):
    c = case
    ptr, esup, rows = D._rows(c.grid)
    got = JM.jvp_models(*c.args(c.bag), c.u, [c.b], [c.dX], np.float64)[0][0]["value"]
    top = np.abs(got).max()
    errs = {}
    for which in ("plain", "extrapolated"):
        fd_w, fd_n = c.fd()[which]
        fd = np.bincount(rows, weights=fd_w * c.u[esup], minlength=c.P) + fd_n * c.b
        errs[which] = np.abs(fd - got).max() / top
    print(f"{c.name}: max|FD - J.dX| / max|J.dX| = {errs['extrapolated']:.2e}; the plain difference at h = {STT.H_SMOOTH}: {errs['plain']:.2e}; "
          f"max|J.dX| = {top:.3e}")
    assert top > 0 and errs["extrapolated"] <= FD_RTOL


def test_duality_in_80_bits(case):
    c = case
    dX, v = c.dX.astype(D.LD), c.v.astype(D.LD)
    bs = (c.b, None)
    jvs, gxs = JM.jvp_models(*c.args(), c.u, bs, [c.dX], D.LD), JM.vjp_models(*c.args(), c.u, bs, [c.v], D.LD)
    for b, (jv,), (gx,) in zip(bs, jvs, gxs):
        terms = gx["grad_points"] * dX
        room = np.abs(terms).sum()
        gap = float(abs(v @ jv["value"] - terms.sum()) / room)
        print(f"{c.name}, b {'given' if b is not None else 'none'}: 80-bit duality gap {gap:.2e} of sum|J^T v . dX|")
        assert room > 0 and gap <= DUALITY_RTOL
        # (c): zero rows stay zero; a Dirichlet node is not computed but has a column
        zero = ~jv["computed"]
        assert zero.any() and not jv["value"][zero].any() and not jv["scale"][zero].any()
        assert c.dirichlet.any() and zero[c.dirichlet].all() and np.abs(gx["grad_points"][c.dirichlet]).max() > 0
    # b really enters
    with_b, without = jvs[0][0]["value"], jvs[1][0]["value"]
    assert np.abs(with_b - without).max() > 1e-6 * np.abs(with_b).max()
