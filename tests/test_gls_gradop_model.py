"""The numpy model of the kept corner-gradient operator (tests/gls_gradop_model.py) pinned on the CPU, on the four meshes
of tests/test_gls_gradient_model.py: the operator is built from tests/gls_gradient_model.py's corner gradients of indicator fields, in
float64, and then

  (a) gop_ptr is the exclusive sum of 3 ne^2 and the colouring is proper: no two cells of a colour share a node;
  (b) apply and transposed apply in float64 are inside the summation bound of their 80-bit restatement;
  (c) <G u, v> = <u, G^T v> to that bound: both sides are the same N = sum_p 3 ne_p^2 terms g u v in two orders, each side at most
      (N + 2) u sum |terms| from the exact sum, so they differ by at most twice that;
  (d) GradientOperator.to_scipy()'s assembly (ninpol_amd.gradop.block_csr) equals, on hex_mesh(2), the dense matrix written entry by
      entry from the layout: explicit zeros kept, indices sorted, int64."""
import numpy as np
import pytest

import gls_gradient_model as GG
import gls_gradop_model as GO
from gls_exact import LD
from ninpol_amd import mesh as M
from ninpol_amd.gradop import block_csr
from test_gls_adjoint_model import MESHES, oracle_case

_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _CASES.clear()          # (the oracle's grids go while its library is still loaded)


class Case:
    def __init__(self, oracle_lib, make):
        self.o, self.perm, self.dmag, self.flag, _ = oracle_case(oracle_lib, make)
        g = self.grid = self.o.grid
        self.ptr, self.esup, self.E = np.asarray(g.esup_ptr).astype(np.int64), np.asarray(g.esup).astype(np.int64), int(g.n_elems)
        self.colour = GO.colour_cells(self.ptr, self.esup, self.E)
        fields = GO.indicator_fields(self.colour)
        self.model = GG.corner_gradients(g, self.perm, self.dmag, self.flag, fields, np.float64)
        self.gop = GO.gop_from_fields(self.ptr, self.esup, self.colour, self.model["grad"])
        rng = np.random.default_rng(29)
        self.u = rng.uniform(-1.0, 1.0, (2, self.E))
        self.v = rng.uniform(-1.0, 1.0, (2, int(self.ptr[-1]), 3))


@pytest.fixture(params=sorted(MESHES))
def case(request, oracle_lib):
    if request.param not in _CASES:
        _CASES[request.param] = Case(oracle_lib, MESHES[request.param][0])
    return _CASES[request.param]


def test_layout_and_colouring(case):
    c = case
    ne = np.diff(c.ptr)
    ptr = GO.gop_ptr(c.ptr)
    assert ptr[0] == 0 and np.array_equal(np.diff(ptr), 3 * ne * ne) and ptr.dtype == np.int64 and len(c.gop) == ptr[-1]
    for p in range(len(ne)):
        cols = c.colour[c.esup[c.ptr[p]:c.ptr[p + 1]]]
        assert len(set(cols.tolist())) == len(cols), p
    computed = c.model["computed"]
    assert 0 < computed.sum() < len(ne)
    for p in np.flatnonzero(~computed):                                 # a zero row: zeros in every entry of the block
        assert not c.gop[ptr[p]:ptr[p + 1]].any()
    assert all(np.abs(c.gop[ptr[p]:ptr[p + 1]]).max() > 0 for p in np.flatnonzero(computed))


def test_products_are_inside_the_summation_bound(case):
    c = case
    for got, exact, mag, n in (
            (GO.apply(c.ptr, c.esup, c.gop, c.u), GO.apply(c.ptr, c.esup, c.gop, c.u, LD), GO.apply(c.ptr, c.esup, c.gop, c.u, LD, True),
             GO.apply_terms(c.ptr)[None]),
            (GO.apply_transpose(c.ptr, c.esup, c.gop, c.v, c.E), GO.apply_transpose(c.ptr, c.esup, c.gop, c.v, c.E, LD),
             GO.apply_transpose(c.ptr, c.esup, c.gop, c.v, c.E, LD, True), GO.transpose_terms(c.ptr, c.esup, c.E)[None])):
        bar = (n + 2) * LD(GO.U64) * mag
        assert np.count_nonzero(exact) > 0 and np.all(np.abs(got.astype(LD) - exact) <= bar)


def test_duality(case):
    c = case
    Gu = GO.apply(c.ptr, c.esup, c.gop, c.u)                            # [2][nnz][3]
    Gtv = GO.apply_transpose(c.ptr, c.esup, c.gop, c.v, c.E)            # [2][E]
    N = int(GO.gop_ptr(c.ptr)[-1])
    mag = GO.apply(c.ptr, c.esup, c.gop, np.abs(c.u), LD, True)         # sum_j |g| |u| per entry
    for f in range(2):
        lhs = float(np.sum(Gu[f].astype(LD) * c.v[f].astype(LD)))
        rhs = float(np.sum(Gtv[f].astype(LD) * c.u[f].astype(LD)))
        room = 2 * (N + 2) * GO.U64 * float(np.sum(mag[f] * np.abs(c.v[f]).astype(LD)))
        print(f"duality gap {abs(lhs - rhs):.2e}, room {room:.2e}")
        assert lhs != 0 and abs(lhs - rhs) <= room


def test_to_scipy_assembly_against_the_dense_matrix(oracle_lib):
    c = Case(oracle_lib, lambda: M.hex_mesh(2, jitter=0.1, seed=1))
    A = block_csr(c.ptr, c.esup, GO.gop_ptr(c.ptr), c.gop, c.E)
    want = GO.dense(c.ptr, c.esup, c.gop, c.E)
    assert A.shape == (3 * int(c.ptr[-1]), c.E) == want.shape and np.count_nonzero(want) > 0
    assert np.array_equal(A.toarray(), want)
    ne = np.diff(c.ptr)
    assert A.nnz == int((3 * ne * ne).sum()) and A.indices.dtype == np.int64 and A.indptr.dtype == np.int64       # explicit zeros kept
    assert np.count_nonzero(A.data) < A.nnz                             # (the Dirichlet nodes' blocks are those zeros)
    for r in range(A.shape[0]):
        assert np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0)
    x = np.random.default_rng(3).uniform(-1, 1, c.E)
    np.testing.assert_allclose(A @ x, GO.apply(c.ptr, c.esup, c.gop, x).reshape(-1), rtol=0, atol=1e-12 * np.abs(want).max())
