"""The numpy model of the assembled GLS Jacobian in the node coordinates (tests/gls_shape_assembly_model.py) pinned on
the CPU, on the four meshes the device tests use (tests/test_gpu_gls_shape_adjoint.MESHES: the same constructors as
tests/test_gls_adjoint_model.MESHES -- jittered hexahedra, tetrahedra, a mixed mesh, a random-cloud Delaunay mesh), with RANDOM records
in [-1, 1]: the chain from the records to the blocks is linear in them, so where they came from does not matter.

  (a) A . dX equals  sum_row cell . dC + sum_row (face . (dFc, dN)) + own . dx  with the geometry tangents of the shape tangent's model
      (STM.geometry_tangents), and
  (b) A^T . v equals the gather of the shape adjoint's model (tests/gls_shape_model.py, "the geometry chain": the records of every node
      times v_p summed per cell and per face, then the chain once per face) -- both in 80 bits, to 1000 x finfo(longdouble).eps of the
      absolute-sum scale the assembly model carries per block.  The longest sum has about 130 terms, so this is an order above
      worst-case rounding and far below any error of a formula;
  (c) the pattern: ascending and unique, row p contains p, equal to the set definition computed with Python sets, 2197 / 1243 / 7861
      blocks on the hexahedron / mixed / Delaunay mesh; the Delaunay mesh has a row of more than 128 candidates and no row of more than
      32 columns, so the deduplication is exercised."""
import numpy as np
import pytest

import gls_shape_assembly_model as AM
import gls_shape_model as SM
import gls_shape_tangent_model as STM
from gls_exact import LD
from test_gls_adjoint_model import MESHES, oracle_case

RTOL = 1000 * float(np.finfo(LD).eps)
N_BLOCKS = {"hex": 2197, "mixed": 1243, "delaunay": 7861}


class Case:
    def __init__(self, name, oracle_lib):
        self.name = name
        self.o = oracle_case(oracle_lib, MESHES[name][0])[0]
        g = self.grid = self.o.grid
        self.coords = np.array(g.point_coords, dtype=np.float64).reshape(-1, 3)
        self.normals = np.array(g.normal_faces, dtype=np.float64).reshape(-1, 3)
        self.P = len(self.coords)
        self.eptr, self.esup, self.fptr, self.fsup = AM._rows(g)
        rng = np.random.default_rng(53)
        self.cell, self.face = rng.uniform(-1.0, 1.0, (len(self.esup), 3)), rng.uniform(-1.0, 1.0, (len(self.fsup), 6))
        self.own = rng.uniform(-1.0, 1.0, (self.P, 3))
        self.dX, self.v = rng.uniform(-1.0, 1.0, (self.P, 3)), rng.uniform(-1.0, 1.0, self.P)
        self.block_ptr, self.block_col = AM.pattern(g, g.inpoel, g.inpofa)
        self.values, self.scale = AM.assemble(self.cell, self.face, self.own, g, self.coords, self.normals, g.inpoel, g.inpofa, LD)
        self.rows = np.repeat(np.arange(self.P), np.diff(self.block_ptr))


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


def test_pattern(case):
    c = case
    g = c.grid
    assert c.block_ptr.dtype == np.int64 and c.block_col.dtype == np.int32 and c.block_ptr[0] == 0 and c.block_ptr[-1] == len(c.block_col)
    cpts, fpts = SM.cell_points(g.inpoel), SM.face_points(g.inpofa)
    for p in range(c.P):
        cols = c.block_col[c.block_ptr[p]:c.block_ptr[p + 1]].astype(np.int64)
        assert np.all(np.diff(cols) > 0) and p in cols                         # ascending, unique, the node itself
        want = {p}
        for e in c.esup[c.eptr[p]:c.eptr[p + 1]]:
            want |= {int(q) for q in cpts[e]}
        for f in c.fsup[c.fptr[p]:c.fptr[p + 1]]:
            want |= {int(q) for q in fpts[f]}
        assert set(cols.tolist()) == want, p
    n_cand = np.array([len(x) for x in AM.candidates(g, g.inpoel, g.inpofa)])
    n_cols = np.diff(c.block_ptr)
    print(f"{c.name}: P = {c.P}, n_blocks = {len(c.block_col)}, candidates per row <= {n_cand.max()}, columns per row <= {n_cols.max()}")
    if c.name in N_BLOCKS:
        assert len(c.block_col) == N_BLOCKS[c.name]
    if c.name == "delaunay":
        assert n_cand.max() > 128 and n_cols.max() <= 32


def test_matrix_times_direction_is_the_records_times_the_geometry_tangents(case):
    c = case
    g = c.grid
    dX = c.dX.astype(LD)
    dC, dFc, dN = STM.geometry_tangents(g, g.inpoel, g.inpofa, c.dX, LD)
    cell, face, own = c.cell.astype(LD), c.face.astype(LD), c.own.astype(LD)
    want = (own * dX).sum(axis=1)
    np.add.at(want, np.repeat(np.arange(c.P), np.diff(c.eptr)), (cell * dC[c.esup]).sum(axis=1))
    np.add.at(want, np.repeat(np.arange(c.P), np.diff(c.fptr)), (face[:, :3] * dFc[c.fsup]).sum(axis=1) + (face[:, 3:] * dN[c.fsup]).sum(axis=1))
    cols = c.block_col.astype(np.int64)
    got, room = np.zeros(c.P, dtype=LD), np.zeros(c.P, dtype=LD)
    np.add.at(got, c.rows, (c.values * dX[cols]).sum(axis=1))
    np.add.at(room, c.rows, (c.scale * np.abs(dX[cols])).sum(axis=1))
    err = float((np.abs(got - want) / room).max())
    print(f"{c.name}: max |A dX - records . geometry tangents| / scale = {err:.2e} (bar {RTOL:.2e}); max |A dX| = {float(np.abs(got).max()):.3e}")
    assert np.all(room > 0) and np.abs(got).max() > 0 and err <= RTOL


def test_transpose_times_field_is_the_adjoint_models_gather(case):
    c = case
    g = c.grid
    v = c.v.astype(LD)
    X, Nres = c.coords.astype(LD), c.normals.astype(LD)
    E, F = len(SM.cell_points(g.inpoel)), len(c.normals)
    # the records of every node times v_p, summed per cell and per face ...
    Cb, Fb, Nb = np.zeros((E, 3), dtype=LD), np.zeros((F, 3), dtype=LD), np.zeros((F, 3), dtype=LD)
    vc, vf = v[np.repeat(np.arange(c.P), np.diff(c.eptr))], v[np.repeat(np.arange(c.P), np.diff(c.fptr))]
    np.add.at(Cb, c.esup, vc[:, None] * c.cell.astype(LD))
    np.add.at(Fb, c.fsup, vf[:, None] * c.face[:, :3].astype(LD))
    np.add.at(Nb, c.fsup, vf[:, None] * c.face[:, 3:].astype(LD))
    # ... then gls_shape_model's geometry chain, once per cell and per face
    want = v[:, None] * c.own.astype(LD)
    for e, pts in enumerate(SM.cell_points(g.inpoel)):
        want[pts] += Cb[e] / len(pts)
    for f, pts in enumerate(SM.face_points(g.inpofa)):
        want[pts] += Fb[f] / len(pts)
        v1, v2 = X[pts[0]] - X[pts[1]], X[pts[2]] - X[pts[1]]
        n = np.cross(v1, v2)
        nbar = (Nb[f] - (Nb[f] @ Nres[f]) * Nres[f]) / np.sqrt(n @ n)
        v1b, v2b = np.cross(v2, nbar), np.cross(nbar, v1)
        want[pts[0]] += v1b
        want[pts[2]] += v2b
        want[pts[1]] -= v1b + v2b
    cols = c.block_col.astype(np.int64)
    got, room = np.zeros((c.P, 3), dtype=LD), np.zeros((c.P, 3), dtype=LD)
    np.add.at(got, cols, v[c.rows][:, None] * c.values)
    np.add.at(room, cols, np.abs(v[c.rows])[:, None] * c.scale)
    err = float((np.abs(got - want) / room).max())
    print(f"{c.name}: max |A^T v - gather| / scale = {err:.2e} (bar {RTOL:.2e}); max |A^T v| = {float(np.abs(got).max()):.3e}")
    assert np.all(room > 0) and np.abs(got).max() > 0 and err <= RTOL


def test_the_float64_model_is_the_80_bit_model_to_rounding(case):
    c = case
    g = c.grid
    v64, s64 = AM.assemble(c.cell, c.face, c.own, g, c.coords, c.normals, g.inpoel, g.inpofa, np.float64)
    assert v64.dtype == np.float64 and np.all(np.isfinite(v64))
    err = float((np.abs(v64 - c.values) / c.scale).max())
    print(f"{c.name}: float64 model against the 80-bit model: {err:.2e} of the block scale")
    assert err <= 100 * np.finfo(np.float64).eps            # a block sums at most about 60 records' terms of at most a dozen operations
