"""The GLS Jacobian in the node coordinates assembled as a block-CSR matrix on the device: GlsShapeJacobian.pattern /
fetch_pattern / launch_assemble / fetch_assembled, PointsJacobian.assemble and Linearization.assemble, held to the numpy model of
tests/gls_shape_assembly_model.py (which tests/test_gls_shape_assembly_model.py pins on the CPU) and, end to end, to the 80-bit models
the two products of the kept Jacobian are held to.

The cases are tests/test_gpu_gls_shape_jacobian.get_case's -- the four small meshes, the Neumann plane z = 0, the ALH tensor -- so the
80-bit models are made once per session.  Every output buffer is NaN-filled before a launch.

The bars, on the models' own scales:

    values:           dist(device, 80-bit assembly of the device's own fetched records)
                          <= max(util.GLS_EXACT_SLACK_CAP x dist(float64 assembly model, 80-bit), ADJOINT_RTOL)   per block entry, on the
                      sum of the absolute contributions carried through the chain
    A @ dX, A.T @ v:  the bars of launch_jvp / launch_vjp (tests/test_gpu_gls_shape_jacobian.jvp_bar / vjp_bar)

The slack and the floor are the ones the project already holds this same geometry chain to (the shape adjoint's gather); nothing in a
bar is measured on the code under test.  Measured on an MI355X: see DESIGN.md 4.19."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the child process of test_forced_slow_symbolic_pass: the paths tests/conftest.py sets up
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import gls_derivative_exact as D  # noqa: E402
import gls_shape_assembly_model as AM  # noqa: E402
import test_gpu_gls_shape_jacobian as SJ  # noqa: E402
from test_gpu_gls_tangent import ADJOINT_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

SLACK = SJ.SLACK
HELD = SJ.HELD
FORCE_SLOW = "NIN_GLS_XJAC_PATTERN_FORCE_SLOW"


def _torch():
    import torch
    return torch


@pytest.fixture(params=sorted(SJ.MESHES))
def case(request):
    return SJ.get_case(request.param)


def model_pattern(c):
    if "assembly_pattern" not in c._models:
        c._models["assembly_pattern"] = AM.pattern(c.grid, c.inpoel, c.inpofa)
    return c._models["assembly_pattern"]


def normals(c):
    return np.asarray(c.grid.normal_faces, dtype=np.float64).reshape(-1, 3)


def assembled(c, J):
    """values (n_blocks, 3) from launch_assemble into a NaN-filled buffer"""
    torch = _torch()
    n = J.pattern(c.stream())[0]
    out = torch.full((n, 3), float("nan"), dtype=torch.float64, device=c.dev)
    J.launch_assemble(out.data_ptr(), c.stream())
    torch.cuda.synchronize(c.dev)
    return out.cpu().numpy()


def block_rows(c):
    bp = model_pattern(c)[0]
    return np.repeat(np.arange(c.P), np.diff(bp))


# ---- 1. the pattern -----------------------------------------------------------------------------------------------------------------------

def test_pattern_is_the_models_before_any_linearisation(case):
    from ninpol_amd.interpolator import GlsShapeJacobian
    c = case
    bp, bc = model_pattern(c)
    raw = GlsShapeJacobian(c.grid)                     # never linearised
    before = raw.nbytes
    got_ptr, got_col = raw.fetch_pattern()
    assert got_ptr.dtype == np.int64 and got_col.dtype == np.int32
    assert got_ptr.tobytes() == bp.tobytes() and got_col.tobytes() == bc.tobytes()
    n, p1, p2 = raw.pattern()
    assert n == len(bc) and p1 and p2 and raw.pattern() == (n, p1, p2)           # the object's own arrays, made once
    assert raw.nbytes == before + 8 * (c.P + 1) + 4 * n and raw.stamp == (-1, -1, -1)
    # copied device-to-device into torch's buffers
    torch = _torch()
    tp = torch.full((c.P + 1,), -7, dtype=torch.int64, device=c.dev)
    tc = torch.full((n,), -7, dtype=torch.int32, device=c.dev)
    raw.launch_pattern_copy(tp.data_ptr(), tc.data_ptr(), c.stream())
    torch.cuda.synchronize(c.dev)
    assert tp.cpu().numpy().tobytes() == bp.tobytes() and tc.cpu().numpy().tobytes() == bc.tobytes()
    raw.release()
    # the linearised objects of the session hold the same pattern
    J = c.jac(True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(J.fetch_pattern(), (bp, bc)))


# ---- 2. the values against the model on the device's own records --------------------------------------------------------------------------

def test_values_against_the_model_on_the_fetched_records(case):
    """the object linearised with neumann values (the chain does not know where the records came from; the object without them is held
    end to end below)"""
    c = case
    J = c.jac(True)
    got = assembled(c, J)
    cell, face, own = J.fetch()
    args = (cell, face, own, c.grid, c.coords, normals(c), c.inpoel, c.inpofa)
    (ex, scale), (re, _) = AM.assemble(*args, D.LD), AM.assemble(*args, np.float64)
    assert got.shape == ex.shape and np.all(np.isfinite(got))                  # every entry written, none left NaN
    d_ref, d_dev = D.dist(re, ex, scale), D.dist(got, ex, scale)
    bar = max(SLACK * d_ref, ADJOINT_RTOL)
    print(f"{c.name}: assembled values, float64 model {d_ref:.2e}, device {d_dev:.2e}, bar {bar:.2e}{'' if d_dev <= bar else '  MISSED'}; "
          f"max |value| {np.abs(got).max():.3e}")
    assert np.abs(got).max() > 0 and d_dev <= bar
    assert got.tobytes() == J.fetch_assembled().tobytes()                       # the host entry point: the same bytes


# ---- 3. end to end: the scipy matrix against the models of the two products --------------------------------------------------------------

def test_assembled_matrix_against_the_models_of_the_products(case):
    import scipy.sparse as sp
    c = case
    (jex, vex), (jre, vre) = c.jacobian_models(D.LD), c.jacobian_models(np.float64)
    bp, bc = model_pattern(c)
    ok = []
    for i, with_b in enumerate((True, False)):
        op = c.I.points_jacobian("u", c.u, c.b if with_b else None)
        A = op.assemble()
        assert sp.isspmatrix_csr(A) and A.shape == (c.P, 3 * c.P) and A.dtype == np.float64 and A.nnz == 3 * len(bc)
        assert A.indices.dtype == np.int64 and A.indptr.dtype == np.int64 and A.has_sorted_indices
        assert np.array_equal(A.indptr, 3 * bp) and np.array_equal(A.indices, (3 * bc.astype(np.int64)[:, None] + np.arange(3)).reshape(-1))
        assert np.all(np.diff(A.indices)[np.setdiff1d(np.arange(A.nnz - 1), A.indptr[1:-1] - 1)] > 0)      # sorted within every row
        assert A.data.tobytes() == assembled(c, c.jac(with_b)).tobytes()            # the kept object of the session: the same bytes
        for k, t in enumerate(HELD):
            tag = f"{c.name} assemble() neumann_values={'given' if with_b else 'none'}, direction {t}"
            ok.append(SJ.jvp_bar(tag, A @ c.dXs[t].reshape(-1), jex[i][k], jre[i][k])[0])
            ok.append(SJ.vjp_bar(tag, (A.T @ c.vs[t]).reshape(c.P, 3), vex[i][k], vre[i][k])[0])
        op.release()
    assert all(ok), c.name


# ---- 4. exact properties ------------------------------------------------------------------------------------------------------------------

def test_exact_properties(case):
    c = case
    J = c.jac(True)
    vals = assembled(c, J)
    rows = block_rows(c)
    # the rows the forward gives as zero hold exact zeros, the Dirichlet nodes among them; their blocks are in the pattern
    own = J.fetch()[2]
    zero = ~(np.abs(own).max(axis=1) > 0)
    dirichlet = (np.asarray(c.grid.boundary_points).astype(np.int64) != 0) & (c.flag == 0)
    assert dirichlet.any() and zero[dirichlet].all() and not zero.all()
    assert zero[rows].any() and not vals[zero[rows]].any() and np.abs(vals[~zero[rows]]).max() > 0
    # two calls agree bit for bit
    assert assembled(c, J).tobytes() == vals.tobytes()
    # 2 u gives exactly twice (without neumann values: with them F = W u + nws b is affine in u)
    twice = c.linearize(False, 2.0 * c.u)
    assert assembled(c, twice).tobytes() == (2.0 * assembled(c, c.jac(False))).tobytes()
    twice.release()
    # relinearize(u2): the values of a fresh object linearised at u2, the pattern where it was
    u2 = np.random.default_rng(31).uniform(-1.0, 1.0, c.E)
    fresh, moved = c.linearize(True, u2), c.linearize(True)
    pat = moved.pattern()
    at_u = assembled(c, moved)
    assert at_u.tobytes() == vals.tobytes()
    ud, bd = c.to_dev(u2), c.to_dev(c.b)
    moved.relinearize(ud.data_ptr(), bd.data_ptr(), c.stream())
    _torch().cuda.synchronize(c.dev)
    at_u2 = assembled(c, moved)
    assert at_u2.tobytes() == assembled(c, fresh).tobytes() and at_u2.tobytes() != at_u.tobytes() and moved.pattern() == pat
    fresh.release()
    moved.release()
    with pytest.raises(ValueError, match="released"):
        moved.launch_assemble(8)


def _digest(c, J):
    bp, bc = J.fetch_pattern()
    return hashlib.sha256(bp.tobytes() + bc.tobytes() + assembled(c, J).tobytes()).hexdigest()


def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    assert os.environ.get(FORCE_SLOW)
    c = SJ.get_case("delaunay")
    bp, bc = AM.pattern(c.grid, c.inpoel, c.inpofa)
    J = c.jac(True)
    got = J.fetch_pattern()
    assert got[0].tobytes() == bp.tobytes() and got[1].tobytes() == bc.tobytes()
    print("DIGEST", _digest(c, J))
    print("CHILD OK")


def test_forced_slow_symbolic_pass():
    """the Delaunay mesh again with every row through the symbolic pass's slow path, in a fresh child process (the switch is read when
    the pattern is made): the default's bytes, pattern and values"""
    c = SJ.get_case("delaunay")
    assert FORCE_SLOW not in os.environ
    want = _digest(c, c.jac(True))
    env = dict(os.environ, **{FORCE_SLOW: "1"})
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout
    assert f"DIGEST {want}" in r.stdout


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------------

def test_state():
    torch = _torch()
    from ninpol_amd import _lib
    from ninpol_amd.interpolator import GlsShapeJacobian
    c = SJ.Case("mixed")                       # its own Interpolator: the resident tables and the mesh are rewritten
    bp, bc = AM.pattern(c.grid, c.inpoel, c.inpofa)
    n = len(bc)
    buf = torch.full((n, 3), float("nan"), dtype=torch.float64, device=c.dev)
    # before the first linearisation: refused, nothing written, no pattern made
    raw = GlsShapeJacobian(c.grid)
    with pytest.raises(_lib.NinpolError) as e:
        raw.launch_assemble(buf.data_ptr(), c.stream())
    assert e.value.code == _lib.NIN_ESTATE and "nin_gls_xjacobian_linearize" in e.value.text
    torch.cuda.synchronize(c.dev)
    assert torch.isnan(buf).all() and raw.nbytes == c.record_bytes()
    raw.release()
    # nbytes grows by the pattern at the first pattern(), and not before
    J = c.linearize(True)
    assert J.nbytes == c.record_bytes()
    pat = J.pattern(c.stream())
    assert pat[0] == n and J.nbytes == c.record_bytes() + 8 * (c.P + 1) + 4 * n
    vals = assembled(c, J)
    assert J.nbytes == c.record_bytes() + 8 * (c.P + 1) + 4 * n and np.all(np.isfinite(vals))
    # updates of the permeability and the flags are not refused: the same bytes
    K2 = c.perm * np.random.default_rng(7).uniform(1.5, 2.5, (c.E, 1))
    c.I.update_permeability(c.to_dev(K2.reshape(c.E, 3, 3)))
    flags = c.flag.astype(np.float64)
    flags[np.flatnonzero(c.flag)[::2]] = 0.0
    c.I.update_neumann_flags("u", c.to_dev(flags))
    torch.cuda.synchronize(c.dev)
    assert not J.is_current() and assembled(c, J).tobytes() == vals.tobytes()
    # an update of the points: refused in the words of the products, nothing written; the pattern stays, the same arrays and bytes
    c.I.update_points(c.coords + np.random.default_rng(11).uniform(-1e-3, 1e-3, (c.P, 3)))
    with pytest.raises(RuntimeError, match="nin_gls_xjacobian_linearize again") as e:
        J.launch_assemble(buf.data_ptr(), c.stream())
    assert isinstance(e.value, _lib.NinpolError) and e.value.code == _lib.NIN_ESTATE and "geometry_updates" in e.value.text
    host = np.full((n, 3), np.nan)
    assert _lib.load().nin_gls_xjacobian_assemble_host(J._handle(), _lib._ptr(host)) == _lib.NIN_ESTATE
    torch.cuda.synchronize(c.dev)
    assert torch.isnan(buf).all() and np.isnan(host).all()
    assert J.pattern(c.stream()) == pat and all(a.tobytes() == b.tobytes() for a, b in zip(J.fetch_pattern(), (bp, bc)))
    # relinearize at the new point: it answers again, as a fresh object does
    ud, bd = c.to_dev(c.u), c.to_dev(c.b)
    J.relinearize(ud.data_ptr(), bd.data_ptr(), c.stream())
    fresh = c.linearize(True)
    moved = assembled(c, J)
    assert moved.tobytes() == assembled(c, fresh).tobytes() and moved.tobytes() != vals.tobytes() and J.pattern(c.stream()) == pat
    # the scratch of the grid goes (the connectivity on the device with it) and the object still answers
    c.grid.release_scratch()
    assert assembled(c, J).tobytes() == moved.tobytes()
    fresh.release()
    J.release()


# ---- 6. torch -----------------------------------------------------------------------------------------------------------------------------

def test_linearization_assemble():
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    shared = SJ.get_case("mixed")              # the models: the same mesh, u and directions
    c = SJ.Case("mixed")                       # its own Interpolator: the op rewrites the resident coordinates
    jex, jre = shared.jvp_models(D.LD), shared.jvp_models(np.float64)
    op = CellToNode(c.I, "u", "gls")
    u0, X0 = c.to_dev(c.u), c.to_dev(c.coords)          # the resident coordinates themselves: the models above are at this point
    lin = op.linearize(u0, points=X0, wrt="points")
    assert np.array_equal(np.asarray(c.grid.point_coords).reshape(-1, 3), shared.coords)
    A = lin.assemble()
    assert A.layout == torch.sparse_csr and A.device == c.dev and A.dtype == torch.float64 and tuple(A.shape) == (c.P, 3 * c.P)
    sop = c.I.points_jacobian("u", c.u)
    S = sop.assemble()
    sop.release()
    assert np.array_equal(A.crow_indices().cpu().numpy(), S.indptr) and np.array_equal(A.col_indices().cpu().numpy(), S.indices)
    assert A.values().cpu().numpy().tobytes() == S.data.tobytes()
    ok = []
    for k, t in enumerate(HELD):
        dX = c.to_dev(c.dXs[t])
        got = torch.sparse.mm(A, dX.reshape(-1, 1)).reshape(-1).cpu().numpy()
        good, bar = SJ.jvp_bar(f"Linearization.assemble(), direction {t}", got, jex[1][k], jre[1][k])
        d = D.dist(got, lin.jvp(dpoints=dX).cpu().numpy(), jex[1][k]["scale"])
        print(f"    torch.sparse.mm(A, dX) against lin.jvp(dpoints=dX): {d:.2e} of the row scale, bar {bar:.2e}")
        ok.append(good and d <= bar)
    assert all(ok)
    for wrt in ("K", "scale"):
        K0 = c.to_dev(c.perm.reshape(c.E, 3, 3))
        other = op.linearize(u0, K=K0, scale=torch.ones(c.E, dtype=torch.float64, device=c.dev), wrt=wrt)
        with pytest.raises(ValueError, match='wrt="points"'):
            other.assemble()
        other.release()
    c.I.update_points(c.coords)
    with pytest.raises(RuntimeError, match="linearize again"):
        lin.assemble()
    lin.release()
    torch.cuda.synchronize(c.dev)


if __name__ == "__main__":
    _child()
