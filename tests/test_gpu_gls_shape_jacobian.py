"""The GLS Jacobian in the node coordinates kept on the device: DevicePlan.linearize_points, GlsShapeJacobian.launch_jvp
/ launch_vjp, Interpolator.points_jacobian and CellToNode.linearize(wrt="points"), held to the 80-bit model of
tests/gls_shape_jacobian_model.py (which tests/test_gls_shape_jacobian_model.py pins against central differences of its own smooth
forward and against its own transpose).

The meshes, the Neumann plane z = 0 and the ALH tensor are those of tests/test_gpu_gls_shape_adjoint.py; the random-cloud Delaunay
mesh populates every bin of the adjoint kernel.  Every output buffer is NaN-filled before a launch.  n = 1 and 5 directions, so that a
chunk is crossed (four directions per pass of J . dX, two fields per pass of J^T . v: there n = 3 as well); directions 0 and 4 are held to
the model.

The bars, on the model's own scales (per row: the tangent's row scale times sum |u| + |b|; per coordinate: the sum of the absolute
contributions carried through the geometry chain, |v| included):

    J . dX:   dist(device, exact) <= max(util.GLS_EXACT_SLACK_CAP x dist(float64 restatement, exact), TANGENT_RTOL)
    J^T . v:  dist(device, exact) <= max(util.GLS_EXACT_SLACK_CAP x dist(float64 restatement, exact), ADJOINT_RTOL)

The restatement is the same algorithm in plain float64 on the CPU; TANGENT_RTOL and ADJOINT_RTOL are the tangent's and the adjoint
kernel's existing bars.  Nothing in a bar is measured on the code under test.  Measured on an MI355X: see DESIGN.md 4.18."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the child process of test_forced_global_class: the paths tests/conftest.py sets up
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import gls_derivative_exact as D  # noqa: E402
import gls_shape_jacobian_model as JM  # noqa: E402
import test_gpu_gls_shape_adjoint as SA  # noqa: E402
import test_gpu_gls_shape_tangent as ST  # noqa: E402
import util  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402
from test_gpu_gls_tangent import ADJOINT_RTOL, TANGENT_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

SLACK = util.GLS_EXACT_SLACK_CAP
MESHES = SA.MESHES
N_DIR = 5
HELD = (0, N_DIR - 1)               # the directions held to the model
APPLY_CHUNK, TRANSPOSE_CHUNK = 4, 2


def _torch():
    import torch
    return torch


class Case(ST.Case):
    """ST.Case (one mesh on the device, its tables on the host, the launches of the shape adjoint and the shape tangent) with a cell
    field u, node values b, N_DIR directions and node fields, the kept Jacobian and the models' answers"""

    def __init__(self, name, make=None):
        super().__init__(name, make)
        rng = np.random.default_rng(43)
        self.u, self.b = rng.uniform(-1.0, 1.0, self.E), rng.uniform(-1.0, 1.0, self.P)
        self.dXs = rng.uniform(-1.0, 1.0, (N_DIR, self.P, 3))
        self.vs = rng.uniform(-1.0, 1.0, (N_DIR, self.P))
        self.nnz_f = int(self.grid._scalar("nnz_fsup"))
        self.ptr, self.esup, self.rows = D._rows(self.grid)
        self._jac = {}

    def stream(self):
        return _torch().cuda.current_stream(self.dev).cuda_stream

    def to_dev(self, a):
        return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def linearize(self, with_b=True, u=None):
        ud, bd = self.to_dev(self.u if u is None else u), self.to_dev(self.b)
        J = self.plan.linearize_points(ud.data_ptr(), bd.data_ptr() if with_b else 0, self.stream())
        _torch().cuda.synchronize(self.dev)
        return J

    def jac(self, with_b=True):
        if with_b not in self._jac:
            self._jac[with_b] = self.linearize(with_b)
        return self._jac[with_b]

    def _apply(self, launch, x, per_in, out_shape):
        torch = _torch()
        x = np.ascontiguousarray(x, dtype=np.float64)
        x = x[None] if x.ndim == per_in else x
        n = len(x)
        xd = self.to_dev(x)
        out = torch.full((n,) + out_shape, float("nan"), dtype=torch.float64, device=self.dev)
        launch(xd.data_ptr(), out.data_ptr(), n, self.stream())
        torch.cuda.synchronize(self.dev)
        return out.cpu().numpy()

    def jvp(self, J, dX):
        """J . dX [n][P] for dX [P][3] or [n][P][3], into a NaN-filled buffer"""
        return self._apply(J.launch_jvp, dX, 2, (self.P,))

    def vjp(self, J, v):
        """J^T . v [n][P][3] for v [P] or [n][P], into a NaN-filled buffer"""
        return self._apply(J.launch_vjp, v, 1, (self.P, 3))

    def backward_points(self, ghat, gnws=None):
        """launch_weights_backward_points(ghat, gnws), add_neumann = True, into a NaN-filled buffer"""
        torch = _torch()
        g, gn = self.to_dev(ghat), None if gnws is None else self.to_dev(gnws)
        out = torch.full((self.P, 3), float("nan"), dtype=torch.float64, device=self.dev)
        self.plan.launch_weights_backward_points(g.data_ptr(), out.data_ptr(), 0 if gn is None else gn.data_ptr(), self.stream(), add_neumann=True)
        torch.cuda.synchronize(self.dev)
        return out.cpu().numpy()

    def model_args(self):
        return (self.grid, self.perm, self.dmag, self.flag, self.inpoel, self.inpofa)

    def jvp_models(self, dtype):
        """[with b, without][held direction] dicts of the model of J . dX in dtype, one pass over the nodes"""
        if ("jvp", dtype) not in self._models:
            self._models[("jvp", dtype)] = JM.jvp_models(*self.model_args(), self.u, (self.b, None), [self.dXs[t] for t in HELD], dtype)
        return self._models[("jvp", dtype)]

    def vjp_models(self, dtype):
        """the same for J^T . v"""
        if ("vjp", dtype) not in self._models:
            self._models[("vjp", dtype)] = JM.vjp_models(*self.model_args(), self.u, (self.b, None), [self.vs[t] for t in HELD], dtype)
        return self._models[("vjp", dtype)]

    def jacobian_models(self, dtype):
        return self.jvp_models(dtype), self.vjp_models(dtype)

    def record_bytes(self):
        return 24 * self.nnz + 48 * self.nnz_f + 24 * self.P

    def scratch_bytes(self, n_jvp, n_vjp):
        return min(n_jvp, APPLY_CHUNK) * (24 * self.E + 48 * self.F) + min(n_vjp, TRANSPOSE_CHUNK) * (24 * self.E + 96 * self.F)


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=sorted(MESHES))
def case(request):
    return get_case(request.param)


def jvp_bar(tag, got, ex, re):
    """prints the line of record and returns (whether `got` is inside the J . dX bar of the module's docstring, the bar)"""
    d_ref, d_dev = D.dist(re["value"], ex["value"], ex["scale"]), D.dist(got, ex["value"], ex["scale"])
    assert d_ref <= D.CASE_CAP, (tag, d_ref)
    bar = max(SLACK * d_ref, TANGENT_RTOL)
    ratio = d_dev / d_ref if d_ref > 0 else float("inf")
    print(f"{tag}: J.dX restatement {d_ref:.2e}, device {d_dev:.2e}, ratio {ratio:.2f}, bar {bar:.2e}{'' if d_dev <= bar else '  MISSED'}")
    return d_dev <= bar, bar


def vjp_bar(tag, got, ex, re):
    """the same for J^T . v"""
    d_ref, d_dev = D.dist(re["grad_points"], ex["grad_points"], ex["scale"]), D.dist(got, ex["grad_points"], ex["scale"])
    assert d_ref <= D.CASE_CAP, (tag, d_ref)
    bar = max(SLACK * d_ref, ADJOINT_RTOL)
    ratio = d_dev / d_ref if d_ref > 0 else float("inf")
    print(f"{tag}: J^T.v restatement {d_ref:.2e}, device {d_dev:.2e}, ratio {ratio:.2f}, bar {bar:.2e}{'' if d_dev <= bar else '  MISSED'}")
    return d_dev <= bar, bar


def check_jvp_against_the_model(c, tag=""):
    jex, jre = c.jvp_models(D.LD), c.jvp_models(np.float64)
    ok = []
    for i, with_b in enumerate((True, False)):
        J = c.jac(with_b)
        out, one = c.jvp(J, c.dXs), c.jvp(J, c.dXs[0])                       # n = 5 crosses the chunk of four, n = 1
        assert out.shape == (N_DIR, c.P) and np.all(np.isfinite(out)) and one[0].tobytes() == out[0].tobytes()
        for k, t in enumerate(HELD):
            zero = ~jex[i][k]["computed"]
            assert zero.any() and not zero.all() and not out[:, zero].any()      # zero rows of the forward: exactly 0
            ok.append(jvp_bar(f"{c.name}{tag} neumann_values={'given' if with_b else 'none'}, direction {t}", out[t], jex[i][k], jre[i][k])[0])
    # b really enters
    assert np.abs(jex[0][0]["value"] - jex[1][0]["value"]).max() > 1e-6 * np.abs(jex[0][0]["value"]).max()
    assert all(ok), (c.name, tag)


def check_vjp_against_the_model(c, tag=""):
    vex, vre = c.vjp_models(D.LD), c.vjp_models(np.float64)
    ok = []
    for i, with_b in enumerate((True, False)):
        J = c.jac(with_b)
        grads = {n: c.vjp(J, c.vs[:n]) for n in (N_DIR, 1, TRANSPOSE_CHUNK + 1)}     # n = 5 and 3 cross the chunk of two
        g = grads[N_DIR]
        assert g.shape == (N_DIR, c.P, 3) and np.all(np.isfinite(g))
        assert grads[1][0].tobytes() == g[0].tobytes() and grads[TRANSPOSE_CHUNK + 1].tobytes() == g[:TRANSPOSE_CHUNK + 1].tobytes()
        for k, t in enumerate(HELD):
            ok.append(vjp_bar(f"{c.name}{tag} neumann_values={'given' if with_b else 'none'}, direction {t}", g[t], vex[i][k], vre[i][k])[0])
    assert np.abs(vex[0][0]["grad_points"] - vex[1][0]["grad_points"]).max() > 1e-6 * np.abs(vex[0][0]["grad_points"]).max()
    assert all(ok), (c.name, tag)


def test_jvp_against_the_model(case):
    """J . dX with and without neumann values, n = 1 and 5"""
    check_jvp_against_the_model(case)


def test_vjp_against_the_model(case):
    """J^T . v with and without neumann values, n = 1, 3 and 5"""
    check_vjp_against_the_model(case)


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    c.jac(True)                                # (the linearisation makes the bins itself)
    plan = c.grid.gls_adjoint_plan()
    assert list(plan) == ["lds1", "lds2", "lds4", "global"] and all(v > 0 for v in plan.values()), plan
    assert sum(plan.values()) == c.P


def test_a_batch_of_seven_equals_its_members_one_by_one():
    """J . dX in chunks of 4 + 3 and J^T . v in chunks of 2 + 2 + 2 + 1, on the smallest mesh"""
    c = get_case("tet")
    J = c.jac(True)
    seven = lambda x: np.concatenate([x, 0.5 * x, -3.0 * x])[:7]          # noqa: E731  (the module's five, and scaled copies of the first two)
    dXs, vs = seven(c.dXs), seven(c.vs)
    bj, bv = c.jvp(J, dXs), c.vjp(J, vs)
    assert bj.shape == (7, c.P) and bj[6].any() and bj.tobytes() == np.stack([c.jvp(J, dXs[t])[0] for t in range(7)]).tobytes()
    assert bv.shape == (7, c.P, 3) and bv[6].any() and bv.tobytes() == np.stack([c.vjp(J, vs[t])[0] for t in range(7)]).tobytes()


def test_bit_for_bit(case):
    c = case
    J = c.jac(True)
    # v = 1 is the shape adjoint of the cotangent (u[esup], b), bit for bit
    ones = c.vjp(J, np.ones(c.P))[0]
    assert ones.tobytes() == c.backward_points(c.u[c.esup], c.b).tobytes()
    assert c.vjp(c.jac(False), np.ones(c.P))[0].tobytes() == c.backward_points(c.u[c.esup]).tobytes()
    # batches of 2, 3 and 5 equal their members one by one; two calls agree
    singles_j = [c.jvp(J, c.dXs[t])[0] for t in range(N_DIR)]
    singles_v = [c.vjp(J, c.vs[t])[0] for t in range(N_DIR)]
    for n in (2, 3, 5):
        bj, bv = c.jvp(J, c.dXs[:n]), c.vjp(J, c.vs[:n])
        for t in range(n):
            assert bj[t].tobytes() == singles_j[t].tobytes() and bv[t].tobytes() == singles_v[t].tobytes(), (n, t)
    assert c.jvp(J, c.dXs).tobytes() == c.jvp(J, c.dXs).tobytes() and c.vjp(J, c.vs).tobytes() == c.vjp(J, c.vs).tobytes()
    # 2 dX and 2 v give exactly twice; a zero direction gives exact zeros (inside a batch too)
    assert c.jvp(J, 2.0 * c.dXs[0])[0].tobytes() == (2.0 * singles_j[0]).tobytes()
    assert c.vjp(J, 2.0 * c.vs[0])[0].tobytes() == (2.0 * singles_v[0]).tobytes()
    zj = c.jvp(J, np.stack([c.dXs[1], np.zeros((c.P, 3)), c.dXs[2]]))
    zv = c.vjp(J, np.stack([c.vs[1], np.zeros(c.P), c.vs[2]]))
    assert not zj[1].any() and not zv[1].any() and zj[0].tobytes() == singles_j[1].tobytes() and zv[2].tobytes() == singles_v[2].tobytes()
    # zero-row nodes: exact zeros in J . dX, and no contribution to J^T . v; a Dirichlet node is one of them but has an entry in J^T . v
    cell, face, own = J.fetch()
    assert cell.shape == (c.nnz, 3) and face.shape == (c.nnz_f, 6) and own.shape == (c.P, 3)
    assert np.all(np.isfinite(cell)) and np.all(np.isfinite(face)) and np.all(np.isfinite(own))
    computed = np.abs(own).max(axis=1) > 0
    zero = ~computed
    dirichlet = (np.asarray(c.grid.boundary_points).astype(np.int64) != 0) & (c.flag == 0)
    assert dirichlet.any() and zero[dirichlet].all() and computed.any()
    assert not cell[zero[c.rows]].any() and not np.stack(singles_j)[:, zero].any()
    assert not c.vjp(J, np.where(zero, c.vs[0], 0.0)).any()                  # a cotangent on the zero rows alone
    assert np.count_nonzero(np.abs(singles_v[0][dirichlet]).max(axis=1)) >= 1


def test_relinearize_is_a_fresh_linearisation(case):
    c = case
    u2 = np.random.default_rng(31).uniform(-1.0, 1.0, c.E)
    fresh = c.linearize(True, u2)
    J = c.linearize(True)                      # at u ...
    before = J.fetch()[0]
    ud, bd = c.to_dev(u2), c.to_dev(c.b)
    J.relinearize(ud.data_ptr(), bd.data_ptr(), c.stream())                  # ... moved to u2
    _torch().cuda.synchronize(c.dev)
    a, b = J.fetch(), fresh.fetch()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].tobytes() != before.tobytes()
    assert c.jvp(J, c.dXs).tobytes() == c.jvp(fresh, c.dXs).tobytes() and c.vjp(J, c.vs).tobytes() == c.vjp(fresh, c.vs).tobytes()
    assert all(J.record_ptrs) and J.record_ptrs[0] != fresh.record_ptrs[0]
    assert J.nbytes == c.record_bytes() + c.scratch_bytes(N_DIR, N_DIR)
    fresh.release()
    J.release()
    with pytest.raises(ValueError, match="released"):
        J.launch_jvp(8, 8)


def test_duality_on_the_device(case):
    """|<v, J dX> - <J^T v, dX>| <= ADJOINT_RTOL sum scale_X |dX| + TANGENT_RTOL sum_row scale_row |v_row|, both sides from the device --
    the form of the shape tangent's duality bar, the scales from the 80-bit models.  And launch_jvp against launch_weights_tangent_points
    followed by the row sums, which factorises every node again, under the J . dX bar."""
    c = case
    (jex, vex), (jre, _) = c.jacobian_models(D.LD), c.jacobian_models(np.float64)
    for i, with_b in enumerate((True, False)):
        J = c.jac(with_b)
        for k, t in enumerate(HELD):
            dX, v = c.dXs[t], c.vs[t]
            out, g = c.jvp(J, dX)[0], c.vjp(J, v)[0]
            lhs, rhs = float(v @ out), float((g * dX).sum())
            bar = ADJOINT_RTOL * float((vex[i][k]["scale"] * np.abs(dX)).sum()) + TANGENT_RTOL * float((jex[i][k]["scale"] * np.abs(v)).sum())
            print(f"{c.name} neumann_values={'given' if with_b else 'none'}, direction {t}: duality gap {abs(lhs - rhs):.3e}, bar {bar:.3e}, "
                  f"|<J^T v, dX>| {abs(rhs):.3e}")
            assert abs(rhs) > 0 and abs(lhs - rhs) <= bar
            # the one-shot tangent followed by the row sums
            dw, dn = c.tangent(True, True, dX)
            ref = np.bincount(c.rows, weights=dw[0] * c.u[c.esup], minlength=c.P) + (dn[0] * c.b if with_b else 0.0)
            d_ref = D.dist(jre[i][k]["value"], jex[i][k]["value"], jex[i][k]["scale"])
            d = D.dist(out, ref, jex[i][k]["scale"])
            bar = max(SLACK * d_ref, TANGENT_RTOL)
            print(f"    launch_jvp against launch_weights_tangent_points + row sums: {d:.2e} of the row scale, bar {bar:.2e}")
            assert d <= bar


# ---- state ----------------------------------------------------------------------------------------------------------------------------

def test_a_jacobian_only_session_makes_none_of_the_grids_buffers():
    from ninpol_amd import _lib
    from ninpol_amd.interpolator import GlsShapeJacobian
    c = Case("tet")                            # a grid of its own: nothing has run on it
    scalars = ("gls_shape_contrib_bytes", "gls_shape_tangent_bytes", "gls_adjoint_contrib_bytes")
    assert all(c.grid._scalar(s) == 0 for s in scalars)
    J = c.linearize(True)
    assert J.is_current() and J.stamp == (c.grid.field_updates, c.grid.geometry_updates, c.grid.flag_updates)
    assert J.record_bytes == c.record_bytes() and J.nbytes == c.record_bytes()              # no scratch before the first apply
    jb = c.jvp(J, c.dXs[0])
    assert J.nbytes == c.record_bytes() + c.scratch_bytes(1, 0)
    vb = c.vjp(J, c.vs[0])
    assert J.nbytes == c.record_bytes() + c.scratch_bytes(1, 1)
    j5, v5 = c.jvp(J, c.dXs), c.vjp(J, c.vs)
    assert J.nbytes == c.record_bytes() + c.scratch_bytes(N_DIR, N_DIR)                     # grown to a whole chunk, and kept
    assert j5[0].tobytes() == jb[0].tobytes() and v5[0].tobytes() == vb[0].tobytes()        # growth left the bits
    assert c.jvp(J, c.dXs[0]).tobytes() == jb.tobytes() and J.nbytes == c.record_bytes() + c.scratch_bytes(N_DIR, N_DIR)
    assert all(c.grid._scalar(s) == 0 for s in scalars)
    # a launch_weights_backward_points in between leaves the object's answers bit-identical, and the other way round
    rng = np.random.default_rng(5)
    gh, gn = rng.uniform(-1, 1, c.nnz), rng.uniform(-1, 1, c.P)
    xb = c.backward_points(gh, gn)                                                          # makes and fills the grid's own records
    assert c.grid._scalar("gls_shape_contrib_bytes") == 24 * c.nnz + 48 * c.nnz_f + 96 * c.F
    assert c.jvp(J, c.dXs).tobytes() == j5.tobytes() and c.vjp(J, c.vs).tobytes() == v5.tobytes()
    assert c.backward_points(gh, gn).tobytes() == xb.tobytes()
    # the scratch goes -- bins, transpose index, connectivity, the grid's records -- and the object still answers
    c.grid.release_scratch()
    assert c.grid._scalar("gls_shape_contrib_bytes") == 0 and not c.grid.has_transpose_index
    assert c.jvp(J, c.dXs).tobytes() == j5.tobytes()
    assert c.vjp(J, c.vs).tobytes() == v5.tobytes() and c.grid.has_transpose_index
    assert all(c.grid._scalar(s) == 0 for s in scalars)
    # argument errors on a live object, and the state error of one that was never linearised
    with pytest.raises(_lib.NinpolError) as e:
        J.launch_jvp(8, 8, n=0)
    assert e.value.code == _lib.NIN_EINVAL
    with pytest.raises(_lib.NinpolError) as e:
        J.launch_vjp(0, 8)
    assert e.value.code == _lib.NIN_EINVAL
    raw = GlsShapeJacobian(c.grid)
    for launch in (raw.launch_jvp, raw.launch_vjp):
        with pytest.raises(_lib.NinpolError) as e:
            launch(8, 8)
        assert e.value.code == _lib.NIN_ESTATE and "nin_gls_xjacobian_linearize" in e.value.text
    assert raw.stamp == (-1, -1, -1) and not raw.is_current()
    with pytest.raises(_lib.NinpolError) as e:
        raw.fetch()
    assert e.value.code == _lib.NIN_ESTATE
    raw.release()
    # release() frees everything
    J.release()
    for call in (lambda: J.launch_jvp(8, 8), lambda: J.launch_vjp(8, 8), lambda: J.nbytes, J.fetch):
        with pytest.raises(ValueError, match="released"):
            call()


def test_updates_of_the_permeability_and_the_flags_are_not_refused_but_the_points_are():
    torch = _torch()
    from ninpol_amd import _lib
    c = Case("mixed")                          # its own Interpolator: the resident tables and the mesh are rewritten
    J = c.linearize(True)
    jb, vb = c.jvp(J, c.dXs), c.vjp(J, c.vs)
    K2 = c.perm * np.random.default_rng(7).uniform(1.5, 2.5, (c.E, 1))
    c.I.update_permeability(c.to_dev(K2.reshape(c.E, 3, 3)))
    flags = c.flag.astype(np.float64)
    flags[np.flatnonzero(c.flag)[::2]] = 0.0   # every other Neumann node becomes a Dirichlet node
    c.I.update_neumann_flags("u", c.to_dev(flags))
    torch.cuda.synchronize(c.dev)
    assert not J.is_current() and c.grid.field_updates >= 1 and c.grid.flag_updates >= 1
    assert c.jvp(J, c.dXs).tobytes() == jb.tobytes() and c.vjp(J, c.vs).tobytes() == vb.tobytes()
    # the backward call on the same grid now answers for the new tables
    assert c.vjp(J, np.ones(c.P))[0].tobytes() != c.backward_points(c.u[c.esup], c.b).tobytes()
    # an update of the points: both applies are refused and write nothing
    X2 = c.coords + np.random.default_rng(11).uniform(-1e-3, 1e-3, (c.P, 3))
    c.I.update_points(X2)
    assert not J.is_current() and J.stamp[1] != c.grid.geometry_updates
    dx, v = c.to_dev(c.dXs), c.to_dev(c.vs)
    out = torch.full((N_DIR, c.P), float("nan"), dtype=torch.float64, device=c.dev)
    grad = torch.full((N_DIR, c.P, 3), float("nan"), dtype=torch.float64, device=c.dev)
    for launch, a, o in ((J.launch_jvp, dx, out), (J.launch_vjp, v, grad)):
        for n in (1, N_DIR):
            with pytest.raises(RuntimeError, match="nin_gls_xjacobian_linearize again") as e:
                launch(a.data_ptr(), o.data_ptr(), n, c.stream())
            assert isinstance(e.value, _lib.NinpolError) and e.value.code == _lib.NIN_ESTATE and "geometry_updates" in e.value.text
    L = _lib.load()
    hx, hv, ho, hg = c.dXs[0].copy(), c.vs[0].copy(), np.full(c.P, np.nan), np.full((c.P, 3), np.nan)
    assert L.nin_gls_xjacobian_apply_host(J._handle(), 1, _lib._ptr(hx), _lib._ptr(ho)) == _lib.NIN_ESTATE
    assert L.nin_gls_xjacobian_apply_transpose_host(J._handle(), 1, _lib._ptr(hv), _lib._ptr(hg)) == _lib.NIN_ESTATE
    torch.cuda.synchronize(c.dev)
    assert torch.isnan(out).all() and torch.isnan(grad).all() and np.isnan(ho).all() and np.isnan(hg).all()
    # relinearize: a fresh linearisation at the new point (geometry, K and flags)
    ud, bd = c.to_dev(c.u), c.to_dev(c.b)
    J.relinearize(ud.data_ptr(), bd.data_ptr(), c.stream())
    fresh = c.linearize(True)
    assert J.is_current() and fresh.is_current()
    a, b = J.fetch(), fresh.fetch()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    j2, v2 = c.jvp(J, c.dXs), c.vjp(J, c.vs)
    assert j2.tobytes() == c.jvp(fresh, c.dXs).tobytes() and v2.tobytes() == c.vjp(fresh, c.vs).tobytes()
    assert np.abs(j2 - jb).max() > 1e-6 * np.abs(jb).max()
    assert c.vjp(J, np.ones(c.P))[0].tobytes() == c.backward_points(c.u[c.esup], c.b).tobytes()


# ---- the upper layers -------------------------------------------------------------------------------------------------------------------

def test_points_jacobian():
    c = get_case("mixed")
    (jex, vex), (jre, vre) = c.jacobian_models(D.LD), c.jacobian_models(np.float64)
    with_b = c.I.points_jacobian("u", c.u, c.b)
    op = c.I.points_jacobian("u", c.u)
    assert op.shape == (c.P, 3 * c.P) and op.dtype == np.float64 and not hasattr(op, "to_scipy")
    X = np.ascontiguousarray(c.dXs.reshape(N_DIR, 3 * c.P).T)           # (3 P, k)
    V = np.ascontiguousarray(c.vs.T)                                   # (P, k)
    mv, rmv, mm, rmm = op.matvec(X[:, 0]), op.rmatvec(V[:, 0]), op.matmat(X), op.rmatmat(V)
    assert mv.shape == (c.P,) and rmv.shape == (3 * c.P,) and mm.shape == (c.P, N_DIR) and rmm.shape == (3 * c.P, N_DIR)
    assert mm[:, 0].tobytes() == mv.tobytes() and rmm[:, 0].tobytes() == rmv.tobytes()
    assert (op @ X[:, 4]).tobytes() == np.ascontiguousarray(mm[:, 4]).tobytes() and (op.T @ V[:, 4]).tobytes() == np.ascontiguousarray(rmm[:, 4]).tobytes()
    # the kept object's own launches
    J = c.jac(False)
    assert c.jvp(J, c.dXs).tobytes() == np.ascontiguousarray(mm.T).tobytes() and c.vjp(J, c.vs).tobytes() == np.ascontiguousarray(rmm.T).tobytes()
    ok = []
    for k, t in enumerate(HELD):
        ok.append(jvp_bar(f"points_jacobian, direction {t}", mm[:, t], jex[1][k], jre[1][k])[0])
        ok.append(vjp_bar(f"points_jacobian, direction {t}", rmm[:, t].reshape(c.P, 3), vex[1][k], vre[1][k])[0])
        ok.append(jvp_bar(f"points_jacobian with neumann values, direction {t}", with_b.matvec(X[:, t]), jex[0][k], jre[0][k])[0])
        ok.append(vjp_bar(f"points_jacobian with neumann values, direction {t}", with_b.rmatvec(V[:, t]).reshape(c.P, 3), vex[0][k], vre[0][k])[0])
    assert all(ok)
    # against the per-call siblings, which factorise every node again
    dv, dn = c.I.points_tangent("u", c.dXs[0], c.u)
    _, bar = jvp_bar("points_tangent", dv, jex[1][0], jre[1][0])
    d = D.dist(mv, dv, jex[1][0]["scale"])
    print(f"points_jacobian.matvec against points_tangent: {d:.2e} of the row scale, bar {bar:.2e}")
    assert d <= bar
    d = D.dist(with_b.matvec(X[:, 0]), dv + dn * c.b, jex[0][0]["scale"])
    assert d <= max(SLACK * D.dist(jre[0][0]["value"], jex[0][0]["value"], jex[0][0]["scale"]), TANGENT_RTOL)
    gx = c.I.points_gradient("u", c.vs[0], c.u)
    _, bar = vjp_bar("points_gradient", gx, vex[1][0], vre[1][0])
    d = D.dist(rmv.reshape(c.P, 3), gx, vex[1][0]["scale"])
    print(f"points_jacobian.rmatvec against points_gradient: {d:.2e} of the coordinate scale, bar {bar:.2e}")
    assert d <= bar
    with pytest.raises(ValueError):
        c.I.points_jacobian("u", c.u[:-1])
    with pytest.raises(ValueError):
        c.I.points_jacobian("u", c.u, c.b[:-1])
    op.release()
    with_b.release()
    with pytest.raises(ValueError, match="released"):
        op.matvec(X[:, 0])


def test_cell_to_node_linearize_points():
    """CellToNode.linearize(u, points=X, wrt="points"): jvp against forward_ad of CellToNode(u, points=X), vjp against its backward"""
    torch = _torch()
    import torch.autograd.forward_ad as fwAD
    from ninpol_amd.torch_ops import CellToNode
    c = Case("mixed")                          # its own Interpolator: the op rewrites the resident coordinates
    dev = c.dev
    op = CellToNode(c.I, "u", "gls")
    rng = np.random.default_rng(9)
    u0, du0, g0 = (torch.from_numpy(rng.uniform(-1.0, 1.0, n)).to(dev) for n in (c.E, c.E, c.P))
    X0 = torch.from_numpy(c.coords + rng.uniform(-1e-3, 1e-3, (c.P, 3))).to(dev)
    dX0 = torch.from_numpy(c.dXs[0]).to(dev)
    b0 = torch.from_numpy(c.b).to(dev)
    geom = c.grid.geometry_updates
    lin = op.linearize(u0, points=X0, wrt="points")
    assert c.grid.geometry_updates == geom + 1 and lin.wrt == "points" and lin.jacobian.is_current()
    assert torch.equal(lin.value, op(u0, points=X0))                      # bit-identical to forward (which moves the mesh to X0 again)
    lin = op.linearize(u0, wrt="points")                                  # at what is resident: X0, and a current stamp
    assert torch.equal(lin.value, op._spmv(op._launch_weights()[0], u0)) and lin.jacobian.is_current()
    # the models at X0 (the grid's arrays are fetched again after an update)
    assert np.array_equal(np.asarray(c.grid.point_coords).reshape(-1, 3), X0.cpu().numpy())
    u_np, g_np = u0.cpu().numpy(), g0.cpu().numpy()
    args = (c.grid, c.perm, c.dmag, c.flag, c.inpoel, c.inpofa)
    jex, jre = (JM.jvp_models(*args, u_np, [None], [c.dXs[0]], dt)[0][0] for dt in (D.LD, np.float64))
    vex, vre = (JM.vjp_models(*args, u_np, [None], [g_np], dt)[0][0] for dt in (D.LD, np.float64))
    # forward mode: W du + J dX against forward_ad's W du + dW u
    with fwAD.dual_level():
        out = op(fwAD.make_dual(u0, du0), points=fwAD.make_dual(X0, dX0))
        tangent = fwAD.unpack_dual(out).tangent
        only_x = fwAD.unpack_dual(op(u0, points=fwAD.make_dual(X0, dX0))).tangent
    lin = op.linearize(u0, wrt="points")                                  # (forward moved the mesh to X0 again: a new stamp)
    w_du = op._spmv(lin.weights, du0)
    jx = lin.jvp(dpoints=dX0)
    assert torch.equal(lin.jvp(du0), w_du) and torch.equal(lin.jvp(du0, dpoints=dX0), w_du + jx)
    _, bar = jvp_bar("CellToNode.linearize(wrt='points').jvp", jx.cpu().numpy(), jex, jre)
    d = D.dist(jx.cpu().numpy(), only_x.cpu().numpy(), jex["scale"])
    d2 = D.dist((w_du + jx).cpu().numpy(), tangent.cpu().numpy(), jex["scale"])
    print(f"jvp against forward_ad: {d:.2e} (dual points), {d2:.2e} (dual u and points) of the row scale, bar {bar:.2e}")
    assert d <= bar and d2 <= bar and jx.abs().max() > 0
    batch = lin.jvp(dpoints=torch.stack([dX0, 2.0 * dX0]))
    assert batch.shape == (2, c.P) and torch.equal(batch[0], jx) and torch.equal(batch[1], 2.0 * jx)
    assert torch.equal(lin.jvp(), torch.zeros(c.P, dtype=torch.float64, device=dev))
    # reverse mode against backward()
    X, u = X0.clone().requires_grad_(), u0.clone().requires_grad_()
    (op(u, points=X) * g0).sum().backward()
    lin = op.linearize(u0, wrt="points")
    gu, gx = lin.vjp(g0)
    assert gx.shape == (c.P, 3) and torch.equal(gu, u.grad)
    _, bar = vjp_bar("CellToNode.linearize(wrt='points').vjp", gx.cpu().numpy(), vex, vre)
    d = D.dist(gx.cpu().numpy(), X.grad.cpu().numpy(), vex["scale"])
    print(f"vjp against backward(): {d:.2e} of the coordinate scale, bar {bar:.2e}")
    assert d <= bar
    gub, gxb = lin.vjp(torch.stack([g0, g0]))
    assert gxb.shape == (2, c.P, 3) and torch.equal(gxb[0], gx) and torch.equal(gxb[1], gx) and gub.shape == (2, c.E)
    # neumann values enter the Jacobian, not the value
    linb = op.linearize(u0, neumann_values=b0, wrt="points")
    assert torch.equal(linb.value, lin.value) and not torch.equal(linb.jvp(dpoints=dX0), jx)
    # the refusals: a direction in K, a direction in the points for a linearisation in K, IDW / LS, a moved mesh
    K0 = torch.from_numpy(c.perm.reshape(c.E, 3, 3).copy()).to(dev)
    for kw, t in (("dK", K0), ("dscale", u0)):
        with pytest.raises(ValueError, match='a linearisation taken with wrt="points" holds no derivative in K: ' + kw + " must be None"):
            lin.jvp(**{kw: t})
    with pytest.raises(ValueError, match="dpoints must be None"):
        op.linearize(u0).jvp(dpoints=dX0)
    with pytest.raises(ValueError, match="wrt must be"):
        op.linearize(u0, wrt="X")
    for meth in ("idw", "ls"):
        other = CellToNode(c.I, "u", meth)
        with pytest.raises(ValueError, match="not differentiated"):
            other.linearize(u0, wrt="points")
        with pytest.raises(ValueError, match="not differentiated"):
            other.linearize(u0, points=X0)
        with pytest.raises(ValueError, match="do depend on the node coordinates, but they are not differentiated"):
            other.plan.linearize_points(u0.data_ptr())
    c.I.update_points(X0)
    with pytest.raises(RuntimeError, match="linearize again"):
        lin.jvp(dpoints=dX0)
    with pytest.raises(RuntimeError, match="linearize again"):
        lin.vjp(g0)
    lin.release()
    linb.release()
    torch.cuda.synchronize(dev)


# ---- the ABI contract of the entry points on a device -----------------------------------------------------------------------------------

def test_abi_two_dimensional_grid_and_before_the_first_linearisation():
    import ninpol_amd
    from ninpol_amd import _lib
    torch = _torch()
    L = _lib.load()
    dev, buf = torch.zeros(1 << 12, dtype=torch.float64, device="cuda"), np.zeros(1 << 12)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                         # noqa: E731
    hp = buf.ctypes.data_as(ctypes.c_void_p)
    mesh = M.attach_fields(M.quad_tri_mesh_2d(4), "u", perm="LIN", neumann_plane=(1, 0.0), seed=5)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    assert int(I.grid.dim) == 2 and int(I.grid.n_points) * 3 <= 1 << 12
    I._gls_tables_to_device("u")
    h = ctypes.c_void_p()
    assert L.nin_gls_xjacobian_create(I.grid._h, ctypes.byref(h)) == _lib.NIN_OK and h.value
    for call in (lambda: L.nin_gls_xjacobian_linearize(h, vp(dev), vp(dev), None), lambda: L.nin_gls_xjacobian_linearize_host(h, hp, hp)):
        rc, text = call(), L.nin_last_error().decode()
        assert rc == _lib.NIN_EINVAL and "3-D grids only" in text and "2-D" in text, (rc, text)
    # never linearised: every apply and the fetch are refused, in the words of the kept Jacobian in K
    stamp = np.zeros(3, dtype=np.int64)
    assert L.nin_gls_xjacobian_stamp(h, stamp.ctypes.data_as(ctypes.c_void_p)) == _lib.NIN_OK and tuple(stamp) == (-1, -1, -1)
    for call in (lambda: L.nin_gls_xjacobian_apply(h, 1, vp(dev), vp(dev), None), lambda: L.nin_gls_xjacobian_apply_transpose(h, 1, vp(dev), vp(dev), None),
                 lambda: L.nin_gls_xjacobian_apply_host(h, 1, hp, hp), lambda: L.nin_gls_xjacobian_apply_transpose_host(h, 1, hp, hp),
                 lambda: L.nin_gls_xjacobian_fetch_host(h, hp, hp, hp)):
        rc, text = call(), L.nin_last_error().decode()
        assert rc == _lib.NIN_ESTATE and text == "the Jacobian has not been linearised (call nin_gls_xjacobian_linearize first)", (rc, text)
    for call in (lambda: L.nin_gls_xjacobian_apply(h, 0, vp(dev), vp(dev), None), lambda: L.nin_gls_xjacobian_apply_transpose(h, 1, None, vp(dev), None),
                 lambda: L.nin_gls_xjacobian_apply(h, 1, vp(dev), None, None), lambda: L.nin_gls_xjacobian_linearize(h, None, None, None)):
        assert call() == _lib.NIN_EINVAL
    assert not buf.any() and not dev.any().item()                        # nothing was written
    assert I.grid._scalar("gls_shape_contrib_bytes") == 0 and I.grid._scalar("gls_shape_tangent_bytes") == 0
    L.nin_gls_xjacobian_destroy(h)


# ---- every system in global-memory scratch ------------------------------------------------------------------------------------------

def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    c.jac(True)                             # (the linearisation makes the bins itself)
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    check_jvp_against_the_model(c, " forced global")
    check_vjp_against_the_model(c, " forced global")
    assert c.vjp(c.jac(True), np.ones(c.P))[0].tobytes() == c.backward_points(c.u[c.esup], c.b).tobytes()
    print("CHILD OK")


def test_forced_global_class():
    """the hexahedron mesh again with every system in global-memory scratch, in a fresh process (the switch is read when the bins are
    made), under the same bars"""
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


if __name__ == "__main__":
    _child()
