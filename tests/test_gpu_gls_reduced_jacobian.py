"""The GLS Jacobian in a reduced parametrisation of the permeability: DevicePlan.linearize_reduced /
GlsReducedJacobian.launch_jvp / launch_vjp, Interpolator.permeability_jacobian(basis=...) and CellToNode.linearize(wrt="scale"), held to
the numpy model of tests/gls_reduced_jacobian_model.py (which tests/test_gls_reduced_jacobian_model.py pins against central differences
of the oracle), to the full Jacobian of DESIGN.md 4.13 on the same device, to a derived duality bound, and bit for bit to themselves.

The meshes, the field, the Neumann plane and the cotangents are those of tests/test_gpu_gls_jacobian.py (its Case objects are shared,
and with them the adjoint models and the full Jacobians).  The bases: the resident permeability through a NULL pointer (M = 1), a
random per-cell basis of one parameter, the built-in "diagonal" (M = 3) and "symmetric" (M = 6) as shared [M][9] arrays, a random
per-cell basis of three parameters and a random shared one of six.  Every output buffer is NaN-filled before its launch and must come
back finite.

The bars start as JVP_RTOL and VJP_RTOL of tests/test_gpu_gls_jacobian.py, imported: the row scale is the model's own for the
direction B . dtheta, the scale of parameter m of cell e is sum_k |B_(e,m)[k]| times that file's folded cell scale.

Measured on an MI355X, worst over the six bases and all variants (with / without neumann_values, n = 1 and n = 5), against the model:
  J_theta . dtheta  per row, of the model's row scale:     5.69e-13 (Delaunay, per-cell basis of three; 3.2e-13 hex, 1.2e-13 mixed, 5.4e-14 tet)
  J_theta^T . v     per parameter, of the scale above:     7.81e-12 (Delaunay, diagonal / symmetric; 3.2e-13 hex, 3.1e-13 mixed, 3.3e-13 tet)
The first is above a tenth of the imported JVP_RTOL (4.5e-12), so by the project's convention the bar of the reduced apply is 10 x the
measured worst, RJVP_RTOL = 5.7e-12; the second is below a tenth of VJP_RTOL (8.7e-11), which stands.  Neither is looser than the 1e-8
at which the model is pinned.  Against the full Jacobian on the same device the reduced products measured 2.0e-15 (apply) and 2.9e-16
(transpose) at worst, against bars that are the sum of the two kernels' bars; the device duality gap measured 0 to 3.4e-16 absolute
against derived bars of 1.0e-13 and more."""
import math

import numpy as np
import pytest

import gls_adjoint_model as GM
import gls_jacobian_model as JM
import gls_reduced_jacobian_model as RM
import gls_tangent_model as TM
from test_gpu_gls_jacobian import JVP_RTOL, MODELLED, N_DIR, U, VJP_RTOL, Case, get_case, jvp_err
from test_gpu_gls_tangent import ADJOINT_RTOL, MESHES, TANGENT_RTOL

pytestmark = pytest.mark.gpu

RJVP_RTOL = 5.7e-12      # 10 x the worst measured (see above)
RVJP_RTOL = VJP_RTOL
assert JVP_RTOL <= RJVP_RTOL <= 1e-8 and RVJP_RTOL <= 1e-8

VARIANTS = ("scale", "percell1", "diagonal", "symmetric", "percell3", "shared6")


def _torch():
    import torch
    return torch


class Reduced:
    """the reduced side of one Case: bases, directions in theta, linearisations and models (computed once, lazily)"""

    def __init__(self, c):
        self.c = c
        E = c.E
        rng = np.random.default_rng(37)
        # name -> (M, the array handed to the device or None: the resident permeability, per-cell flag)
        self.bases = {
            "scale": (1, None, True),
            "percell1": (1, rng.uniform(-1.0, 1.0, (E, 1, 9)), True),
            "diagonal": (3, RM.builtin_basis("diagonal", c.perm)[0].copy(), False),
            "symmetric": (6, RM.builtin_basis("symmetric", c.perm)[0].copy(), False),
            "percell3": (3, rng.uniform(-1.0, 1.0, (E, 3, 9)), True),
            "shared6": (6, rng.uniform(-1.0, 1.0, (6, 9)), False),
        }
        self.dtheta = {}
        for k in VARIANTS:
            self.dtheta[k] = rng.uniform(-1.0, 1.0, (N_DIR, E, self.bases[k][0]))
            self.dtheta[k][2] = 0.0                                                   # a zero direction inside the batch
        self._jac, self._tan = {}, {}

    def M(self, k):
        return self.bases[k][0]

    def B(self, k):
        """the basis as the model takes it, [E][M][9]"""
        arr = self.bases[k][1]
        return self.c.perm.reshape(self.c.E, 1, 9) if arr is None else RM.per_cell(arr, self.c.E)

    def linearize(self, k, with_b=True, u=None, basis="own", per_cell=None, plan=None):
        c = self.c
        M, arr, pc = self.bases[k]
        if not isinstance(basis, str):
            arr, pc = basis, per_cell
        ud, bd = c.to_dev(c.u if u is None else u), c.to_dev(c.b)
        Bd = None if arr is None else c.to_dev(arr)
        J = (plan or c.plan).linearize_reduced(ud.data_ptr(), M, 0 if Bd is None else Bd.data_ptr(), pc, bd.data_ptr() if with_b else 0,
                                               c.stream())
        _torch().cuda.synchronize(c.dev)
        assert J.n_params == M and J.nbytes == 8 * M * c.nnz and J.buffer_ptr
        return J

    def jac(self, k, with_b=True):
        if (k, with_b) not in self._jac:
            self._jac[(k, with_b)] = self.linearize(k, with_b)
        return self._jac[(k, with_b)]

    def jvp(self, J, dtheta):
        """dtheta [n][E][M] -> [n][P]"""
        c = self.c
        d = np.ascontiguousarray(dtheta).reshape(-1, c.E, J.n_params)
        dd, out = c.to_dev(d), c.nan(len(d), c.P)
        J.launch_jvp(dd.data_ptr(), out.data_ptr(), len(d), c.stream())
        _torch().cuda.synchronize(c.dev)
        out = out.cpu().numpy()
        assert np.all(np.isfinite(out)), "J_theta . dtheta is not finite (or was not written)"
        return out

    def vjp(self, J, v):
        """v [n][P] -> [n][E][M]"""
        c = self.c
        v = np.ascontiguousarray(v).reshape(-1, c.P)
        vd, out = c.to_dev(v), c.nan(len(v), c.E, J.n_params)
        J.launch_vjp(vd.data_ptr(), out.data_ptr(), len(v), c.stream())
        _torch().cuda.synchronize(c.dev)
        out = out.cpu().numpy()
        assert np.all(np.isfinite(out)), "J_theta^T . v is not finite (or was not written)"
        return out

    def jvp_model(self, k, t, with_b):
        c = self.c
        if (k, t) not in self._tan:                       # (the tangent model depends on the direction alone, not on u or b)
            self._tan[(k, t)] = TM.gls_tangent_model(c.grid, c.perm, c.dmag, c.flag, RM.direction(self.B(k), self.dtheta[k][t]),
                                                     add_neumann=True)
        return RM.jvp_model(c.grid, c.perm, c.dmag, c.flag, c.u, self.B(k), self.dtheta[k][t], b=c.b if with_b else None,
                            tangent=self._tan[(k, t)])

    def vjp_model(self, k, t, with_b):
        c = self.c
        return RM.vjp_model(c.grid, c.perm, c.dmag, c.flag, c.u, self.B(k), c.v[t], b=c.b if with_b else None, full=c.vjp_model(t, with_b))


_REDUCED = {}


def get_reduced(name):
    if name not in _REDUCED:
        _REDUCED[name] = Reduced(get_case(name))
    return _REDUCED[name]


@pytest.fixture(scope="module", params=sorted(MESHES))
def red(request):
    return get_reduced(request.param)


def vjp_err(got, m):
    """max over (cell, parameter) of |device - model| / its scale; where the scale is 0 both are exactly 0"""
    none = m["scale"] == 0
    assert not got[none].any() and not m["grad_theta"][none].any()
    return float((np.abs(got - m["grad_theta"])[~none] / m["scale"][~none]).max())


@pytest.mark.parametrize("k", VARIANTS)
def test_jvp_against_the_model(red, k):
    r, c = red, red.c
    worst = 0.0
    for with_b in (True, False):
        J = r.jac(k, with_b)
        batch = r.jvp(J, r.dtheta[k])
        one = r.jvp(J, r.dtheta[k][0])
        for tag, got, t in [("n=1", one[0], 0)] + [(f"n={N_DIR}[{t}]", batch[t], t) for t in MODELLED]:
            e = jvp_err(got, r.jvp_model(k, t, with_b))
            print(f"{c.name} {k} jvp neumann_values={with_b} {tag}: {e:.2e} of the row scale")
            assert e <= RJVP_RTOL
            worst = max(worst, e)
    print(f"{c.name} {k}: reduced jvp worst over the variants {worst:.3e}")
    m = r.jvp_model(k, 0, True)
    assert (m["scale"] == 0).any() and np.abs(m["value"]).max() > 0
    assert np.abs(r.jvp_model(k, 0, False)["value"] - m["value"]).max() > 1e-6 * np.abs(m["value"]).max()      # b is really in


@pytest.mark.parametrize("k", VARIANTS)
def test_vjp_against_the_model(red, k):
    r, c = red, red.c
    worst = 0.0
    for with_b in (True, False):
        J = r.jac(k, with_b)
        batch = r.vjp(J, c.v)
        one = r.vjp(J, c.v[0])
        for tag, got, t in [("n=1", one[0], 0)] + [(f"n={N_DIR}[{t}]", batch[t], t) for t in MODELLED]:
            m = r.vjp_model(k, t, with_b)
            e = vjp_err(got, m)
            print(f"{c.name} {k} vjp neumann_values={with_b} {tag}: {e:.2e} of the parameter scale")
            assert e <= RVJP_RTOL
            worst = max(worst, e)
    print(f"{c.name} {k}: reduced vjp worst over the variants {worst:.3e}")
    assert np.abs(r.vjp_model(k, 0, True)["grad_theta"]).max() > 0


@pytest.mark.parametrize("k", VARIANTS)
def test_against_the_full_jacobian_on_the_same_device(red, k):
    """launch_jvp of a GlsJacobian at dK = B . dtheta, and its folded launch_vjp contracted with B on the host: the reduced result lies
    within the sum of the two bars of it (both are within their bar of the model, in the model's scales)"""
    r, c = red, red.c
    B = r.B(k)
    for with_b in (True, False):
        J, F = r.jac(k, with_b), c.jac(with_b)
        got = r.jvp(J, r.dtheta[k])
        full = c.jvp(F, np.stack([RM.direction(B, r.dtheta[k][t]) for t in range(N_DIR)]))
        gt = r.vjp(J, c.v)
        fp, _ = c.vjp(F, c.v, False)
        for t in MODELLED:
            m = r.jvp_model(k, t, with_b)
            none = m["scale"] == 0
            assert not got[t][none].any() and not full[t][none].any()
            e = float((np.abs(got[t] - full[t])[~none] / m["scale"][~none]).max())
            a = r.vjp_model(k, t, with_b)
            want = np.einsum("emk,ek->em", B, fp[t].reshape(c.E, 9))
            zero = a["scale"] == 0
            assert not gt[t][zero].any() and not want[zero].any()
            ev = float((np.abs(gt[t] - want)[~zero] / a["scale"][~zero]).max())
            print(f"{c.name} {k} neumann_values={with_b} t={t}: reduced against full, jvp {e:.2e}, vjp {ev:.2e}")
            assert e <= RJVP_RTOL + JVP_RTOL and ev <= RVJP_RTOL + VJP_RTOL


@pytest.mark.parametrize("k", VARIANTS)
def test_duality_on_the_device(red, k):
    """|<v, R dtheta> - <R^T v, dtheta>| <= 2 (N + 2) 2^-53 S with N = M nnz products per side and S = sum |v_p R[pos][m] dtheta_(e,m)|
    from the fetched R: the worst-case bound of two sums of N products, each product and each addition rounded once (the host's dot
    products are taken with math.fsum), as DESIGN.md 4.13 derives it"""
    r, c = red, red.c
    for with_b in (True, False):
        J = r.jac(k, with_b)
        R = J.fetch()
        assert R.shape == (c.nnz, r.M(k)) and np.all(np.isfinite(R))
        N = r.M(k) * c.nnz
        for t in MODELLED:
            v, dth = c.v[t], r.dtheta[k][t]
            lhs = math.fsum(v * r.jvp(J, dth)[0])
            rhs = math.fsum((r.vjp(J, v)[0] * dth).reshape(-1))
            S = math.fsum((np.abs(v[c.rows])[:, None] * np.abs(R * dth[c.esup])).reshape(-1))
            bar = 2 * (N + 2) * U * S
            print(f"{c.name} {k} neumann_values={with_b} t={t}: gap {abs(lhs - rhs):.3e}, bar {bar:.3e}, S {S:.3e}")
            assert S > 0 and abs(lhs - rhs) <= bar


@pytest.mark.parametrize("k", VARIANTS)
def test_a_batch_of_seven_equals_its_members_one_by_one(k):
    """a full chunk of four and a chunk of three behind it, both products, for M = 1, 3 and 6 on the smallest mesh"""
    r = get_reduced("tet")
    c = r.c
    J = r.jac(k, True)
    seven = lambda x: np.concatenate([x, 0.5 * x, -3.0 * x])[:7]          # noqa: E731  (the module's five, and scaled copies of the first two)
    dth, v = seven(r.dtheta[k]), seven(c.v)
    batch = r.jvp(J, dth)
    assert batch.shape == (7, c.P) and batch[6].any() and batch.tobytes() == np.stack([r.jvp(J, dth[t])[0] for t in range(7)]).tobytes()
    vb = r.vjp(J, v)
    assert vb.shape == (7, c.E, r.M(k)) and vb[6].any() and vb.tobytes() == np.stack([r.vjp(J, v[t])[0] for t in range(7)]).tobytes()


@pytest.mark.parametrize("k", VARIANTS)
def test_determinism_batching_zero_and_linearity(red, k):
    r, c = red, red.c
    J = r.jac(k, True)
    dth = r.dtheta[k]
    batch = r.jvp(J, dth)
    assert batch.tobytes() == r.jvp(J, dth).tobytes()                                 # two calls agree
    for t in range(N_DIR):                                                            # a batch equals its members one by one
        assert r.jvp(J, dth[t])[0].tobytes() == batch[t].tobytes(), t
    for n in (2, 3):                                                                  # ... and the shorter chunks
        assert r.jvp(J, dth[:n]).tobytes() == batch[:n].tobytes(), n
    assert not batch[2].any() and batch[0].any() and batch[4].any()                   # a zero direction: exact zeros
    assert (2.0 * batch).tobytes() == r.jvp(J, 2.0 * dth).tobytes()                   # 2 dtheta gives exactly twice
    vb = r.vjp(J, c.v)
    assert vb.tobytes() == r.vjp(J, c.v).tobytes()
    for t in range(N_DIR):
        assert r.vjp(J, c.v[t])[0].tobytes() == vb[t].tobytes(), t
    for n in (2, 3):
        assert r.vjp(J, c.v[:n]).tobytes() == vb[:n].tobytes(), n
    assert not vb[2].any() and vb[0].any() and vb[4].any()
    assert (2.0 * vb).tobytes() == r.vjp(J, 2.0 * c.v).tobytes()


@pytest.mark.parametrize("k", VARIANTS)
def test_zero_row_nodes_give_exact_zeros(red, k):
    r, c = red, red.c
    J = r.jac(k, True)
    computed = c.tangent_model(0, False)["computed"]
    zero = ~computed
    assert zero.any() and computed.any()
    R = J.fetch()
    assert not R[zero[c.rows]].any() and R[computed[c.rows]].any()
    assert not r.jvp(J, r.dtheta[k])[:, zero].any()
    assert not r.vjp(J, np.where(zero, c.v[0], 0.0)).any()                            # a cotangent on the zero rows alone


def test_relinearize_is_a_fresh_linearisation(red):
    r, c = red, red.c
    u2 = np.random.default_rng(31).uniform(-1.0, 1.0, c.E)
    for k, other in (("scale", "percell1"), ("percell3", "diagonal"), ("symmetric", "shared6")):
        M, arr, pc = r.bases[k]
        fresh = r.linearize(k, True, u2)
        J = r.linearize(other, True)           # at u, with another basis of the same M
        before = J.fetch()
        ud, bd, Bd = c.to_dev(u2), c.to_dev(c.b), None if arr is None else c.to_dev(arr)
        J.relinearize(ud.data_ptr(), 0 if Bd is None else Bd.data_ptr(), pc, bd.data_ptr(), c.stream())   # ... moved to u2 and basis k
        _torch().cuda.synchronize(c.dev)
        a, b = J.fetch(), fresh.fetch()
        assert a.tobytes() == b.tobytes() and a.tobytes() != before.tobytes()
        assert r.jvp(J, r.dtheta[k]).tobytes() == r.jvp(fresh, r.dtheta[k]).tobytes()
        assert J.nbytes == 8 * M * c.nnz and J.buffer_ptr and J.buffer_ptr != fresh.buffer_ptr
        fresh.release()
        J.release()
        with pytest.raises(ValueError, match="released"):
            J.launch_jvp(8, 8)


def test_shared_and_null_bases_are_their_per_cell_forms_bit_for_bit(red):
    r, c = red, red.c
    for k in ("diagonal", "shared6"):                                                 # shared = the same basis replicated per cell
        rep = np.ascontiguousarray(np.broadcast_to(r.bases[k][1][None], (c.E,) + r.bases[k][1].shape))
        J = r.linearize(k, True, basis=rep, per_cell=True)
        assert J.fetch().tobytes() == r.jac(k, True).fetch().tobytes(), k
        J.release()
    perm_dev = _resident_perm(c)                                                      # NULL = the fetched resident perm given explicitly
    assert perm_dev.tobytes() == c.perm.tobytes()
    J = r.linearize("scale", True, basis=perm_dev.reshape(c.E, 1, 9), per_cell=True)
    assert J.fetch().tobytes() == r.jac("scale", True).fetch().tobytes()
    J.release()


def _resident_perm(c):
    """the grid's resident permeability [E][9], fetched from the device"""
    import ctypes
    from ninpol_amd import _lib
    perm, dmag = np.empty((c.E, 9)), np.empty(c.E)
    _lib.check(_lib.load().nin_fields_get_permeability(c.grid._h, perm.ctypes.data_as(ctypes.c_void_p), dmag.ctypes.data_as(ctypes.c_void_p)))
    return perm


def test_the_object_keeps_its_linearisation_point_and_its_states():
    """after update_permeability to another K and a flag flip the object answers the same bits, while a fresh linearisation differs;
    the state errors of an object that was never linearised, and argument errors on a live one"""
    torch = _torch()
    from ninpol_amd import _lib
    from ninpol_amd.interpolator import GlsReducedJacobian
    c = Case("mixed")                          # its own Interpolator: the resident tables are rewritten
    r = Reduced(c)
    Js = {k: r.linearize(k, True) for k in ("scale", "percell3", "symmetric")}
    assert all(J.is_current() and J.stamp == (c.grid.field_updates, c.grid.geometry_updates, c.grid.flag_updates) for J in Js.values())
    before = {k: (r.jvp(J, r.dtheta[k]), r.vjp(J, c.v), J.fetch()) for k, J in Js.items()}
    K2 = c.perm * np.random.default_rng(7).uniform(1.5, 2.5, (c.E, 1))
    c.I.update_permeability(c.to_dev(K2.reshape(c.E, 3, 3)))
    flags = c.flag.astype(np.float64)
    neu = np.flatnonzero(c.flag)
    flags[neu[::2]] = 0.0                      # every other Neumann node becomes a Dirichlet node
    c.I.update_neumann_flags("u", c.to_dev(flags))
    torch.cuda.synchronize(c.dev)
    for k, J in Js.items():
        assert not J.is_current()
        assert r.jvp(J, r.dtheta[k]).tobytes() == before[k][0].tobytes() and r.vjp(J, c.v).tobytes() == before[k][1].tobytes()
        J2 = r.linearize(k, True)
        now = J2.fetch()
        assert J2.is_current() and np.abs(now - before[k][2]).max() > 1e-3 * np.abs(before[k][2]).max()
        J2.release()
    J = Js["scale"]
    with pytest.raises(_lib.NinpolError) as e:
        J.launch_jvp(8, 8, n=0)
    assert e.value.code == _lib.NIN_EINVAL
    with pytest.raises(_lib.NinpolError) as e:
        J.launch_vjp(0, 8)
    assert e.value.code == _lib.NIN_EINVAL
    raw = GlsReducedJacobian(c.grid, 6)
    with pytest.raises(_lib.NinpolError) as e:
        raw.launch_jvp(8, 8)
    assert e.value.code == _lib.NIN_ESTATE and raw.stamp == (-1, -1, -1)
    with pytest.raises(_lib.NinpolError) as e:
        raw.fetch()
    assert e.value.code == _lib.NIN_ESTATE
    with pytest.raises(ValueError, match="basis_ptr"):
        raw.relinearize(8)                     # six parameters and no basis
    raw.release()
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0                           # nothing of 80 bytes per entry was made on this path


def test_permeability_jacobian_with_a_basis():
    c = Case("mixed")
    r = Reduced(c)
    full = c.I.permeability_jacobian("u", c.u, c.b)
    V = np.ascontiguousarray(c.v.T)                                                   # (P, n)
    bases = {"scale": "scale", "diagonal": "diagonal", "symmetric": "symmetric", "percell3": r.bases["percell3"][1],
             "shared6": r.bases["shared6"][1].reshape(6, 3, 3)}
    for k, basis in bases.items():
        M, B = r.M(k), r.B(k)
        op = c.I.permeability_jacobian("u", c.u, c.b, basis=basis)
        assert op.shape == (c.P, M * c.E) and op.dtype == np.float64 and op.jacobian.nbytes == 8 * M * c.nnz
        A = op.to_scipy()
        assert A.shape == op.shape and A.nnz == M * c.nnz
        absA = abs(A)
        N = M * c.nnz
        X = np.ascontiguousarray(r.dtheta[k].reshape(N_DIR, M * c.E).T)               # (M E, n)
        for got, want, room in ((op.matvec(X[:, 0]), A @ X[:, 0], absA @ np.abs(X[:, 0])),
                                (op.rmatvec(V[:, 0]), A.T @ V[:, 0], absA.T @ np.abs(V[:, 0])),
                                (op.matmat(X), A @ X, absA @ np.abs(X)),
                                (op.rmatmat(V), A.T @ V, absA.T @ np.abs(V)),
                                (op @ X[:, 4], A @ X[:, 4], absA @ np.abs(X[:, 4])),
                                (op.T @ V[:, 4], A.T @ V[:, 4], absA.T @ np.abs(V[:, 4]))):
            assert got.shape == want.shape and np.all(np.isfinite(got))
            assert np.all(np.abs(got - want) <= 2 * (N + 2) * U * room) and np.abs(want).max() > 0
        assert op.matmat(X)[:, 1].tobytes() == op.matvec(X[:, 1]).tobytes()
        # the operator without a basis, composed with B on the host
        m = r.jvp_model(k, 0, True)
        got, want = op.matvec(X[:, 0]), full.matvec(RM.direction(B, r.dtheta[k][0]).reshape(-1))
        none = m["scale"] == 0
        assert not got[none].any() and not want[none].any()
        e = (np.abs(got - want)[~none] / m["scale"][~none]).max()
        a = r.vjp_model(k, 0, True)
        gt, wt = op.rmatvec(V[:, 0]).reshape(c.E, M), np.einsum("emk,ek->em", B, full.rmatvec(V[:, 0]).reshape(c.E, 9))
        zero = a["scale"] == 0
        assert not gt[zero].any() and not wt[zero].any()
        ev = (np.abs(gt - wt)[~zero] / a["scale"][~zero]).max()
        print(f"permeability_jacobian(basis={k}) against the basis=None operator composed with B: matvec {e:.2e}, rmatvec {ev:.2e}")
        assert e <= RJVP_RTOL + JVP_RTOL and ev <= RVJP_RTOL + VJP_RTOL
        assert jvp_err(got, m) <= RJVP_RTOL
        op.release()
        with pytest.raises(ValueError, match="released"):
            op.matvec(X[:, 0])
    full.release()


def test_cell_to_node_linearize_wrt_scale():
    """CellToNode.linearize(u, K, scale, wrt="scale") against the wrt="K" linearisation's jvp(dscale=...) and vjp(g)[2], and against
    forward_ad / backward of CellToNode(u, K, scale), at the margins of tests/test_gpu_gls_jacobian.py's linearize test"""
    torch = _torch()
    import torch.autograd.forward_ad as fwAD
    from ninpol_amd.interpolator import GlsReducedJacobian
    from ninpol_amd.torch_ops import CellToNode
    c = Case("mixed")                          # its own Interpolator: the op rewrites the resident permeability
    op = CellToNode(c.I, "u", "gls")
    rng = np.random.default_rng(9)
    s_np, ds_np, du_np = rng.uniform(0.5, 1.5, c.E), rng.uniform(-1.0, 1.0, c.E), rng.uniform(-1.0, 1.0, c.E)
    K0 = c.to_dev(c.perm.reshape(c.E, 3, 3))
    s0, ds0, u0, du0, g0 = c.to_dev(s_np), c.to_dev(ds_np), c.to_dev(c.u), c.to_dev(du_np), c.to_dev(c.v[0])
    perm = s_np[:, None] * c.perm
    dmag = GM.diff_mag_of(perm)
    absu = np.bincount(c.rows, weights=np.abs(c.u[c.esup]), minlength=c.P)
    room = TM.gls_tangent_model(c.grid, perm, dmag, c.flag, ds_np[:, None] * c.perm)["scale"] * absu
    none = room == 0

    linK = op.linearize(u0, K0, s0)
    lin = op.linearize(u0, K0, s0, wrt="scale")
    assert isinstance(lin.jacobian, GlsReducedJacobian) and lin.jacobian.nbytes == 8 * c.nnz and lin.jacobian.is_current()
    assert torch.equal(lin.value, linK.value)
    with fwAD.dual_level():
        want_s = fwAD.unpack_dual(op(u0, K0, fwAD.make_dual(s0, ds0))).tangent.cpu().numpy()
        want_us = fwAD.unpack_dual(op(fwAD.make_dual(u0, du0), K0, fwAD.make_dual(s0, ds0))).tangent.cpu().numpy()
    for tag, got, other in (("dscale", lin.jvp(dscale=ds0), linK.jvp(dscale=ds0)), ("du, dscale", lin.jvp(du0, dscale=ds0), linK.jvp(du0, dscale=ds0))):
        got, other = got.cpu().numpy(), other.cpu().numpy()
        want = want_s if tag == "dscale" else want_us
        assert got.shape == (c.P,) and not (got - want)[none].any() and not (got - other)[none].any()
        e1 = (np.abs(got - other)[~none] / room[~none]).max()
        e2 = (np.abs(got - want)[~none] / room[~none]).max()
        print(f'linearize(wrt="scale").jvp({tag}): against wrt="K" {e1:.2e}, against forward_ad {e2:.2e} of the row scale')
        assert e1 <= RJVP_RTOL + JVP_RTOL and e2 <= RJVP_RTOL + TANGENT_RTOL
    assert torch.equal(lin.jvp(du0), linK.jvp(du0))                                   # W du: the same kernel on the same weights
    both = lin.jvp(torch.stack([du0, du0 * 0.5]), dscale=torch.stack([ds0, ds0 * 0.5]))
    assert both.shape == (2, c.P) and torch.allclose(both[0], lin.jvp(du0, dscale=ds0), rtol=0, atol=1e-13)
    assert torch.equal(lin.jvp(dscale=torch.stack([ds0, ds0 * 0.5]))[0], lin.jvp(dscale=ds0))
    assert lin.jvp().shape == (c.P,) and not lin.jvp().any()
    with pytest.raises(ValueError, match="dK must be None"):
        lin.jvp(dK=K0)

    K, s, u = K0.clone().requires_grad_(), s0.clone().requires_grad_(), u0.clone().requires_grad_()
    (op(u, K, s) * g0).sum().backward()
    linK = op.linearize(u0, K0, s0)
    lin = op.linearize(u0, K0, s0, wrt="scale")
    gu, gK, gs = lin.vjp(g0)
    guK, _, gsK = linK.vjp(g0)
    assert gK is None and gs.shape == (c.E,) and torch.equal(gu, u.grad) and torch.equal(gu, guK)
    a = JM.vjp_model(c.grid, perm, dmag, c.flag, c.u, c.v[0])
    sc = a["scale_perm"] + a["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(perm))
    scale = 9 * np.abs(c.perm).max(axis=1) * sc                                       # (the scale of the existing linearize test)
    d1, d2 = np.abs((gs - gsK).cpu().numpy()), np.abs((gs - s.grad).cpu().numpy())
    assert not d1[sc == 0].any() and not d2[sc == 0].any()
    e1, e2 = (d1[sc > 0] / scale[sc > 0]).max(), (d2[sc > 0] / scale[sc > 0]).max()
    print(f'linearize(wrt="scale").vjp: against wrt="K" {e1:.2e}, against backward {e2:.2e} of the cell scale')
    assert e1 <= RVJP_RTOL + VJP_RTOL and e2 <= RVJP_RTOL + ADJOINT_RTOL
    gu2, gK2, gs2 = lin.vjp(torch.stack([g0, 2.0 * g0]))
    assert gK2 is None and gs2.shape == (2, c.E) and torch.equal(gs2[0], gs) and torch.equal(gs2[1], 2.0 * gs) and torch.equal(gu2[0], gu)
    lin.release()

    # IDW does not depend on K: W du, zeros for scale, and no buffer
    idw = CellToNode(c.I, "u", "idw")
    li = idw.linearize(u0, K0, s0, wrt="scale")
    assert li.jacobian is None and torch.equal(li.value, idw(u0))
    assert torch.equal(li.jvp(du0, dscale=ds0), idw(du0)) and not li.jvp(dscale=ds0).any()
    gu, gK, gs = li.vjp(g0)
    assert gK is None and gs.shape == (c.E,) and not gs.any()
