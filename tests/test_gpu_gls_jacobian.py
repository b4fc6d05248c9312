"""The GLS Jacobian in the permeability kept on the device: DevicePlan.linearize / GlsJacobian.launch_jvp / launch_vjp,
Interpolator.permeability_jacobian and CellToNode.linearize, held to the numpy model of tests/gls_jacobian_model.py (which
tests/test_gls_jacobian_model.py pins against central differences of the oracle), to the backward call bit for bit, and to each other
through a derived duality bound.

The meshes are those of tests/test_gpu_gls_tangent.py with the Neumann plane z = 0: rows of 1 to ~65 cells, cells of 4 to 8 nodes,
Dirichlet zero rows, Neumann rows, every adjoint bin on the Delaunay mesh, and P, E, nnz that are no multiples of 64 or 256.  Every
output buffer is NaN-filled before its launch and must come back finite.

Measured on an MI355X, worst over the four meshes and all variants (folded / explicit diff_mag, with / without neumann_values, n = 1
and n = 5), against the model:
  J . dK    per row, of the model's row scale:                        4.45e-13 (Delaunay; 9.0e-14 hex, 1.5e-13 mixed, 2.5e-14 tet)
  J^T . v   per cell, of scale_perm / scale_diff_mag (+ their fold):  8.64e-12 (Delaunay; 5.2e-13 hex, 3.2e-13 mixed, 3.6e-13 tet)
The bars are 10 x those, never looser than the 1e-8 at which the model itself is pinned.  The device duality gap measured 0 to 3.3e-16
absolute against derived bars of 4.9e-12 and more.
The Delaunay figures contain the lstsq MODEL's own distance from the exact derivative: against the 80-bit model of
tests/gls_derivative_exact.py (this file's u and b, one direction and one cotangent of its own) the lstsq model is 6.1e-13 (J . dK) and
1.02e-11 (J^T . v, grad_perm; 3.9e-12 grad_diff_mag) away on that mesh, the device 4.4e-15 to 9.0e-15 (J . dK) and 7.5e-14 / 4.3e-12
(J^T . v, grad_perm / grad_diff_mag) -- tests/test_gpu_gls_derivative_exact.py, profiles/r17.  The bars stay: they bound the distance
between the device and this model."""
import math

import numpy as np
import pytest

import gls_adjoint_model as GM
import gls_jacobian_model as JM
import gls_tangent_model as TM
from test_gpu_gls_tangent import ADJOINT_RTOL, MESHES, TANGENT_RTOL
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

JVP_RTOL = 4.5e-12
VJP_RTOL = 8.7e-11
assert JVP_RTOL <= 1e-8 and VJP_RTOL <= 1e-8
N_DIR = 5            # a chunk of four directions is crossed
MODELLED = (0, 4)    # the directions of a batch that are held to the model: one of the full chunk, and the one behind it
U = 2.0 ** -53


def _torch():
    import torch
    return torch


class Case:
    """one mesh on the device, a field, directions, and the models (computed once, lazily)"""

    def __init__(self, name):
        import ninpol_amd
        from ninpol_amd.interpolator import DevicePlan
        torch = _torch()
        self.name = name
        mesh = M.attach_fields(MESHES[name](), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
        self.I = I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=mesh)
        self.dev = torch.device("cuda", int(I.device))
        self.plan = DevicePlan(I, "u", "gls")
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        perm, dmag = I._perm_rows()
        self.perm, self.dmag = np.array(perm).reshape(self.E, 9), np.array(dmag)
        self.flag = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        rng = np.random.default_rng(23)
        self.u, self.b = rng.uniform(-1.0, 1.0, self.E), rng.uniform(-1.0, 1.0, self.P)
        self.dK = rng.uniform(-1, 1, (N_DIR, self.E, 9))
        self.ddm = rng.uniform(-1, 1, (N_DIR, self.E))
        self.v = rng.uniform(-1, 1, (N_DIR, self.P))
        self.dK[2], self.ddm[2], self.v[2] = 0.0, 0.0, 0.0          # a zero direction inside the batch
        self.ptr, self.esup = np.asarray(g.esup_ptr).astype(np.int64), np.asarray(g.esup).astype(np.int64)
        self.rows = np.repeat(np.arange(self.P), np.diff(self.ptr))
        self._jac, self._tan, self._adj = {}, {}, {}

    def stream(self):
        return _torch().cuda.current_stream(self.dev).cuda_stream

    def to_dev(self, a):
        return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def nan(self, *shape):
        torch = _torch()
        return torch.full(shape, float("nan"), dtype=torch.float64, device=self.dev)

    def linearize(self, with_b=True, u=None):
        ud, bd = self.to_dev(self.u if u is None else u), self.to_dev(self.b)
        J = self.plan.linearize(ud.data_ptr(), bd.data_ptr() if with_b else 0, self.stream())
        _torch().cuda.synchronize(self.dev)
        return J

    def jac(self, with_b=True):
        if with_b not in self._jac:
            self._jac[with_b] = self.linearize(with_b)
        return self._jac[with_b]

    def jvp(self, J, dK, ddm=None):
        """dK [k][E][9] (ddm [k][E] or None: folded) -> [k][P]"""
        dK = np.ascontiguousarray(dK).reshape(-1, self.E, 9)
        k = len(dK)
        d, dm = self.to_dev(dK), None if ddm is None else self.to_dev(np.reshape(ddm, (k, self.E)))
        out = self.nan(k, self.P)
        J.launch_jvp(d.data_ptr(), out.data_ptr(), k, 0 if dm is None else dm.data_ptr(), self.stream())
        _torch().cuda.synchronize(self.dev)
        out = out.cpu().numpy()
        assert np.all(np.isfinite(out)), "J . dK is not finite (or was not written)"
        return out

    def vjp(self, J, v, unfolded=False):
        """v [k][P] -> (grad_perm [k][E][9], grad_diff_mag [k][E] or None)"""
        v = np.ascontiguousarray(v).reshape(-1, self.P)
        k = len(v)
        vd = self.to_dev(v)
        gp, gd = self.nan(k, self.E, 9), self.nan(k, self.E) if unfolded else None
        J.launch_vjp(vd.data_ptr(), gp.data_ptr(), k, gd.data_ptr() if unfolded else 0, self.stream())
        _torch().cuda.synchronize(self.dev)
        gp, gd = gp.cpu().numpy(), gd.cpu().numpy() if unfolded else None
        assert np.all(np.isfinite(gp)) and (gd is None or np.all(np.isfinite(gd))), "J^T . v is not finite (or was not written)"
        return gp, gd

    def backward(self, grad_csr, gnws, unfolded, plan=None):
        g, gn = self.to_dev(grad_csr), None if gnws is None else self.to_dev(gnws)
        gp, gd = self.nan(self.E, 9), self.nan(self.E) if unfolded else None
        (plan or self.plan).launch_weights_backward(g.data_ptr(), gp.data_ptr(), gd.data_ptr() if unfolded else 0,
                                                    0 if gn is None else gn.data_ptr(), self.stream(), add_neumann=True)
        _torch().cuda.synchronize(self.dev)
        return gp.cpu().numpy(), (gd.cpu().numpy() if unfolded else None)

    def tangent_model(self, t, explicit):
        if (t, explicit) not in self._tan:
            self._tan[(t, explicit)] = TM.gls_tangent_model(self.grid, self.perm, self.dmag, self.flag, self.dK[t],
                                                            ddm=self.ddm[t] if explicit else None, add_neumann=True)
        return self._tan[(t, explicit)]

    def jvp_model(self, t, explicit, with_b):
        return JM.jvp_model(self.grid, self.perm, self.dmag, self.flag, self.u, self.dK[t], b=self.b if with_b else None,
                            tangent=self.tangent_model(t, explicit))

    def vjp_model(self, t, with_b):
        if (t, with_b) not in self._adj:
            self._adj[(t, with_b)] = JM.vjp_model(self.grid, self.perm, self.dmag, self.flag, self.u, self.v[t], b=self.b if with_b else None)
        return self._adj[(t, with_b)]


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module", params=sorted(MESHES))
def case(request):
    return get_case(request.param)


def jvp_err(got, m):
    """max over rows of |device - model| / the row's scale; where the scale is 0 both are exactly 0"""
    none = m["scale"] == 0
    assert not got[none].any() and not m["value"][none].any()
    return float((np.abs(got - m["value"])[~none] / m["scale"][~none]).max())


def vjp_err(c, gp, gd, m):
    """max over cells of |device - model| / the cell's scale: unfolded against scale_perm and scale_diff_mag, folded (gd None) against
    scale_perm + scale_diff_mag |d diff_mag / d K_dd|; where the scale is 0 both are exactly 0"""
    if gd is None:
        want, sc = m["folded"], m["scale_perm"] + m["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(c.perm))
    else:
        want, sc = m["grad_perm"], m["scale_perm"]
    d = np.abs(gp.reshape(c.E, 9) - want).max(axis=1)
    none = sc == 0
    assert not gp.reshape(c.E, 9)[none].any() and not d[none].any()
    e = float((d[~none] / sc[~none]).max())
    if gd is not None:
        sd = m["scale_diff_mag"]
        dd = np.abs(gd - m["grad_diff_mag"])
        assert not gd[sd == 0].any() and not dd[sd == 0].any()
        e = max(e, float((dd[sd > 0] / sd[sd > 0]).max()))
    return e


def test_jvp_against_the_model(case):
    c = case
    worst = 0.0
    for with_b in (True, False):
        J = c.jac(with_b)
        for explicit in (False, True):
            batch = c.jvp(J, c.dK, c.ddm if explicit else None)
            one = c.jvp(J, c.dK[0], c.ddm[0] if explicit else None)
            for tag, got, t in [("n=1", one[0], 0)] + [(f"n={N_DIR}[{t}]", batch[t], t) for t in MODELLED]:
                e = jvp_err(got, c.jvp_model(t, explicit, with_b))
                print(f"{c.name} jvp neumann_values={with_b} explicit_ddm={explicit} {tag}: {e:.2e} of the row scale")
                assert e <= JVP_RTOL
                worst = max(worst, e)
    print(f"{c.name}: jvp worst over the variants {worst:.3e}")
    m = c.jvp_model(0, False, True)
    top = np.abs(m["value"]).max()
    assert (m["scale"] == 0).any() and top > 0
    assert np.abs(c.jvp_model(0, True, True)["value"] - m["value"]).max() > 1e-6 * top      # the variants really differ
    assert np.abs(c.jvp_model(0, False, False)["value"] - m["value"]).max() > 1e-6 * top


def test_vjp_against_the_model(case):
    c = case
    worst = 0.0
    for with_b in (True, False):
        J = c.jac(with_b)
        for unfolded in (False, True):
            bp, bd = c.vjp(J, c.v, unfolded)
            op, od = c.vjp(J, c.v[0], unfolded)
            for tag, gp, gd, t in [("n=1", op[0], od[0] if unfolded else None, 0)] + \
                                  [(f"n={N_DIR}[{t}]", bp[t], bd[t] if unfolded else None, t) for t in MODELLED]:
                e = vjp_err(c, gp, gd, c.vjp_model(t, with_b))
                print(f"{c.name} vjp neumann_values={with_b} unfolded={unfolded} {tag}: {e:.2e} of the cell scale")
                assert e <= VJP_RTOL
                worst = max(worst, e)
    print(f"{c.name}: vjp worst over the variants {worst:.3e}")
    assert np.count_nonzero(c.vjp_model(0, True)["grad_diff_mag"]) > 0, "the eta chain is not exercised"


def test_vjp_of_ones_is_the_backward_call_bit_for_bit(case):
    c = case
    ones = np.ones(c.P)
    for with_b in (True, False):
        J = c.jac(with_b)
        for unfolded in (False, True):
            gp, gd = c.vjp(J, ones, unfolded)
            wp, wd = c.backward(c.u[c.esup], c.b if with_b else None, unfolded)
            assert gp[0].tobytes() == wp.tobytes(), (with_b, unfolded)
            assert not unfolded or gd[0].tobytes() == wd.tobytes()
            assert np.abs(wp).max() > 0


def test_determinism_batching_zero_and_linearity(case):
    c = case
    J = c.jac(True)
    for explicit in (False, True):
        ddm = c.ddm if explicit else None
        batch = c.jvp(J, c.dK, ddm)
        assert batch.tobytes() == c.jvp(J, c.dK, ddm).tobytes()                       # two calls agree
        for t in range(N_DIR):                                                        # a batch equals its members one by one
            assert c.jvp(J, c.dK[t], None if ddm is None else ddm[t])[0].tobytes() == batch[t].tobytes(), (explicit, t)
        for k in (2, 3):                                                              # ... and the shorter chunks
            assert c.jvp(J, c.dK[:k], None if ddm is None else ddm[:k]).tobytes() == batch[:k].tobytes(), (explicit, k)
        assert not batch[2].any() and batch[0].any() and batch[4].any()               # a zero direction: exact zeros
        twice = c.jvp(J, 2.0 * c.dK, None if ddm is None else 2.0 * ddm)
        assert (2.0 * batch).tobytes() == twice.tobytes()                             # 2 dK gives exactly twice
    for unfolded in (False, True):
        bp, bd = c.vjp(J, c.v, unfolded)
        ap, ad = c.vjp(J, c.v, unfolded)
        assert bp.tobytes() == ap.tobytes() and (not unfolded or bd.tobytes() == ad.tobytes())
        for t in range(N_DIR):
            op, od = c.vjp(J, c.v[t], unfolded)
            assert op[0].tobytes() == bp[t].tobytes() and (not unfolded or od[0].tobytes() == bd[t].tobytes()), (unfolded, t)
        for k in (2, 3):
            kp, kd = c.vjp(J, c.v[:k], unfolded)
            assert kp.tobytes() == bp[:k].tobytes() and (not unfolded or kd.tobytes() == bd[:k].tobytes()), (unfolded, k)
        assert not bp[2].any() and bp[0].any() and bp[4].any() and (not unfolded or not bd[2].any())
        tp, td = c.vjp(J, 2.0 * c.v, unfolded)
        assert (2.0 * bp).tobytes() == tp.tobytes() and (not unfolded or (2.0 * bd).tobytes() == td.tobytes())


def _seven(x):
    """seven inputs from the module's N_DIR: the five, and scaled copies of the first two"""
    return np.concatenate([x, 0.5 * x, -3.0 * x])[:7]


def test_a_batch_of_seven_equals_its_members_one_by_one():
    """a full chunk of four and a chunk of three behind it, both products, on the smallest mesh"""
    c = get_case("tet")
    J = c.jac(True)
    dK, ddm, v = _seven(c.dK), _seven(c.ddm), _seven(c.v)
    for explicit in (False, True):
        batch = c.jvp(J, dK, ddm if explicit else None)
        ones = np.stack([c.jvp(J, dK[t], ddm[t] if explicit else None)[0] for t in range(7)])
        assert batch.shape == (7, c.P) and batch[6].any() and batch.tobytes() == ones.tobytes(), explicit
    for unfolded in (False, True):
        bp, bd = c.vjp(J, v, unfolded)
        singles = [c.vjp(J, v[t], unfolded) for t in range(7)]
        assert bp.shape == (7, c.E, 9) and bp[6].any() and bp.tobytes() == np.stack([s[0][0] for s in singles]).tobytes(), unfolded
        assert not unfolded or bd.tobytes() == np.stack([s[1][0] for s in singles]).tobytes()


def test_zero_row_nodes_give_exact_zeros(case):
    c = case
    J = c.jac(True)
    computed = c.tangent_model(0, False)["computed"]
    zero = ~computed
    assert zero.any() and computed.any()
    contrib, fold = J.fetch()
    assert contrib.shape == (c.nnz, 10) and fold.shape == (c.E,) and np.all(np.isfinite(contrib)) and np.all(np.isfinite(fold))
    assert not contrib[zero[c.rows]].any() and contrib[computed[c.rows]].any()
    assert np.allclose(fold, GM.diff_mag_derivative(c.perm), rtol=8 * U, atol=0)      # the same five operations, each rounded once
    out = c.jvp(J, c.dK, c.ddm)
    assert not out[:, zero].any()
    gp, gd = c.vjp(J, np.where(zero, c.v[0], 0.0), True)                              # a cotangent on the zero rows alone
    assert not gp.any() and not gd.any()


def test_relinearize_is_a_fresh_linearisation(case):
    c = case
    u2 = np.random.default_rng(31).uniform(-1.0, 1.0, c.E)
    fresh = c.linearize(True, u2)
    J = c.linearize(True)                      # at u ...
    before = J.fetch()[0]
    ud, bd = c.to_dev(u2), c.to_dev(c.b)
    J.relinearize(ud.data_ptr(), bd.data_ptr(), c.stream())                           # ... moved to u2
    _torch().cuda.synchronize(c.dev)
    a, b = J.fetch(), fresh.fetch()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].tobytes() != before.tobytes()
    assert c.jvp(J, c.dK).tobytes() == c.jvp(fresh, c.dK).tobytes()
    assert J.nbytes == 80 * c.nnz + 8 * c.E and J.contrib_ptr and J.fold_ptr and J.contrib_ptr != fresh.contrib_ptr
    fresh.release()
    J.release()
    with pytest.raises(ValueError, match="released"):
        J.launch_jvp(8, 8)


def test_duality_on_the_device(case):
    """|<v, J dK> - <J^T v, dK>| <= 2 (N + 2) 2^-53 S with N = 10 nnz products per side and S = sum |v_p C[pos][k] dK| from the fetched
    buffer: the worst-case bound of two sums of N products, each product and each addition rounded once (the host's dot products are
    taken with math.fsum)"""
    c = case
    for with_b in (True, False):
        J = c.jac(with_b)
        contrib, fold = J.fetch()
        N = 10 * c.nnz
        for t in (0, 4):
            v, dK, ddm = c.v[t], c.dK[t], c.ddm[t]
            # unfolded: diff_mag a direction of its own
            out = c.jvp(J, dK, ddm)[0]
            gp, gd = c.vjp(J, v, True)
            lhs = math.fsum(v * out)
            rhs = math.fsum((gp[0] * dK).reshape(-1)) + math.fsum(gd[0] * ddm)
            S = math.fsum((np.abs(v[c.rows])[:, None] * np.abs(contrib[:, :9] * dK[c.esup])).reshape(-1)) + \
                math.fsum(np.abs(v[c.rows] * contrib[:, 9] * ddm[c.esup]))
            bar = 2 * (N + 2) * U * S
            print(f"{c.name} neumann_values={with_b} t={t} unfolded: gap {abs(lhs - rhs):.3e}, bar {bar:.3e}, S {S:.3e}")
            assert S > 0 and abs(lhs - rhs) <= bar
            # folded: ddm = fold tr dK on one side, fold acc[9] onto the diagonal on the other -- three more roundings a term, inside N + 2
            out = c.jvp(J, dK)[0]
            gp, _ = c.vjp(J, v, False)
            lhs = math.fsum(v * out)
            rhs = math.fsum((gp[0] * dK).reshape(-1))
            trabs = (np.abs(dK[:, 0]) + np.abs(dK[:, 4]) + np.abs(dK[:, 8])) * np.abs(fold)
            S = math.fsum((np.abs(v[c.rows])[:, None] * np.abs(contrib[:, :9] * dK[c.esup])).reshape(-1)) + \
                math.fsum(np.abs(v[c.rows] * contrib[:, 9]) * trabs[c.esup])
            bar = 2 * (N + 2) * U * S
            print(f"{c.name} neumann_values={with_b} t={t} folded: gap {abs(lhs - rhs):.3e}, bar {bar:.3e}")
            assert abs(lhs - rhs) <= bar


def test_the_object_is_independent_of_the_grids_backward_buffer():
    c = Case("tet")                            # a grid of its own: nothing has run on it
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0
    J = c.linearize(True)
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0                           # the object's buffer is not the grid's
    assert J.is_current() and J.stamp == (c.grid.field_updates, c.grid.geometry_updates, c.grid.flag_updates)
    before = c.jvp(J, c.dK)
    vbefore = c.vjp(J, c.v, True)
    rng = np.random.default_rng(5)
    c.backward(rng.uniform(-1, 1, c.nnz), rng.uniform(-1, 1, c.P), True)              # overwrites the grid's contribution buffer
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 80 * c.nnz
    assert c.jvp(J, c.dK).tobytes() == before.tobytes()
    after = c.vjp(J, c.v, True)
    assert after[0].tobytes() == vbefore[0].tobytes() and after[1].tobytes() == vbefore[1].tobytes()
    # the scratch goes -- bins, transpose index, the grid's buffer -- and the object still answers (the index is built again)
    c.grid.release_scratch()
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0 and not c.grid.has_transpose_index
    assert c.jvp(J, c.dK).tobytes() == before.tobytes()
    assert c.vjp(J, c.v, True)[0].tobytes() == vbefore[0].tobytes() and c.grid.has_transpose_index
    # argument errors on a live object, and the state error of one that was never linearised
    from ninpol_amd import _lib
    from ninpol_amd.interpolator import GlsJacobian
    with pytest.raises(_lib.NinpolError) as e:
        J.launch_jvp(8, 8, n=0)
    assert e.value.code == _lib.NIN_EINVAL
    with pytest.raises(_lib.NinpolError) as e:
        J.launch_vjp(0, 8)
    assert e.value.code == _lib.NIN_EINVAL
    raw = GlsJacobian(c.grid)
    with pytest.raises(_lib.NinpolError) as e:
        raw.launch_jvp(8, 8)
    assert e.value.code == _lib.NIN_ESTATE and raw.stamp == (-1, -1, -1)
    raw.release()


def test_the_object_keeps_its_linearisation_point():
    """after update_permeability to another K and a flag flip the object answers the same bits (the fold is a snapshot), while the
    backward call on the same grid now differs"""
    torch = _torch()
    c = Case("mixed")                          # its own Interpolator: the resident tables are rewritten
    J = c.linearize(True)
    ones = np.ones(c.P)
    jb = c.jvp(J, c.dK)
    vb = c.vjp(J, c.v, False)
    same = c.vjp(J, ones, False)[0][0]
    assert same.tobytes() == c.backward(c.u[c.esup], c.b, False)[0].tobytes()
    K2 = c.perm * np.random.default_rng(7).uniform(1.5, 2.5, (c.E, 1))
    c.I.update_permeability(c.to_dev(K2.reshape(c.E, 3, 3)))
    flags = c.flag.astype(np.float64)
    neu = np.flatnonzero(c.flag)
    flags[neu[::2]] = 0.0                      # every other Neumann node becomes a Dirichlet node
    c.I.update_neumann_flags("u", c.to_dev(flags))
    torch.cuda.synchronize(c.dev)
    assert not J.is_current() and c.grid.field_updates >= 1 and c.grid.flag_updates >= 1
    assert c.jvp(J, c.dK).tobytes() == jb.tobytes()
    va = c.vjp(J, c.v, False)
    assert va[0].tobytes() == vb[0].tobytes()
    assert c.vjp(J, ones, False)[0][0].tobytes() == same.tobytes()
    now = c.backward(c.u[c.esup], c.b, False)[0]
    assert np.abs(now - same).max() > 1e-3 * np.abs(same).max()
    # a new linearisation is taken at the new point
    J2 = c.linearize(True)
    assert J2.is_current() and c.vjp(J2, ones, False)[0][0].tobytes() == now.tobytes()


def test_permeability_jacobian():
    c = Case("mixed")
    with_b = c.I.permeability_jacobian("u", c.u, c.b)
    op = c.I.permeability_jacobian("u", c.u)
    assert op.shape == (c.P, 9 * c.E) and op.dtype == np.float64
    A = op.to_scipy()
    assert A.shape == op.shape and A.nnz == 9 * c.nnz
    absA = abs(A)
    N = 10 * c.nnz
    X = np.ascontiguousarray(c.dK.reshape(N_DIR, 9 * c.E).T)           # (9 E, k)
    V = np.ascontiguousarray(c.v.T)                                   # (P, k)
    for got, want, room in ((op.matvec(X[:, 0]), A @ X[:, 0], absA @ np.abs(X[:, 0])),
                            (op.rmatvec(V[:, 0]), A.T @ V[:, 0], absA.T @ np.abs(V[:, 0])),
                            (op.matmat(X), A @ X, absA @ np.abs(X)),
                            (op.rmatmat(V), A.T @ V, absA.T @ np.abs(V)),
                            (op @ X[:, 4], A @ X[:, 4], absA @ np.abs(X[:, 4])),
                            (op.T @ V[:, 4], A.T @ V[:, 4], absA.T @ np.abs(V[:, 4]))):
        assert got.shape == want.shape and np.all(np.isfinite(got))
        assert np.all(np.abs(got - want) <= 2 * (N + 2) * U * room) and np.abs(want).max() > 0
    assert op.matmat(X)[:, 1].tobytes() == op.matvec(X[:, 1]).tobytes()
    # against the per-call siblings, which factorise every node again: both are within their bars of the model
    m = c.jvp_model(0, False, False)
    dv, _ = c.I.permeability_tangent("u", c.dK[0].reshape(c.E, 3, 3), c.u)
    none = m["scale"] == 0
    assert not dv[none].any() and not op.matvec(X[:, 0])[none].any()
    e = (np.abs(op.matvec(X[:, 0]) - dv)[~none] / m["scale"][~none]).max()
    print(f"permeability_jacobian.matvec against permeability_tangent: {e:.2e} of the row scale")
    assert e <= JVP_RTOL + TANGENT_RTOL
    a = c.vjp_model(0, False)
    sc = a["scale_perm"] + a["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(c.perm))
    gk = c.I.permeability_gradient("u", c.v[0], c.u).reshape(c.E, 9)
    d = np.abs(op.rmatvec(V[:, 0]).reshape(c.E, 9) - gk).max(axis=1)
    assert not d[sc == 0].any()
    e = (d[sc > 0] / sc[sc > 0]).max()
    print(f"permeability_jacobian.rmatvec against permeability_gradient: {e:.2e} of the cell scale")
    assert e <= VJP_RTOL + ADJOINT_RTOL
    # the neumann values are in the other operator
    assert np.abs(with_b.matvec(X[:, 0]) - op.matvec(X[:, 0])).max() > 1e-6 * np.abs(op.matvec(X[:, 0])).max()
    assert jvp_err(with_b.matvec(X[:, 0]), c.jvp_model(0, False, True)) <= JVP_RTOL
    op.release()
    with_b.release()
    with pytest.raises(ValueError, match="released"):
        op.matvec(X[:, 0])


def test_cell_to_node_linearize():
    """CellToNode.linearize(u, K, scale): jvp against forward_ad of CellToNode(u, K, scale), vjp against its backward, for dual K, scale
    and u singly and together.  Both sides are within their bars of the model, whose scales measure the difference."""
    torch = _torch()
    import torch.autograd.forward_ad as fwAD
    from ninpol_amd.torch_ops import CellToNode
    c = Case("mixed")                          # its own Interpolator: the op rewrites the resident permeability
    dev = c.dev
    op = CellToNode(c.I, "u", "gls")
    rng = np.random.default_rng(9)
    s_np, ds_np, du_np = rng.uniform(0.5, 1.5, c.E), rng.uniform(-1.0, 1.0, c.E), rng.uniform(-1.0, 1.0, c.E)
    K0, dK0 = c.to_dev(c.perm.reshape(c.E, 3, 3)), c.to_dev(c.dK[0].reshape(c.E, 3, 3))
    s0, ds0, u0, du0 = c.to_dev(s_np), c.to_dev(ds_np), c.to_dev(c.u), c.to_dev(du_np)
    g0 = c.to_dev(c.v[0])
    perm = s_np[:, None] * c.perm
    dmag = GM.diff_mag_of(perm)
    absu = np.bincount(c.rows, weights=np.abs(c.u[c.esup]), minlength=c.P)

    lin = op.linearize(u0, K0, s0)
    assert lin.jacobian.is_current()
    assert torch.equal(lin.value, op(u0, K0, s0))          # (the call makes scale * K resident again: the same point, a later stamp)
    for mask in range(1, 8):
        dual_K, dual_s, dual_u = bool(mask & 1), bool(mask & 2), bool(mask & 4)
        with fwAD.dual_level():
            out = op(fwAD.make_dual(u0, du0) if dual_u else u0, fwAD.make_dual(K0, dK0) if dual_K else K0,
                     fwAD.make_dual(s0, ds0) if dual_s else s0)
            want = fwAD.unpack_dual(out).tangent.cpu().numpy()
        got = lin.jvp(du0 if dual_u else None, dK0 if dual_K else None, ds0 if dual_s else None)
        assert got.shape == (c.P,)
        got = got.cpu().numpy()
        if not (dual_K or dual_s):
            assert got.tobytes() == want.tobytes()                                    # W du: the same kernel on the same weights
            continue
        tperm = (s_np[:, None] * c.dK[0] if dual_K else 0.0) + (ds_np[:, None] * c.perm if dual_s else 0.0)
        room = TM.gls_tangent_model(c.grid, perm, dmag, c.flag, tperm)["scale"] * absu
        none = room == 0
        assert not (got - want)[none].any()
        e = (np.abs(got - want)[~none] / room[~none]).max()
        print(f"linearize().jvp against forward_ad, dual K={dual_K} scale={dual_s} u={dual_u}: {e:.2e} of the row scale")
        assert e <= JVP_RTOL + TANGENT_RTOL                 # (with a dual u both sides add the same W du, one rounding each)
    # a leading batch dimension, every argument
    both = lin.jvp(torch.stack([du0, du0 * 0.5]), torch.stack([dK0, dK0 * 0.5]), torch.stack([ds0, ds0 * 0.5]))
    assert both.shape == (2, c.P) and torch.allclose(both[0], lin.jvp(du0, dK0, ds0), rtol=0, atol=1e-13)
    assert torch.equal(lin.jvp(dK=torch.stack([dK0, dK0 * 0.5]))[0], lin.jvp(dK=dK0))
    assert lin.jvp().shape == (c.P,) and not lin.jvp().any()
    with pytest.raises(ValueError, match="batch"):
        lin.jvp(du0, torch.stack([dK0, dK0]))

    K, s, u = K0.clone().requires_grad_(), s0.clone().requires_grad_(), u0.clone().requires_grad_()
    (op(u, K, s) * g0).sum().backward()
    lin = op.linearize(u0, K0, s0)             # (the backward pass above read what forward made resident: the same point)
    gu, gK, gs = lin.vjp(g0)
    assert gK.shape == K.grad.shape and gs.shape == (c.E,) and torch.equal(gu, u.grad)
    a = JM.vjp_model(c.grid, perm, dmag, c.flag, c.u, c.v[0])
    sc = a["scale_perm"] + a["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(perm))
    bar = VJP_RTOL + ADJOINT_RTOL
    d = np.abs((gK - K.grad).reshape(c.E, 9).cpu().numpy()).max(axis=1)
    ds_ = np.abs((gs - s.grad).cpu().numpy())
    assert not d[sc == 0].any() and not ds_[sc == 0].any()
    e_K = (d[sc > 0] / (s_np * sc)[sc > 0]).max()
    e_s = (ds_[sc > 0] / (9 * np.abs(c.perm).max(axis=1) * sc)[sc > 0]).max()
    print(f"linearize().vjp against backward: K {e_K:.2e}, scale {e_s:.2e} of the cell scale")
    assert e_K <= bar and e_s <= bar
    gu2, gK2, gs2 = lin.vjp(torch.stack([g0, 2.0 * g0]))
    assert gK2.shape == (2,) + tuple(K.shape) and torch.equal(gK2[0], gK) and torch.equal(gK2[1], 2.0 * gK) and torch.equal(gu2[0], gu)
    assert gs2.shape == (2, c.E) and torch.allclose(gs2[1], 2.0 * gs, rtol=1e-14, atol=0)
    # K alone: no scale, no gradient for it
    lin1 = op.linearize(u0, K0)
    assert lin1.vjp(g0)[2] is None and lin1.jvp(dK=dK0.reshape(c.E, 9)).shape == (c.P,)
    with pytest.raises(ValueError, match="dscale"):
        lin1.jvp(dscale=ds0)
    with pytest.raises(ValueError, match="shape"):
        op.linearize(torch.stack([u0, u0]), K0)

    # IDW does not depend on K: W du, zeros for K and scale, and no buffer
    idw = CellToNode(c.I, "u", "idw")
    li = idw.linearize(u0, K0, s0)
    assert li.jacobian is None and torch.equal(li.value, idw(u0))
    assert torch.equal(li.jvp(du0, dK0, ds0), idw(du0)) and not li.jvp(dK=dK0).any()
    gu, gK, gs = li.vjp(g0)
    assert not gK.any() and not gs.any() and gK.shape == K0.shape
    uu = u0.clone().requires_grad_()
    (idw(uu) * g0).sum().backward()
    assert torch.equal(gu, uu.grad)
