"""The directional derivative of the GLS weights in the permeability, on the device: DevicePlan.launch_weights_tangent,
Interpolator.permeability_tangent and CellToNode(u, K, scale) under torch.autograd.forward_ad, held to the numpy model of
tests/gls_tangent_model.py (which tests/test_gls_tangent_model.py pins against central differences of the oracle) and, through the
duality <ghat, dd> + <ghat_nws, dnws> = <Kbar, dK>, to the adjoint kernel.

The meshes are those of tests/test_gpu_gls_adjoint.py, Neumann plane z = 0 included: Neumann rows, the neumann_ws fold, zero-row corners
and Dirichlet rows are all in, and the random-cloud Delaunay mesh populates all four bins of the kernel.

A row's tangent is a difference of two terms, dr_i / rho and r_i drho / rho^2: the error is measured per row against the model's
max_i (|dr_i| / rho + |r_i| |drho| / rho^2) + |dnws|."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the child process of test_forced_global_class: the paths tests/conftest.py sets up
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import gls_adjoint_model as GM  # noqa: E402
import gls_tangent_model as TM  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu

# Device tangent against the model, per row, relative to the row's scale above.  Measured on an MI355X over the four meshes below and all
# call variants (add_neumann on / off, with / without tangent_neumann_ws, folded / explicit d diff_mag): 1.80e-12 at worst (the Delaunay
# mesh, folded; 1.4e-12 to 1.6e-12 there with an explicit d diff_mag; 1.6e-13, 2.5e-13 and 1.2e-13 on the hex, mixed and tet meshes;
# DESIGN.md 4.12).  The bar is 10 x the worst value; it may never be looser than the 1e-8 at which the model itself is pinned.  The
# duality gap against the adjoint kernel measured 0 to 8.5e-15 absolute (|<Kbar, dK>| 0.05 to 2.5), far inside its derived bar.
# The Delaunay figures are the lstsq MODEL's own distance from the exact derivative, not the kernel's: against the 80-bit model of
# tests/gls_derivative_exact.py (the same inputs) the lstsq model is 1.81e-12 (folded) and 1.63e-12 (explicit) away on that mesh, the
# device 3.4e-14 and 2.7e-14 (tests/test_gpu_gls_derivative_exact.py, profiles/r17); on the three other meshes the model is 1.2e-13 to
# 2.5e-13 away, the device 9e-15 to 5.3e-14.  The bar stays: it bounds the distance between the device and this model.
TANGENT_RTOL = 1.8e-11
ADJOINT_RTOL = 5.1e-11      # tests/test_gpu_gls_adjoint.py: the adjoint kernel's bar, for the derived bar of the duality test
assert TANGENT_RTOL <= 1e-8

MESHES = {
    "hex": lambda: M.hex_mesh(5, jitter=0.1, seed=1),
    "tet": lambda: M.tet_mesh(3, jitter=0.1, seed=3),
    "mixed": lambda: M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2),
    "delaunay": lambda: M.delaunay_tet_mesh(6, seed=4, lattice="random"),
}


def _torch():
    import torch
    return torch


class Case:
    """one mesh on the device, its tables on the host, a direction and the model's answers (computed once, lazily)"""

    def __init__(self, name):
        import ninpol_amd
        from ninpol_amd.interpolator import DevicePlan
        self.name = name
        mesh = M.attach_fields(MESHES[name](), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
        self.I = I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=mesh)
        self.plan = DevicePlan(I, "u", "gls")
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        perm, dmag = I._perm_rows()
        self.perm, self.dmag = np.array(perm).reshape(self.E, 9), np.array(dmag)
        self.flag = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        self.dK = np.random.default_rng(1).uniform(-1, 1, (self.E, 9))
        self.ddm = np.random.default_rng(2).uniform(-1, 1, self.E)
        rng = np.random.default_rng(17)
        self.ghat = rng.uniform(-1.0, 1.0, self.nnz)
        self.gnws = rng.uniform(-1.0, 1.0, self.P)
        ptr = np.asarray(g.esup_ptr)
        self.ptr, self.esup = ptr, np.asarray(g.esup)
        self.rows = np.repeat(np.arange(self.P), np.diff(ptr))
        self._models = {}

    def model(self, add_neumann=True, explicit=False):
        key = (add_neumann, explicit)
        if key not in self._models:
            self._models[key] = TM.gls_tangent_model(self.grid, self.perm, self.dmag, self.flag, self.dK,
                                                     ddm=self.ddm if explicit else None, add_neumann=add_neumann)
        return self._models[key]

    def device(self, add_neumann=True, with_nws=True, explicit=False, dK=None, ddm=None):
        """(tangent_csr [k][nnz], tangent_neumann_ws [k][P] or None) from DevicePlan.launch_weights_tangent; dK [E][9] or [k][E][9]"""
        torch = _torch()
        dev = torch.device("cuda", int(self.I.device))
        dK = np.ascontiguousarray(self.dK if dK is None else dK).reshape(-1, self.E, 9)
        k = len(dK)
        d = torch.from_numpy(dK).to(dev)
        dm = None
        if explicit:
            dm = torch.from_numpy(np.ascontiguousarray(self.ddm if ddm is None else ddm).reshape(k, self.E)).to(dev)
        out = torch.full((k, self.nnz), float("nan"), dtype=torch.float64, device=dev)     # NaN: every entry must be written
        nws = torch.full((k, self.P), float("nan"), dtype=torch.float64, device=dev) if with_nws else None
        self.plan.launch_weights_tangent(d.data_ptr(), out.data_ptr(), k, dm.data_ptr() if explicit else 0, nws.data_ptr() if with_nws else 0,
                                         torch.cuda.current_stream(dev).cuda_stream, add_neumann=add_neumann)
        torch.cuda.synchronize(dev)
        return out.cpu().numpy(), (nws.cpu().numpy() if with_nws else None)

    def backward(self, unfolded):
        torch = _torch()
        dev = torch.device("cuda", int(self.I.device))
        g, gn = torch.from_numpy(self.ghat).to(dev), torch.from_numpy(self.gnws).to(dev)
        gp = torch.full((self.E, 9), float("nan"), dtype=torch.float64, device=dev)
        gd = torch.full((self.E,), float("nan"), dtype=torch.float64, device=dev) if unfolded else None
        self.plan.launch_weights_backward(g.data_ptr(), gp.data_ptr(), gd.data_ptr() if unfolded else 0, gn.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream, add_neumann=True)
        torch.cuda.synchronize(dev)
        return gp.cpu().numpy(), (gd.cpu().numpy() if unfolded else None)


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module", params=sorted(MESHES))
def case(request):
    return get_case(request.param)


def row_err(c, dev_csr, dev_nws, m):
    """max over rows of |device - model| / the row's scale, over the row's entries and its neumann_ws; where the scale is 0 both are
    exactly 0"""
    assert np.all(np.isfinite(dev_csr)), "the device result is not finite (or was not written)"
    scale = m["scale"]
    none = scale == 0
    d = np.zeros(c.P)
    np.maximum.at(d, c.rows, np.abs(dev_csr - m["tangent"]))
    assert not dev_csr[none[c.rows]].any() and not m["tangent"][none[c.rows]].any()
    if dev_nws is not None:
        assert np.all(np.isfinite(dev_nws)), "tangent_neumann_ws is not finite (or was not written)"
        assert not dev_nws[none].any() and not m["tangent_neumann_ws"][none].any()
        assert not dev_nws[c.flag == 0].any()
        d = np.maximum(d, np.abs(dev_nws - m["tangent_neumann_ws"]))
    return float((d[~none] / scale[~none]).max())


def check(tag, c, got, m):
    e = row_err(c, got[0][0], None if got[1] is None else got[1][0], m)
    print(f"{tag}: {e:.2e} of the row scale")
    assert e <= TANGENT_RTOL, (tag, e)
    return e


def test_against_the_model(case):
    """every variant: add_neumann on / off, with / without tangent_neumann_ws, d diff_mag folded / explicit"""
    m = case.model()
    assert np.count_nonzero(m["tangent_neumann_ws"]) > 0 and not m["computed"].all() and (m["scale"] == 0).any()
    worst = 0.0
    for add_neumann in (True, False):
        for explicit in (False, True):
            mm = case.model(add_neumann, explicit)
            for with_nws in (True, False):
                got = case.device(add_neumann, with_nws, explicit)
                worst = max(worst, check(f"{case.name} add_neumann={add_neumann} explicit_ddm={explicit} nws={with_nws}", case, got, mm))
    print(f"{case.name}: worst over the variants {worst:.2e}")
    # the variants really differ
    top = np.abs(m["tangent"]).max()
    assert np.abs(case.model(False)["tangent"] - m["tangent"]).max() > 1e-6 * top
    assert np.abs(case.model(True, True)["tangent"] - m["tangent"]).max() > 1e-6 * top


def test_duality_with_the_adjoint_kernel(case):
    """<ghat, dd> + <ghat_nws, dnws> = <Kbar, dK> (+ <etabar, ddm> unfolded), both sides from the device.  The bar is what the two kernels'
    own bars allow: ADJOINT_RTOL on every cell's gradient against its absolute-contribution scale, TANGENT_RTOL on every row's tangent
    against its scale."""
    c = case
    adj = GM.gls_adjoint_model(c.grid, c.perm, c.dmag, c.flag, c.ghat, add_neumann=True, grad_neumann_ws=c.gnws)
    rowsum = np.bincount(c.rows, weights=np.abs(c.ghat), minlength=c.P) + np.abs(c.gnws)
    dkmax = np.abs(c.dK).max(axis=1)
    for unfolded in (False, True):
        m = c.model(True, unfolded)
        gp, gd = c.backward(unfolded)
        dd, dn = c.device(True, True, unfolded)
        lhs = c.ghat @ dd[0] + c.gnws @ dn[0]
        if unfolded:
            rhs = (gp * c.dK).sum() + gd @ c.ddm
            bar = ADJOINT_RTOL * ((9 * adj["scale_perm"] * dkmax).sum() + (adj["scale_diff_mag"] * np.abs(c.ddm)).sum())
        else:
            rhs = (gp * c.dK).sum()
            sc = adj["scale_perm"] + adj["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(c.perm))
            bar = ADJOINT_RTOL * (9 * sc * dkmax).sum()
        bar += TANGENT_RTOL * (m["scale"] * rowsum).sum()
        print(f"{c.name} {'unfolded' if unfolded else 'folded'}: duality gap {abs(lhs - rhs):.3e}, bar {bar:.3e}, |<Kbar, dK>| {abs(rhs):.3e}")
        assert abs(rhs) > 0 and abs(lhs - rhs) <= bar


def test_determinism_batching_zero_and_linearity(case):
    c = case
    a, b = c.device(), c.device()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # three directions in one call = three single calls, bit for bit (one factorisation, the same tail per direction)
    rng = np.random.default_rng(8)
    three = np.stack([c.dK, rng.uniform(-1, 1, (c.E, 9)), np.zeros((c.E, 9))])
    ddm3 = np.stack([c.ddm, rng.uniform(-1, 1, c.E), np.zeros(c.E)])
    for explicit in (False, True):
        batch = c.device(explicit=explicit, dK=three, ddm=ddm3)
        assert batch[0].shape == (3, c.nnz) and batch[1].shape == (3, c.P)
        for t in range(3):
            one = c.device(explicit=explicit, dK=three[t], ddm=ddm3[t])
            assert one[0][0].tobytes() == batch[0][t].tobytes() and one[1][0].tobytes() == batch[1][t].tobytes()
        # a zero direction: exactly zero
        assert not batch[0][2].any() and not batch[1][2].any()
        assert batch[0][0].any() and batch[0][1].any()
    # linearity: 2 dK gives twice the result BIT FOR BIT -- dK enters through products and sums only, and doubling commutes with each
    twice = c.device(dK=2.0 * c.dK)
    assert (2.0 * a[0]).tobytes() == twice[0].tobytes() and (2.0 * a[1]).tobytes() == twice[1].tobytes()


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    plan = c.grid.gls_adjoint_plan()
    print(f"delaunay: bins {plan}")
    assert list(plan.values()) == [59, 139, 321, 40] and sum(plan.values()) == c.P


CHILD = """the hexahedron mesh with every node in the global-scratch class (NIN_GLS_ADJ_FORCE_GLOBAL=1)"""


def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    got = c.device()                        # (the tangent call makes the bins itself)
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    check("hex, forced global", c, got, c.model())
    check("hex, forced global, explicit ddm, add_neumann=False", c, c.device(False, True, True), c.model(False, True))
    again = c.device()
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    print("CHILD OK")


def test_forced_global_class():
    """the same comparison with every system in global-memory scratch, in a fresh process (the switch is read when the bins are made)"""
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


def test_a_tangent_only_user_pays_no_contribution_buffer():
    c = Case("tet")                         # a grid of its own: nothing has run on it
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0
    got = c.device()
    check("tet, fresh grid", c, got, get_case("tet").model())
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0 and not c.grid.has_transpose_index
    # a backward call afterwards makes the buffer and still matches its model
    gp, gd = c.backward(True)
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 80 * c.nnz
    adj = GM.gls_adjoint_model(c.grid, c.perm, c.dmag, c.flag, c.ghat, add_neumann=True, grad_neumann_ws=c.gnws)
    for got_, key, sk in ((gp, "grad_perm", "scale_perm"), (gd, "grad_diff_mag", "scale_diff_mag")):
        sc = adj[sk]
        d = np.abs(got_.reshape(c.E, -1) - adj[key].reshape(c.E, -1)).max(axis=1)
        assert np.all(np.isfinite(got_)) and not d[sc == 0].any() and (d[sc > 0] / sc[sc > 0]).max() <= ADJOINT_RTOL
    again = c.device()
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    # both go with the scratch, and come back
    c.grid.release_scratch()
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0
    again = c.device()
    assert again[0].tobytes() == got[0].tobytes() and c.grid._scalar("gls_adjoint_contrib_bytes") == 0


def test_a_plan_of_another_method_is_refused():
    from ninpol_amd.interpolator import DevicePlan
    c = get_case("tet")
    with pytest.raises(ValueError, match="GLS only"):
        DevicePlan(c.I, "u", "idw").launch_weights_tangent(8, 8)


def _row_sums(c, w, u):
    """[k][P]: sum over the row's entries of w[k or broadcast][pos] * u[k][esup[pos]]"""
    w, u = np.atleast_2d(w), np.atleast_2d(u)
    return np.stack([np.bincount(c.rows, weights=w[f % len(w)] * u[f][c.esup], minlength=c.P) for f in range(len(u))])


def test_permeability_tangent_against_the_model():
    c = get_case("mixed")
    rng = np.random.default_rng(3)
    u2 = rng.uniform(-1.0, 1.0, (2, c.E))
    dK2 = np.stack([c.dK, rng.uniform(-1, 1, (c.E, 9))])
    m2 = [c.model(), TM.gls_tangent_model(c.grid, c.perm, c.dmag, c.flag, dK2[1])]
    ucell = np.asarray(c.I.cells_data[c.I.variable_to_index["cells"]["u"]])[:c.E]
    for tag, dK, uu, arg, models in (("k = 2", dK2, u2, u2, m2), ("one direction, the cell variable", dK2[0], ucell[None], None, m2[:1])):
        dv, dn = c.I.permeability_tangent("u", dK.reshape(dK.shape[:-1] + (3, 3)), arg)
        want_shape = (2, c.P) if dK.ndim == 3 else (c.P,)
        assert dv.shape == want_shape and dn.shape == want_shape and dv.dtype == np.float64
        dv, dn = np.atleast_2d(dv), np.atleast_2d(dn)
        for f, m in enumerate(models):
            expect = _row_sums(c, m["tangent"], uu[f])[0]
            room = m["scale"] * _row_sums(c, np.ones(c.nnz), np.abs(uu[f]))[0]
            none = room == 0
            assert not dv[f][none].any() and not expect[none].any()
            e_v = (np.abs(dv[f] - expect)[~none] / room[~none]).max()
            e_n = (np.abs(dn[f] - m["tangent_neumann_ws"])[m["scale"] > 0] / m["scale"][m["scale"] > 0]).max()
            print(f"permeability_tangent, {tag}, field {f}: node values {e_v:.2e}, neumann_ws {e_n:.2e}")
            assert e_v <= TANGENT_RTOL and e_n <= TANGENT_RTOL and not dn[f][m["scale"] == 0].any()
    with pytest.raises(ValueError):
        c.I.permeability_tangent("u", c.dK)
    with pytest.raises(ValueError):
        c.I.permeability_tangent("u", dK2.reshape(2, c.E, 3, 3), u2[0])
    # apply() really moves that way: one central difference through the library's own update_permeability() and apply()
    h = 1e-5
    vals = []
    try:
        for sgn in (+1, -1):
            c.I.update_permeability(c.perm + sgn * h * c.dK)
            vals.append(c.I.apply("u", "gls", values=u2))
    finally:
        c.I.update_permeability(c.perm)
    dv, dn = c.I.permeability_tangent("u", np.stack([c.dK, c.dK]).reshape(2, c.E, 3, 3), u2)
    fd_v, fd_n = (vals[0][0] - vals[1][0]) / (2 * h), (vals[0][1] - vals[1][1]) / (2 * h)
    assert np.abs(fd_v - dv).max() <= 1e-6 * np.abs(dv).max() and np.abs(fd_n - dn[0]).max() <= 1e-6 * np.abs(dv).max()


def test_torch_forward_ad():
    """CellToNode(u, K, scale) under forward_ad.dual_level() on the mixed mesh, k = 2 fields: every combination of dual inputs"""
    torch = _torch()
    import torch.autograd.forward_ad as fwAD
    from ninpol_amd.torch_ops import CellToNode, _GlsWeightsFn
    c = Case("mixed")                       # its own Interpolator: the op rewrites the resident permeability
    dev = torch.device("cuda", int(c.I.device))
    op = CellToNode(c.I, "u", "gls")
    rng = np.random.default_rng(9)
    u_np, du_np = rng.uniform(-1.0, 1.0, (2, c.E)), rng.uniform(-1.0, 1.0, (2, c.E))
    s_np, ds_np = rng.uniform(0.5, 1.5, c.E), rng.uniform(-1.0, 1.0, c.E)
    v = torch.from_numpy(rng.uniform(-1.0, 1.0, (2, c.P))).to(dev)
    K0 = torch.from_numpy(c.perm.reshape(c.E, 3, 3).copy()).to(dev)
    dK0 = torch.from_numpy(c.dK.reshape(c.E, 3, 3).copy()).to(dev)
    s0, ds0 = torch.from_numpy(s_np).to(dev), torch.from_numpy(ds_np).to(dev)
    u0, du0 = torch.from_numpy(u_np).to(dev), torch.from_numpy(du_np).to(dev)

    def grads():
        K, s, u = K0.clone().requires_grad_(), s0.clone().requires_grad_(), u0.clone().requires_grad_()
        (op(u, K, s) * v).sum().backward()
        return K.grad, s.grad, u.grad

    before = grads()
    plain = op(u0, K0, s0)
    w_dev = torch.empty(c.nnz, dtype=torch.float64, device=dev)
    nws_dev = torch.empty(c.P, dtype=torch.float64, device=dev)
    op.plan.launch(w_dev.data_ptr(), nws_dev.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)   # the weights of scale * K
    torch.cuda.synchronize(dev)
    w_np = w_dev.cpu().numpy()
    perm = s_np[:, None] * c.perm                       # one multiplication per entry, as update_permeability forms it
    worst = 0.0
    for mask in range(1, 8):
        dual_K, dual_s, dual_u = bool(mask & 1), bool(mask & 2), bool(mask & 4)
        with fwAD.dual_level():
            K = fwAD.make_dual(K0, dK0) if dual_K else K0
            s = fwAD.make_dual(s0, ds0) if dual_s else s0
            u = fwAD.make_dual(u0, du0) if dual_u else u0
            out = op(u, K, s)
            primal, tangent = fwAD.unpack_dual(out)
            assert torch.equal(primal, plain)           # the primal output is the non-dual call's, bit for bit
            assert tangent is not None and tangent.shape == (2, c.P)
            tangent = tangent.cpu().numpy()
        tperm = (s_np[:, None] * c.dK if dual_K else 0.0) + (ds_np[:, None] * c.perm if dual_s else 0.0)
        expect, room = np.zeros((2, c.P)), np.zeros((2, c.P))
        if dual_K or dual_s:
            m = TM.gls_tangent_model(c.grid, perm, GM.diff_mag_of(perm), c.flag, tperm)
            expect += _row_sums(c, m["tangent"], u_np)
            room += TANGENT_RTOL * m["scale"] * _row_sums(c, np.ones(c.nnz), np.abs(u_np))
        if dual_u:                                      # W du on the device's own weights: only the order of a row's sum may differ
            expect += _row_sums(c, w_np, du_np)
            room += 1e-14 * _row_sums(c, np.abs(w_np), np.abs(du_np))
        none = room == 0
        assert not tangent[none].any() and not expect[none].any()
        e = (np.abs(tangent - expect)[~none] / room[~none]).max()
        worst = max(worst, e)
        print(f"torch forward_ad, dual K={dual_K} scale={dual_s} u={dual_u}: {e:.2e} of the allowed error")
        assert e <= 1.0
    # K alone, no scale
    with fwAD.dual_level():
        tangent = fwAD.unpack_dual(op(u0, fwAD.make_dual(K0, dK0))).tangent.cpu().numpy()
    m = c.model()
    room = TANGENT_RTOL * m["scale"] * _row_sums(c, np.ones(c.nnz), np.abs(u_np))
    assert np.all(np.abs(tangent - _row_sums(c, m["tangent"], u_np)) <= room)
    # weights_of: (dW, dneumann_ws) themselves
    with fwAD.dual_level():
        w, nws = op.weights_of(fwAD.make_dual(K0, dK0))
        dw, dn = fwAD.unpack_dual(w).tangent.cpu().numpy(), fwAD.unpack_dual(nws).tangent.cpu().numpy()
    assert row_err(c, dw, dn, m) <= TANGENT_RTOL
    # backward is what it was, bit for bit
    after = grads()
    assert all(torch.equal(a, b) for a, b in zip(before, after))

    # IDW does not depend on K: a zero tangent from K and scale, W du from u
    op_idw = CellToNode(c.I, "u", "idw")
    with fwAD.dual_level():
        out = op_idw(u0, fwAD.make_dual(K0, dK0), fwAD.make_dual(s0, ds0))
        primal, tangent = fwAD.unpack_dual(out)
        assert torch.equal(primal, op_idw(u0)) and (tangent is None or not tangent.any())
        out = op_idw(fwAD.make_dual(u0, du0), fwAD.make_dual(K0, dK0))
        assert torch.equal(fwAD.unpack_dual(out).tangent, op_idw(du0))

    # jvp after an intervening update refuses, as backward does (autograd itself calls jvp right behind forward: a later caller)
    ctx = types.SimpleNamespace(op=op, stamp=op._stamp(), saved_tensors=(K0.reshape(c.E, 9), None))
    dw, dn = _GlsWeightsFn.jvp(ctx, dK0, None, None)
    assert dw.shape == (c.nnz,) and dn.shape == (c.P,)
    c.I.update_permeability(K0)
    with pytest.raises(RuntimeError, match="field_updates"):
        _GlsWeightsFn.jvp(ctx, dK0, None, None)
    K2 = K0.clone().requires_grad_()
    out2 = op(u0, K2)
    c.I.update_permeability(K0)
    with pytest.raises(RuntimeError, match="field_updates"):
        (out2 * v).sum().backward()


if __name__ == "__main__":
    _child()
