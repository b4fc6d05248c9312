"""The directional derivative of the GLS weights in the node coordinates, on the device: DevicePlan.launch_weights_tangent_points,
Interpolator.points_tangent and the torch op CellToNode(u, points=...) under forward_ad, held to the 80-bit model of
tests/gls_shape_tangent_model.py (which tests/test_gls_shape_tangent_model.py pins against central differences of its own smooth
forward and against the shape adjoint's model).

The meshes, the Neumann plane z = 0 and the ALH tensor are those of tests/test_gpu_gls_shape_adjoint.py; the random-cloud Delaunay
mesh populates every bin of the adjoint kernel.

The bar, per row on the scale of the 80-bit model (D.tangent_dist):

    dist(device, exact) <= max(util.GLS_EXACT_SLACK_CAP x dist(float64 restatement, exact), TANGENT_RTOL)

The restatement is the same algorithm in plain float64 on the CPU; TANGENT_RTOL is the K tangent's existing bar.  The duality test has
both sides from the device -- the coordinate adjoint kernel with its three gathers, and the two geometry-tangent kernels with the
tangent kernel -- under the bar the two kernels' own bars allow.  Nothing in a bar is measured on the code under test.  Measured on
an MI355X: see DESIGN.md 4.17."""
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
import gls_shape_tangent_model as STM  # noqa: E402
import test_gpu_gls_shape_adjoint as SA  # noqa: E402
import util  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402
from test_gpu_gls_tangent import ADJOINT_RTOL, TANGENT_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

SLACK = util.GLS_EXACT_SLACK_CAP
H_FD, FD_RTOL = 1e-3, 1e-4          # the step and the bar of the shape adjoint's central difference through update_points()
MESHES = SA.MESHES
VARIANTS = ((True, True), (True, False), (False, True), (False, False))          # (add_neumann, with tangent_neumann_ws)


def _torch():
    import torch
    return torch


class Case(SA.Case):
    """SA.Case (one mesh on the device, its tables on the host, the shape adjoint's launch) with a direction dX and the tangent's
    launch and models"""

    def __init__(self, name, make=None):
        super().__init__(name, make)
        self.dX = np.random.default_rng(29).uniform(-1.0, 1.0, (self.P, 3))
        self.F = int(self.grid.n_faces)

    def tangent_models(self, dtype, directions=None, key="dX"):
        """shape_tangents of [dX] (or the directions given) in dtype, add_neumann = True (tangent_plain: the other value)"""
        if ("tan", key, dtype) not in self._models:
            self._models[("tan", key, dtype)] = STM.shape_tangents(self.grid, self.perm, self.dmag, self.flag, self.inpoel, self.inpofa,
                                                                   [self.dX] if directions is None else directions, True, dtype)
        return self._models[("tan", key, dtype)]

    def tangent(self, add_neumann=True, with_nws=True, dX=None):
        """(tangent_csr [n][nnz], tangent_neumann_ws [n][P] or None) from DevicePlan.launch_weights_tangent_points, into NaN-filled
        buffers; dX [P][3] or [n][P][3]"""
        torch = _torch()
        d = np.ascontiguousarray(self.dX if dX is None else dX, dtype=np.float64)
        d = d[None] if d.ndim == 2 else d
        n = len(d)
        dx = torch.from_numpy(d).to(self.dev)
        out = torch.full((n, self.nnz), float("nan"), dtype=torch.float64, device=self.dev)
        nws = torch.full((n, self.P), float("nan"), dtype=torch.float64, device=self.dev) if with_nws else None
        self.plan.launch_weights_tangent_points(dx.data_ptr(), out.data_ptr(), n, nws.data_ptr() if with_nws else 0,
                                                torch.cuda.current_stream(self.dev).cuda_stream, add_neumann=add_neumann)
        torch.cuda.synchronize(self.dev)
        return out.cpu().numpy(), nws.cpu().numpy() if with_nws else None


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=sorted(MESHES))
def case(request):
    return get_case(request.param)


def variant_of(model, add_neumann):
    """the model's dict for a launch with this add_neumann"""
    return model if add_neumann else dict(model, tangent=model["tangent_plain"])


def hold(tag, grid, got, got_nws, exact, restated):
    """prints the line of record and returns whether the device's tangent is inside the bar of the module's docstring"""
    d_ref = D.tangent_dist(grid, restated["tangent"], restated["tangent_neumann_ws"], exact)
    d_dev = D.tangent_dist(grid, got, got_nws, exact)
    assert d_ref <= D.CASE_CAP, (tag, d_ref)
    bar = max(SLACK * d_ref, TANGENT_RTOL)
    ratio = d_dev / d_ref if d_ref > 0 else float("inf")
    print(f"{tag}: restatement {d_ref:.2e}, device {d_dev:.2e}, ratio {ratio:.2f}, bar {bar:.2e}{'' if d_dev <= bar else '  MISSED'}")
    return d_dev <= bar


def check_variants(c, tag=""):
    exact, restated = c.tangent_models(D.LD)[0], c.tangent_models(np.float64)[0]
    assert exact["computed"].any() and not exact["computed"].all()              # computed nodes and zero-row nodes
    assert np.all(exact["scale"][exact["computed"]] > 0) and not exact["scale"][~exact["computed"]].any()
    assert np.count_nonzero(exact["tangent_neumann_ws"]) > 0
    rows = D._rows(c.grid)[2]
    ok = []
    for an, nws in VARIANTS:
        got, got_nws = c.tangent(an, nws)
        assert np.all(np.isfinite(got[0])) and not got[0][exact["scale"][rows] == 0].any()          # rows of scale 0: exactly 0
        if nws:
            assert not got_nws[0][exact["scale"] == 0].any() and not got_nws[0][c.flag == 0].any()
        ok.append(hold(f"{c.name}{tag} add_neumann={an}, tangent_neumann_ws={'wanted' if nws else 'not wanted'}", c.grid, got[0],
                       got_nws[0] if nws else None, variant_of(exact, an), variant_of(restated, an)))
    # add_neumann really enters
    assert np.abs(exact["tangent"] - exact["tangent_plain"]).max() > 1e-6 * np.abs(exact["tangent"]).max()
    assert all(ok), (c.name, tag)


def test_against_the_model(case):
    """both add_neumann values, with and without tangent_neumann_ws"""
    check_variants(case)


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    c.tangent()                                # (the tangent call makes the bins itself)
    plan = c.grid.gls_adjoint_plan()
    assert list(plan) == ["lds1", "lds2", "lds4", "global"] and all(v > 0 for v in plan.values()), plan
    assert sum(plan.values()) == c.P


def test_duality_with_the_coordinate_adjoint_kernel(case):
    """<ghat, dd> + <ghat_nws, dnws> = <Xbar, dX>, both sides from the device.  The bar is what the two kernels' own bars allow:
    ADJOINT_RTOL on every coordinate's gradient against its absolute-contribution scale, TANGENT_RTOL on every row's tangent against
    its scale -- the scales from the 80-bit models."""
    c = case
    tan = c.tangent_models(D.LD)[0]
    adjs = c.models(D.LD)                      # SA.VARIANTS: (add_neumann, with ghat_nws) = (True, True), (False, False)
    rowsum = np.bincount(D._rows(c.grid)[2], weights=np.abs(c.ghat), minlength=c.P)
    for (an, nws), adj in zip(SA.VARIANTS, adjs):
        xbar = c.device(an, nws)
        dd, dn = c.tangent(an, nws)
        lhs = c.ghat @ dd[0] + (c.gnws @ dn[0] if nws else 0.0)
        rhs = (xbar * c.dX).sum()
        bar = ADJOINT_RTOL * float((adj["scale"] * np.abs(c.dX)).sum()) + \
            TANGENT_RTOL * float((tan["scale"] * (rowsum + (np.abs(c.gnws) if nws else 0.0))).sum())
        print(f"{c.name} add_neumann={an}, ghat_nws={'given' if nws else 'none'}: duality gap {abs(lhs - rhs):.3e}, bar {bar:.3e}, "
              f"|<Xbar, dX>| {abs(rhs):.3e}")
        assert abs(rhs) > 0 and abs(lhs - rhs) <= bar


def test_determinism_batching_zero_linearity_and_growth():
    c = Case("mixed")                          # a grid of its own: the first call is the one direction
    first = c.tangent()                        # n_tangents = 1: the buffers are made for one direction
    assert c.grid._scalar("gls_shape_tangent_bytes") == 24 * c.E + 48 * c.F
    again = c.tangent()
    assert np.all(np.isfinite(first[0])) and first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    # three directions in one call = three single calls, bit for bit (one factorisation, the same tail per direction); the buffers grow
    three = np.stack([c.dX, np.random.default_rng(8).uniform(-1, 1, (c.P, 3)), np.zeros((c.P, 3))])
    batch = c.tangent(dX=three)
    assert c.grid._scalar("gls_shape_tangent_bytes") == 3 * (24 * c.E + 48 * c.F)
    assert batch[0].shape == (3, c.nnz) and batch[1].shape == (3, c.P)
    assert batch[0][0].tobytes() == first[0][0].tobytes() and batch[1][0].tobytes() == first[1][0].tobytes()      # growth left the first direction's bits
    for t in range(3):
        one = c.tangent(dX=three[t])
        assert one[0][0].tobytes() == batch[0][t].tobytes() and one[1][0].tobytes() == batch[1][t].tobytes()
    assert c.grid._scalar("gls_shape_tangent_bytes") == 3 * (24 * c.E + 48 * c.F)          # (kept at the largest batch)
    # the zero direction: exactly zero
    assert not batch[0][2].any() and not batch[1][2].any() and batch[0][0].any() and batch[0][1].any()
    # linearity: 2 dX gives twice the result BIT FOR BIT -- dX enters through products and sums only, and doubling commutes with each
    twice = c.tangent(dX=2.0 * c.dX)
    assert (2.0 * first[0]).tobytes() == twice[0].tobytes() and (2.0 * first[1]).tobytes() == twice[1].tobytes()


def test_a_tangent_only_session_makes_no_adjoint_buffer():
    c = Case("tet")                            # a grid of its own: nothing has run on it
    assert c.grid._scalar("gls_shape_tangent_bytes") == 0
    got = c.tangent(dX=np.stack([c.dX, -c.dX]))
    assert c.grid._scalar("gls_shape_contrib_bytes") == 0 and c.grid._scalar("gls_adjoint_contrib_bytes") == 0
    assert not c.grid.has_transpose_index
    assert c.grid._scalar("gls_shape_tangent_bytes") == 2 * (24 * c.E + 48 * c.F)
    c.tangent()                                # a smaller batch keeps the larger buffers
    assert c.grid._scalar("gls_shape_tangent_bytes") == 2 * (24 * c.E + 48 * c.F)
    c.grid.release_scratch()
    assert c.grid._scalar("gls_shape_tangent_bytes") == 0
    again = c.tangent(dX=np.stack([c.dX, -c.dX]))
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    assert c.grid._scalar("gls_shape_contrib_bytes") == 0 and c.grid._scalar("gls_adjoint_contrib_bytes") == 0


def test_a_plan_of_another_method_is_refused():
    from ninpol_amd.interpolator import DevicePlan
    c = get_case("tet")
    for meth in ("idw", "ls"):
        with pytest.raises(ValueError, match="do depend on the node coordinates, but they are not differentiated"):
            DevicePlan(c.I, "u", meth).launch_weights_tangent_points(8, 8)


def test_points_tangent_against_the_model_and_a_central_difference():
    torch = _torch()
    c = Case("mixed")                          # its own Interpolator: the differencing moves the mesh
    rng = np.random.default_rng(3)
    u = rng.uniform(-1.0, 1.0, (2, c.E))
    # the second direction moves ONE coordinate, as the shape adjoint's central difference does (its step and bar are for that): the
    # interior node nearest the middle of the mesh, along x
    interior = np.flatnonzero(np.asarray(c.grid.boundary_points).astype(np.int64) == 0)
    p = int(interior[np.argmin(((c.coords[interior] - c.coords.mean(axis=0)) ** 2).sum(axis=1))])
    one = np.zeros((c.P, 3))
    one[p, 0] = 1.0
    dX2 = np.stack([c.dX, one])
    exact, restated = c.tangent_models(D.LD, list(dX2), "pt"), c.tangent_models(np.float64, list(dX2), "pt")
    dv, dn = c.I.points_tangent("u", dX2, u)
    assert dv.shape == (2, c.P) and dn.shape == (2, c.P) and dv.dtype == np.float64 and dn.dtype == np.float64
    for f in range(2):
        ex, re = D.jvp_of(c.grid, exact[f], u[f], None, D.LD), D.jvp_of(c.grid, restated[f], u[f], None, np.float64)
        d_ref, d_dev = D.dist(re["value"], ex["value"], ex["scale"]), D.dist(dv[f], ex["value"], ex["scale"])
        n_ref = D.dist(restated[f]["tangent_neumann_ws"], exact[f]["tangent_neumann_ws"], exact[f]["scale"])
        n_dev = D.dist(dn[f], exact[f]["tangent_neumann_ws"], exact[f]["scale"])
        bar, nbar = max(SLACK * d_ref, TANGENT_RTOL), max(SLACK * n_ref, TANGENT_RTOL)
        print(f"points_tangent, k = 2, field {f}: node values restatement {d_ref:.2e}, device {d_dev:.2e}, bar {bar:.2e}; "
              f"neumann_ws restatement {n_ref:.2e}, device {n_dev:.2e}, bar {nbar:.2e}")
        assert d_ref <= D.CASE_CAP and d_dev <= bar and n_dev <= nbar and np.abs(dv[f]).max() > 0
    single = c.I.points_tangent("u", c.dX)                               # one direction, the cell variable itself
    assert single[0].shape == (c.P,) and single[1].shape == (c.P,) and np.all(np.isfinite(single[0])) and np.abs(single[0]).max() > 0
    assert single[1].tobytes() == dn[0].tobytes()                        # (neumann_ws does not depend on the field)
    with pytest.raises(ValueError):
        c.I.points_tangent("u", c.dX[:-1])
    with pytest.raises(ValueError):
        c.I.points_tangent("u", dX2, u[0])

    # the weights before the differencing, bit for bit what they must be after it
    before = util.torch_to_host(util.torch_launch(c.plan, np.nan, add_neumann=True))
    # apply() really moves that way: one central difference through the library's own update_points() + apply()
    vals = []
    try:
        for sgn in (+1, -1):
            c.I.update_points(c.coords + sgn * H_FD * one)
            vals.append(c.I.apply("u", "gls", values=u[1]))
    finally:
        c.I.update_points(c.coords)
    fd_v, fd_n = (vals[0][0] - vals[1][0]) / (2 * H_FD), (vals[0][1] - vals[1][1]) / (2 * H_FD)
    top = np.abs(dv[1]).max()
    e_v, e_n = np.abs(fd_v - dv[1]).max() / top, np.abs(fd_n - dn[1]).max() / top
    print(f"points_tangent: central difference through update_points(), h = {H_FD}: |difference| / max|d node values| {e_v:.2e} (node values), "
          f"{e_n:.2e} (neumann_ws); max|d node values| {top:.3e}")
    assert e_v <= FD_RTOL and e_n <= FD_RTOL
    after = util.torch_to_host(util.torch_launch(c.plan, np.nan, add_neumann=True))
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    again = c.I.points_tangent("u", dX2, u)
    assert again[0].tobytes() == dv.tobytes() and again[1].tobytes() == dn.tobytes()
    torch.cuda.synchronize()


def test_torch_forward_ad():
    """CellToNode(u, points=X) under forward_ad.dual_level() on the mixed mesh, k = 2 fields"""
    torch = _torch()
    import torch.autograd.forward_ad as fwAD
    from ninpol_amd.torch_ops import CellToNode
    c = Case("mixed")                          # its own Interpolator: the op rewrites the resident coordinates
    dev = c.dev
    op = CellToNode(c.I, "u", "gls")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream          # noqa: E731
    rng = np.random.default_rng(9)
    u_np, du_np, v_np = rng.uniform(-1.0, 1.0, (2, c.E)), rng.uniform(-1.0, 1.0, (2, c.E)), rng.uniform(-1.0, 1.0, (2, c.P))
    u0, du0, v = torch.from_numpy(u_np).to(dev), torch.from_numpy(du_np).to(dev), torch.from_numpy(v_np).to(dev)
    X0 = torch.from_numpy(c.coords + rng.uniform(-1e-3, 1e-3, (c.P, 3))).to(dev)
    dX0 = torch.from_numpy(c.dX).to(dev)
    K0 = torch.from_numpy(c.perm.reshape(c.E, 3, 3).copy()).to(dev)
    dK0 = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (c.E, 3, 3))).to(dev)

    def run():
        """the primal output and the gradients of a run without duals"""
        X, K, u = X0.clone().requires_grad_(), K0.clone().requires_grad_(), u0.clone().requires_grad_()
        out = op(u, K, None, X)
        (out * v).sum().backward()
        return out.detach(), X.grad, K.grad, u.grad

    before = run()
    plain = op(u0, points=X0)
    assert torch.equal(plain, before[0])
    # the kernel-level tangents at X0
    dw = torch.full((c.nnz,), float("nan"), dtype=torch.float64, device=dev)
    dnws = torch.full((c.P,), float("nan"), dtype=torch.float64, device=dev)
    op.plan.launch_weights_tangent_points(dX0.data_ptr(), dw.data_ptr(), 1, dnws.data_ptr(), stream(), add_neumann=True)
    dwk = torch.full((c.nnz,), float("nan"), dtype=torch.float64, device=dev)
    op.plan.launch_weights_tangent(dK0.reshape(c.E, 9).contiguous().data_ptr(), dwk.data_ptr(), 1, 0, 0, stream(), add_neumann=True)
    w_now, _ = op._launch_weights()
    with fwAD.dual_level():
        # dual points alone: spmv(kernel-level dW, u), bit for bit
        out = op(u0, points=fwAD.make_dual(X0, dX0))
        primal, tangent = fwAD.unpack_dual(out)
        assert torch.equal(primal, plain) and tangent is not None and tangent.shape == (2, c.P)
        t_points = op._spmv(dw, u0)
        assert torch.isfinite(tangent).all() and tangent.abs().max() > 0 and torch.equal(tangent, t_points)
        # ... with dual u: + W du
        out = op(fwAD.make_dual(u0, du0), points=fwAD.make_dual(X0, dX0))
        primal, tangent = fwAD.unpack_dual(out)
        assert torch.equal(primal, plain) and torch.equal(tangent, op._spmv(w_now, du0) + t_points)
        # ... with dual K: the sum of the two separate tangents, within TANGENT_RTOL on the row scale of each
        out = op(u0, fwAD.make_dual(K0, dK0), None, fwAD.make_dual(X0, dX0))
        primal, tangent = fwAD.unpack_dual(out)
        assert torch.equal(primal, plain)
        t_both = tangent.cpu().numpy()
        t_perm = op._spmv(dwk, u0)
        # weights_of: (dW, dneumann_ws) themselves
        w, nws = op.weights_of(points=fwAD.make_dual(X0, dX0))
        assert torch.equal(fwAD.unpack_dual(w).tangent, dw) and torch.equal(fwAD.unpack_dual(nws).tangent, dnws)
    # the row scales at what is resident: the geometry of X0 (the grid's arrays are fetched again after an update)
    assert np.array_equal(np.asarray(c.grid.point_coords).reshape(-1, 3), X0.cpu().numpy())
    tp = STM.shape_tangents(c.grid, c.perm, c.dmag, c.flag, c.inpoel, c.inpofa, [c.dX], True, np.float64)[0]
    tk = D.tangent(c.grid, c.perm, c.dmag, c.flag, dK0.cpu().numpy().reshape(c.E, 9), None, True, np.float64)
    ptr, esup, rows = D._rows(c.grid)
    room = np.stack([np.bincount(rows, weights=np.abs(u_np[f])[esup], minlength=c.P) for f in range(2)]) * (tp["scale"] + tk["scale"])
    gap = np.abs(t_both - (t_points + t_perm).cpu().numpy())
    none = room == 0
    worst = float((gap[~none] / room[~none]).max())
    print(f"torch forward_ad, dual points and K: {worst:.2e} of the row scale from the sum of the two separate tangents (bar {TANGENT_RTOL:.1e})")
    assert not gap[none].any() and worst <= TANGENT_RTOL and t_perm.abs().max() > 0
    # the primal output and backward() are what they were, bit for bit
    after = run()
    assert all(torch.equal(a, b) for a, b in zip(before, after))

    # jvp after an intervening update refuses, as backward does (autograd itself calls jvp right behind forward: a later caller)
    import types
    from ninpol_amd.torch_ops import _GlsWeightsFn
    ctx = types.SimpleNamespace(op=op, stamp=op._stamp(), saved_tensors=(None, None))
    dw2, dn2 = _GlsWeightsFn.jvp(ctx, None, None, None, dX0)
    assert torch.equal(dw2, dw) and torch.equal(dn2, dnws)
    c.I.update_points(X0)
    with pytest.raises(RuntimeError, match="geometry_updates"):
        _GlsWeightsFn.jvp(ctx, None, None, None, dX0)
    # IDW / LS depend on the coordinates but are not differentiated: an error, never zeros
    op_idw = CellToNode(c.I, "u", "idw")
    with fwAD.dual_level():
        with pytest.raises(ValueError, match="not differentiated"):
            op_idw(u0, points=fwAD.make_dual(X0, dX0))


# ---- the ABI contract of the device entry point on a device ------------------------------------------------------------------------

def test_abi_two_dimensional_grid_and_zero_directions():
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
    I.grid.to_device(I.device)
    for call in (lambda: L.nin_gls_weights_tangent_points_device(I.grid._h, 1, 1, vp(dev), vp(dev), vp(dev), None),
                 lambda: L.nin_gls_points_tangent_host(I.grid._h, hp, hp, 1, hp, hp)):
        rc, text = call(), L.nin_last_error().decode()
        assert rc == _lib.NIN_EINVAL and "3-D grids only" in text and "2-D" in text, (rc, text)
    assert not buf.any() and not dev.any().item()                        # nothing was written
    assert I.grid._scalar("gls_shape_tangent_bytes") == 0
    # n_tangents = 0: what the K tangent gives, on a 3-D grid on the device
    c = get_case("tet")
    rc_k, text_k = L.nin_gls_weights_tangent_device(c.grid._h, 1, 0, vp(dev), None, vp(dev), None, None), L.nin_last_error().decode()
    rc_x, text_x = L.nin_gls_weights_tangent_points_device(c.grid._h, 1, 0, vp(dev), vp(dev), None, None), L.nin_last_error().decode()
    assert rc_x == rc_k == _lib.NIN_EINVAL and text_x == text_k, (rc_x, text_x, rc_k, text_k)
    assert L.nin_gls_points_tangent_host(c.grid._h, hp, hp, 0, hp, hp) == L.nin_gls_permeability_tangent_host(c.grid._h, hp, hp, 0, hp, hp) == _lib.NIN_EINVAL
    assert not buf.any() and not dev.any().item()


# ---- every system in global-memory scratch ------------------------------------------------------------------------------------------

def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    c.tangent()                             # (the tangent call makes the bins itself)
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    check_variants(c, " forced global")
    a, b = c.tangent(), c.tangent()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    print("CHILD OK")


def test_forced_global_class():
    """the hexahedron mesh again with every system in global-memory scratch, in a fresh process (the switch is read when the bins are
    made), under the same bar"""
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


if __name__ == "__main__":
    _child()
