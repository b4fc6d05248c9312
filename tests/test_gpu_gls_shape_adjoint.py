"""The GLS weights differentiated with respect to the node coordinates, on the device: DevicePlan.launch_weights_backward_points,
Interpolator.points_gradient and the torch op CellToNode(u, points=...), held to the 80-bit model of tests/gls_shape_model.py (which
tests/test_gls_shape_model.py pins against central differences of its own smooth forward and of the oracle).

Every mesh carries the Neumann plane z = 0 and the ALH tensor; the random-cloud Delaunay mesh populates every bin of the adjoint kernel.

The bar, per coordinate on the scale of the 80-bit model (the sum of the absolute contributions):

    dist(device, exact) <= max(util.GLS_EXACT_SLACK_CAP x dist(float64 restatement, exact), ADJOINT_RTOL)

The restatement is the same algorithm in plain float64 on the CPU; ADJOINT_RTOL is the adjoint kernel's existing bar.  Nothing in the
bar is measured on the code under test.  Measured on an MI355X: see DESIGN.md 4.15."""
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
import gls_shape_model as SM  # noqa: E402
import util  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402
from test_gpu_gls_tangent import ADJOINT_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

assert SM.ADJOINT_RTOL == ADJOINT_RTOL          # (the CPU tests take the same number from the model's module)
SLACK = util.GLS_EXACT_SLACK_CAP
H_FD, FD_RTOL = 1e-3, 1e-4          # the step and the bar of tests/test_gls_shape_model.py's oracle differences

MESHES = {
    "hex": lambda: M.hex_mesh(4, jitter=0.1, seed=1),
    "tet": lambda: M.tet_mesh(3, jitter=0.1, seed=3),
    "mixed": lambda: M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2),
    "delaunay": lambda: M.delaunay_tet_mesh(6, seed=4, lattice="random"),
}
VARIANTS = ((True, True), (False, False))          # (add_neumann, with grad_neumann_ws)


def _torch():
    import torch
    return torch


class Case:
    """one mesh on the device, its tables on the host, an upstream gradient and the models' answers (computed once, lazily)"""

    def __init__(self, name, make=None):
        import ninpol_amd
        from ninpol_amd.interpolator import DevicePlan
        self.name = name
        mesh = M.attach_fields((make or MESHES[name])(), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
        self.I = I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=mesh)
        self.plan = DevicePlan(I, "u", "gls")
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        perm, dmag = I._perm_rows()
        self.perm, self.dmag = np.array(perm).reshape(self.E, 9), np.array(dmag)
        self.flag = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        self.coords = np.array(g.point_coords, dtype=np.float64).reshape(self.P, 3)
        self.inpoel, self.inpofa = np.array(g.inpoel), np.array(g.inpofa)
        rng = np.random.default_rng(17)
        self.ghat, self.gnws = rng.uniform(-1.0, 1.0, self.nnz), rng.uniform(-1.0, 1.0, self.P)
        self.dev = _torch().device("cuda", int(I.device))
        self._models = {}

    def models(self, dtype, cotangents=None, key="variants"):
        """shape_adjoints over VARIANTS (or the cotangents given) in dtype: one pass over the nodes per format"""
        if (key, dtype) not in self._models:
            cots = cotangents or [(self.ghat, self.gnws if nws else None, an) for an, nws in VARIANTS]
            self._models[(key, dtype)] = SM.shape_adjoints(self.grid, self.perm, self.dmag, self.flag, self.inpoel, self.inpofa, cots, dtype)
        return self._models[(key, dtype)]

    def device(self, add_neumann=True, with_nws=True, ghat=None):
        """grad_points [P][3] from DevicePlan.launch_weights_backward_points, into a NaN-filled buffer"""
        torch = _torch()
        g = torch.from_numpy(self.ghat if ghat is None else ghat).to(self.dev)
        gn = torch.from_numpy(self.gnws).to(self.dev) if with_nws else None
        out = torch.full((self.P, 3), float("nan"), dtype=torch.float64, device=self.dev)
        self.plan.launch_weights_backward_points(g.data_ptr(), out.data_ptr(), gn.data_ptr() if with_nws else 0,
                                                 torch.cuda.current_stream(self.dev).cuda_stream, add_neumann=add_neumann)
        torch.cuda.synchronize(self.dev)
        return out.cpu().numpy()


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=sorted(MESHES))
def case(request):
    return get_case(request.param)


def hold(tag, got, exact, restated):
    """prints the line of record and returns whether `got` is inside the bar of the module's docstring"""
    d_ref = D.dist(restated["grad_points"], exact["grad_points"], exact["scale"])
    d_dev = D.dist(got, exact["grad_points"], exact["scale"])
    assert d_ref <= D.CASE_CAP, (tag, d_ref)
    bar = max(SLACK * d_ref, ADJOINT_RTOL)
    ratio = d_dev / d_ref if d_ref > 0 else float("inf")
    print(f"{tag}: restatement {d_ref:.2e}, device {d_dev:.2e}, ratio {ratio:.2f}, bar {bar:.2e}{'' if d_dev <= bar else '  MISSED'}")
    return d_dev <= bar


def check_variants(c, tag=""):
    exact, restated = c.models(D.LD), c.models(np.float64)
    ok = []
    for (an, nws), ex, re in zip(VARIANTS, exact, restated):
        assert np.count_nonzero(ex["grad_points"]) > 0 and not ex["computed"].all()
        ok.append(hold(f"{c.name}{tag} add_neumann={an}, grad_neumann_ws={'given' if nws else 'none'}", c.device(an, nws), ex, re))
    # both terms really enter: the two variants answer differently
    assert np.abs(exact[0]["grad_points"] - exact[1]["grad_points"]).max() > 1e-6 * np.abs(exact[0]["grad_points"]).max()
    assert all(ok), (c.name, tag)


def test_against_the_model(case):
    """both add_neumann values, with and without dL/dneumann_ws; the model's forward is the library's own weights"""
    check_variants(case)


def test_two_calls_agree_bit_for_bit(case):
    a, b = case.device(), case.device()
    assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()


def test_dirichlet_vertices_receive_gradient(case):
    """a Dirichlet node has the zero row and is not computed, but it is a vertex of cells and faces of nodes that are"""
    ex = case.models(D.LD)[0]
    dirichlet = (np.asarray(case.grid.boundary_points).astype(np.int64) != 0) & (case.flag == 0)
    assert dirichlet.any() and not ex["computed"][dirichlet].any()
    got = case.device()
    assert np.count_nonzero(np.abs(got[dirichlet]).max(axis=1)) >= 1
    assert np.count_nonzero(np.abs(ex["grad_points"][dirichlet]).max(axis=1)) >= 1


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    plan = c.grid.gls_adjoint_plan()
    assert list(plan) == ["lds1", "lds2", "lds4", "global"] and all(v > 0 for v in plan.values()), plan
    assert sum(plan.values()) == c.P


def test_buffers_are_made_by_the_first_call_and_given_back():
    c = get_case("tet")
    a = c.device()
    F = int(c.grid.n_faces)
    assert c.grid._scalar("gls_shape_contrib_bytes") == 24 * c.nnz + 48 * int(c.grid._scalar("nnz_fsup")) + 96 * F
    assert c.grid._scalar("gls_adjoint_contrib_bytes") == 0          # nothing of the K adjoint's 80 bytes per entry was made
    c.grid.release_scratch()
    assert c.grid._scalar("gls_shape_contrib_bytes") == 0 and not c.grid.has_transpose_index
    assert c.device().tobytes() == a.tobytes()


def test_translation_invariance():
    """translating every point leaves every weight alone: per axis the gradient sums to zero on the scale of its contributions"""
    c = Case("hex12", lambda: M.hex_mesh(12, jitter=0.15))
    got = c.device()
    room = c.models(np.float64, [(c.ghat, c.gnws, True)], "one")[0]["scale"].sum(axis=0)
    total = np.abs(got.sum(axis=0))
    print("hex12: |sum_p grad_points[p]| / sum_p scale[p] per axis: " + ", ".join(f"{t / r:.2e}" for t, r in zip(total, room)))
    assert np.all(room > 0) and np.all(total <= ADJOINT_RTOL * room) and np.abs(got).max() > 0


def test_points_gradient_against_the_model_and_a_central_difference():
    torch = _torch()
    c = Case("mixed")                       # its own Interpolator: the differencing moves the mesh
    rng = np.random.default_rng(3)
    v, u = rng.uniform(-1.0, 1.0, (2, c.P)), rng.uniform(-1.0, 1.0, (2, c.E))
    ptr, esup = np.asarray(c.grid.esup_ptr), np.asarray(c.grid.esup)
    rows = np.repeat(np.arange(c.P), np.diff(ptr))
    ghat = (v[:, rows] * u[:, esup]).sum(axis=0)
    ex = c.models(D.LD, [(ghat, None, True)], "pg")[0]
    re = c.models(np.float64, [(ghat, None, True)], "pg")[0]
    got = c.I.points_gradient("u", v, u)
    assert got.shape == (c.P, 3) and got.dtype == np.float64
    assert hold("points_gradient, k = 2", got, ex, re)
    one = c.I.points_gradient("u", v[0])                               # the cell variable itself
    assert one.shape == (c.P, 3) and np.all(np.isfinite(one)) and np.abs(one).max() > 0

    # the weights before the differencing, bit for bit what they must be after it
    before = util.torch_to_host(util.torch_launch(c.plan, np.nan, add_neumann=True))
    # <v, W(x) u> really moves that way: one central difference through the library's own update_points() + apply()
    p = int(np.argmax(np.abs(got).max(axis=1)))
    k = int(np.argmax(np.abs(got[p])))
    vals = []
    try:
        for sgn in (+1, -1):
            X = c.coords.copy()
            X[p, k] += sgn * H_FD
            c.I.update_points(X)
            vals.append(float((c.I.apply("u", "gls", values=u)[0] * v).sum()))
    finally:
        c.I.update_points(c.coords)
    fd = (vals[0] - vals[1]) / (2 * H_FD)
    print(f"points_gradient: central difference {fd:.9e}, device {got[p, k]:.9e}, |difference| / max|grad| {abs(fd - got[p, k]) / np.abs(got).max():.2e}")
    assert abs(fd - got[p, k]) <= FD_RTOL * np.abs(got).max()
    after = util.torch_to_host(util.torch_launch(c.plan, np.nan, add_neumann=True))
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert c.I.points_gradient("u", v, u).tobytes() == got.tobytes()
    torch.cuda.synchronize()


def test_torch_op():
    """CellToNode(u, K, scale, points) on the mixed mesh, k = 2 fields"""
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    c = Case("mixed")                       # its own Interpolator: the op rewrites the resident coordinates
    dev = c.dev
    op = CellToNode(c.I, "u", "gls")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream          # noqa: E731
    rng = np.random.default_rng(9)
    u_np, v_np = rng.uniform(-1.0, 1.0, (2, c.E)), rng.uniform(-1.0, 1.0, (2, c.P))
    v = torch.from_numpy(v_np).to(dev)
    X_np = c.coords + rng.uniform(-1e-3, 1e-3, (c.P, 3))

    # without points: what the op did before it knew them
    u0 = torch.from_numpy(u_np).to(dev).requires_grad_()
    out0 = op(u0)
    (out0 * v).sum().backward()
    K = torch.from_numpy(c.perm.reshape(c.E, 3, 3).copy()).to(dev)
    uk = torch.from_numpy(u_np).to(dev).requires_grad_()
    Kk = K.clone().requires_grad_()
    outk = op(uk, Kk)
    (outk * v).sum().backward()
    assert torch.equal(outk, out0) and torch.equal(uk.grad, u0.grad)      # (the same K as the loaded one)

    # with points
    geom = c.grid.geometry_updates
    X = torch.from_numpy(X_np).to(dev).requires_grad_()
    u = torch.from_numpy(u_np).to(dev).requires_grad_()
    out = op(u, points=X)
    assert c.grid.geometry_updates == geom + 1
    (out * v).sum().backward()
    assert X.grad.shape == X.shape and torch.isfinite(X.grad).all() and X.grad.abs().max() > 0
    ghat = torch.empty(c.nnz, dtype=torch.float64, device=dev)
    op.plan.launch_sddmm(u.data_ptr(), v.data_ptr(), 2, ghat.data_ptr(), stream())
    direct = torch.full((c.P, 3), float("nan"), dtype=torch.float64, device=dev)
    op.plan.launch_weights_backward_points(ghat.data_ptr(), direct.data_ptr(), 0, stream(), add_neumann=True)
    assert torch.equal(X.grad, direct)
    # d/du: bit for bit the existing path on the same weights
    op.recompute_weights()
    u1 = torch.from_numpy(u_np).to(dev).requires_grad_()
    out1 = op(u1)
    (out1 * v).sum().backward()
    assert torch.equal(out1, out) and torch.equal(u1.grad, u.grad) and not torch.equal(out, out0)

    # K and points together: the two separate calls
    K2, X2, u2 = K.clone().requires_grad_(), X.detach().clone().requires_grad_(), torch.from_numpy(u_np).to(dev).requires_grad_()
    out2 = op(u2, K2, None, X2)
    (out2 * v).sum().backward()
    K3, u3 = K.clone().requires_grad_(), torch.from_numpy(u_np).to(dev)
    (op(u3, K3) * v).sum().backward()
    assert torch.equal(out2, out) and torch.equal(X2.grad, X.grad) and torch.equal(K2.grad, K3.grad) and torch.equal(u2.grad, u.grad)
    # a differentiable weights tensor on its own
    X4 = X.detach().clone().requires_grad_()
    w, nws = op.weights_of(points=X4)
    assert w.shape == (c.nnz,) and nws.shape == (c.P,) and w.requires_grad
    gh, gn = torch.from_numpy(c.ghat).to(dev), torch.from_numpy(c.gnws).to(dev)
    ((w * gh).sum() + (nws * gn).sum()).backward()
    direct4 = torch.full((c.P, 3), float("nan"), dtype=torch.float64, device=dev)
    op.plan.launch_weights_backward_points(gh.data_ptr(), direct4.data_ptr(), gn.data_ptr(), stream(), add_neumann=True)
    assert torch.equal(X4.grad, direct4)

    # backward after an intervening update refuses
    X5 = X.detach().clone().requires_grad_()
    out5 = op(u.detach(), points=X5)
    c.I.update_points(X.detach())
    with pytest.raises(RuntimeError, match="geometry_updates"):
        (out5 * v).sum().backward()
    assert X5.grad is None
    # IDW / LS depend on the coordinates but are not differentiated: an error, never zeros
    op_idw = CellToNode(c.I, "u", "idw")
    with pytest.raises(ValueError, match="not differentiated"):
        op_idw(u.detach(), points=X.detach().clone().requires_grad_())
    # argument errors
    with pytest.raises(TypeError):
        op(u.detach(), points=X_np)
    with pytest.raises(TypeError):
        op(u.detach(), points=X.detach().float())
    with pytest.raises(ValueError):
        op(u.detach(), points=X.detach().cpu())
    with pytest.raises(ValueError):
        op(u.detach(), points=X.detach()[:-1])
    with pytest.raises(ValueError):
        op.weights_of()


def test_a_plan_of_another_method_is_refused():
    from ninpol_amd.interpolator import DevicePlan
    c = get_case("tet")
    for meth in ("idw", "ls"):
        with pytest.raises(ValueError, match="do depend on the node coordinates, but they are not differentiated"):
            DevicePlan(c.I, "u", meth).launch_weights_backward_points(8, 8)


# ---- the ABI contract of the two entry points on a device --------------------------------------------------------------------------

ENTRY_POINTS = {   # entry point -> its arguments after the grid; "dev": a device buffer, "buf": a host buffer
    "nin_gls_weights_backward_points_device": (1, "dev", "dev", "dev", None),
    "nin_gls_points_gradient_host": ("buf", "buf", 1, "buf"),
}


def _call(L, name, g, dev, buf):
    args = [buf.ctypes.data_as(ctypes.c_void_p) if a == "buf" else ctypes.c_void_p(dev.data_ptr()) if a == "dev" else a for a in ENTRY_POINTS[name]]
    rc = getattr(L, name)(g, *args)
    return rc, L.nin_last_error().decode()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_abi_null_grid_and_two_dimensional_grid(name):
    import ninpol_amd
    from ninpol_amd import _lib
    torch = _torch()
    L = _lib.load()
    dev, buf = torch.zeros(1 << 12, dtype=torch.float64, device="cuda"), np.zeros(1 << 12)
    rc, text = _call(L, name, None, dev, buf)
    assert rc == _lib.NIN_EINVAL and text.startswith("NULL"), (rc, text)
    mesh = M.attach_fields(M.quad_tri_mesh_2d(4), "u", perm="LIN", neumann_plane=(1, 0.0), seed=5)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    assert int(I.grid.dim) == 2 and int(I.grid.n_points) * 3 <= 1 << 12
    I.grid.to_device(I.device)
    rc, text = _call(L, name, I.grid._h, dev, buf)
    assert rc == _lib.NIN_EINVAL and "3-D grids only" in text and "2-D" in text, (rc, text)
    assert not buf.any() and not dev.any().item()                       # nothing was written
    assert I.grid._scalar("gls_shape_contrib_bytes") == 0


# ---- every system in global-memory scratch ------------------------------------------------------------------------------------------

def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    check_variants(c, " forced global")
    a, b = c.device(), c.device()
    assert a.tobytes() == b.tobytes()
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
