"""The corner gradients of the GLS reconstruction on the device: DevicePlan.launch_corner_gradients, Interpolator.corner_gradients /
node_gradient and CellToNode.corner_gradients, held to the 80-bit model of tests/gls_gradient_model.py (which
tests/test_gls_gradient_model.py pins against the oracle's weights, the normal equations and two mutants).

The meshes are those of tests/test_gpu_gls_shape_adjoint.py: every one carries jitter, the Neumann plane z = 0 and the ALH tensor; the
random-cloud Delaunay mesh populates every bin of the adjoint kernel.

The bar, per entry on the scale of the 80-bit model (the sum of the absolute contributions):

    dist(device, exact) <= max(util.GLS_EXACT_SLACK_CAP x dist(float64 restatement, exact), ADJOINT_RTOL)

The restatement is the same algorithm in plain float64 on the CPU; ADJOINT_RTOL is the adjoint kernel's existing bar (the same kernel,
the same factorisation, the same kind of tail).  Nothing in the bar is measured on the code under test.  Measured on an MI355X: see
DESIGN.md 4.21.

Linear exactness (one block of the LIN tensor, all-Dirichlet boundary, u = a + beta . x): every interior node must give g_i = beta and
u_p = a + beta . x_p; the device may be away from beta by what the rounding of its inputs allows (the model's propagated room, as
tests/test_gls_gradient_model.py words it) plus the bar above."""
import copy
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
import gls_gradient_model as GG  # noqa: E402
import gls_shape_model as SM  # noqa: E402
import util  # noqa: E402
from gls_exact import LD  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu

ADJOINT_RTOL = SM.ADJOINT_RTOL
SLACK = util.GLS_EXACT_SLACK_CAP
N_FIELDS = 3
A0, BETA = 0.3, (1.0, -2.0, 0.5)

MESHES = {
    "hex": lambda: M.hex_mesh(4, jitter=0.1, seed=1),
    "tet": lambda: M.tet_mesh(3, jitter=0.1, seed=3),
    "mixed": lambda: M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2),
    "delaunay": lambda: M.delaunay_tet_mesh(6, seed=4, lattice="random"),
}
LINEAR_MESHES = {
    "hex": lambda: M.hex_mesh(4, jitter=0.1),
    "delaunay": lambda: M.delaunay_tet_mesh(6, lattice="random"),
}
OUTPUTS = ("grad", "node_values", "flux", "node_gradient")


def _torch():
    import torch
    return torch


class Case:
    """one mesh on the device, its tables on the host, N_FIELDS cell fields and the models' answers (computed once, lazily)"""

    def __init__(self, name, mesh=None):
        import ninpol_amd
        from ninpol_amd.interpolator import DevicePlan
        self.name = name
        self.mesh = mesh if mesh is not None else M.attach_fields(MESHES[name](), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
        self.I = I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=self.mesh)
        self.plan = DevicePlan(I, "u", "gls")
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        perm_rows, dmag = I._perm_rows()
        self.perm, self.dmag = np.array(perm_rows).reshape(self.E, 9), np.array(dmag)
        self.flag = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        self.ptr, self.esup = np.array(g.esup_ptr).astype(np.int64), np.array(g.esup).astype(np.int64)
        self.u = np.random.default_rng(23).uniform(-1.0, 1.0, (N_FIELDS, self.E))
        self.dev = _torch().device("cuda", int(I.device))
        self._models = {}

    def model(self, dtype):
        if dtype not in self._models:
            self._models[dtype] = GG.corner_gradients(self.grid, self.perm, self.dmag, self.flag, self.u, dtype)
        return self._models[dtype]

    def stream(self):
        return _torch().cuda.current_stream(self.dev).cuda_stream

    def device(self, u=None, want=OUTPUTS):
        """{output: numpy array} from DevicePlan.launch_corner_gradients on u [k][E] (default: the case's fields), into NaN-filled buffers"""
        torch = _torch()
        u = self.u if u is None else np.atleast_2d(u)
        k = u.shape[0]
        shapes = {"grad": (k, self.nnz, 3), "node_values": (k, self.P), "flux": (k, self.nnz, 3), "node_gradient": (k, self.P, 3)}
        bufs = {o: torch.full(shapes[o], float("nan"), dtype=torch.float64, device=self.dev) for o in want}
        ptr = lambda o: bufs[o].data_ptr() if o in bufs else 0          # noqa: E731
        ud = torch.from_numpy(np.ascontiguousarray(u)).to(self.dev)
        self.plan.launch_corner_gradients(ud.data_ptr(), ptr("grad"), k, ptr("node_values"), ptr("flux"), ptr("node_gradient"), self.stream())
        torch.cuda.synchronize(self.dev)
        return {o: b.cpu().numpy() for o, b in bufs.items()}


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=sorted(MESHES))
def case(request):
    return get_case(request.param)


def hold(tag, got, exact, restated, key, scale):
    """prints the line of record and returns whether `got` is inside the bar of the module's docstring, the worst of the fields"""
    ok = True
    for f in range(got.shape[0]):
        d_ref = D.dist(restated[key][f], exact[key][f], exact[scale][f])
        d_dev = D.dist(got[f], exact[key][f], exact[scale][f])
        assert d_ref <= D.CASE_CAP, (tag, key, f, d_ref)
        bar = max(SLACK * d_ref, ADJOINT_RTOL)
        ratio = d_dev / d_ref if d_ref > 0 else float("inf")
        print(f"{tag} {key}[{f}]: restatement {d_ref:.2e}, device {d_dev:.2e}, ratio {ratio:.2f}, bar {bar:.2e}{'' if d_dev <= bar else '  MISSED'}")
        ok = ok and d_dev <= bar
    return ok


def check_model(c, tag=""):
    exact, restated = c.model(LD), c.model(np.float64)
    assert np.count_nonzero(exact["grad"]) > 0 and 0 < exact["computed"].sum() < c.P
    got = c.device(want=("grad", "node_values"))
    ok_g = hold(c.name + tag, got["grad"], exact, restated, "grad", "scale")
    ok_n = hold(c.name + tag, got["node_values"], exact, restated, "node_values", "scale_node")
    assert ok_g and ok_n, (c.name, tag)


def test_against_the_model(case):
    """N_FIELDS fields in one launch, the gradients and the node values"""
    check_model(case)


def test_each_field_equals_its_own_launch(case):
    """n_fields = 3 in one launch against n_fields = 1 three times: every output, bit for bit"""
    batch = case.device()
    for f in range(N_FIELDS):
        one = case.device(case.u[f])
        for o in OUTPUTS:
            assert np.all(np.isfinite(one[o])) and one[o][0].tobytes() == batch[o][f].tobytes(), (o, f)


def test_two_calls_agree_bit_for_bit(case):
    a, b = case.device(), case.device()
    for o in OUTPUTS:
        assert np.all(np.isfinite(a[o])) and a[o].tobytes() == b[o].tobytes(), o


def test_zero_rows_are_zeros(case):
    """the forward's zero rows (Dirichlet nodes among them) write zeros into NaN-filled buffers, and only they"""
    got = case.device()
    computed = case.model(np.float64)["computed"]
    dirichlet = (np.asarray(case.grid.boundary_points).astype(np.int64) != 0) & (case.flag == 0)
    assert dirichlet.any() and not computed[dirichlet].any()
    off = np.repeat(~computed, np.diff(case.ptr))
    for o in OUTPUTS:
        assert np.all(np.isfinite(got[o])), o
    assert not got["grad"][:, off].any() and not got["flux"][:, off].any()
    assert not got["node_values"][:, ~computed].any() and not got["node_gradient"][:, ~computed].any()
    assert np.all(np.abs(got["grad"][:, ~off]).max(axis=2) > 0) and np.all(got["node_values"][:, computed] != 0)


def test_node_values_are_the_plans_weights_applied(case):
    """u_p against launch_spmv of the plan's add_neumann=False weights, to the parity bar of tests/util.py: an entry of a row may be
    WEIGHT_RTOL of the row's largest weight away, so the product may be that times sum_i |u_i|"""
    torch = _torch()
    c = case
    w, _ = util.torch_launch(c.plan, np.nan, add_neumann=False)
    ud = torch.from_numpy(c.u).to(c.dev)
    out = torch.full((N_FIELDS, c.P), float("nan"), dtype=torch.float64, device=c.dev)
    c.plan.launch_spmv(w.data_ptr(), ud.data_ptr(), N_FIELDS, out.data_ptr(), c.stream())
    torch.cuda.synchronize(c.dev)
    wh, want = w.cpu().numpy(), out.cpu().numpy()
    got = c.device(want=("grad", "node_values"))["node_values"]
    wmax, usum = np.zeros(c.P), np.zeros((N_FIELDS, c.P))
    rows = np.repeat(np.arange(c.P), np.diff(c.ptr))
    np.maximum.at(wmax, rows, np.abs(wh))
    for f in range(N_FIELDS):
        np.add.at(usum[f], rows, np.abs(c.u[f, c.esup]))
    room = wmax * usum
    on = room > 0
    assert not got[~on].any() and not want[~on].any()
    worst = float((np.abs(got - want)[on] / room[on]).max())
    print(f"{c.name}: |u_p - spmv| / (max |w| sum |u|) {worst:.2e}")
    assert worst <= util.WEIGHT_RTOL


def test_flux_is_minus_K_grad_bit_for_bit(case):
    """flux[f][pos][c] = -((K[3c] g[0] + K[3c+1] g[1]) + K[3c+2] g[2]) of the returned g, K the resident tensor of cell esup[pos]"""
    got = case.device(want=("grad", "flux"))
    K = case.perm[case.esup]                                             # [nnz][9]
    g = got["grad"]
    want = np.stack([-((K[:, 3 * c + 0] * g[:, :, 0] + K[:, 3 * c + 1] * g[:, :, 1]) + K[:, 3 * c + 2] * g[:, :, 2]) for c in range(3)], axis=2)
    assert np.count_nonzero(want) > 0 and got["flux"].tobytes() == np.ascontiguousarray(want).tobytes()


def test_node_gradient_is_the_row_order_mean(case):
    """summed from 0.0 in row order, divided by the number of cells; bit for bit"""
    got = case.device(want=("grad", "node_gradient"))
    cnt = np.diff(case.ptr)
    acc = np.zeros((N_FIELDS, case.P, 3))
    for j in range(int(cnt.max())):
        on = cnt > j
        acc[:, on] += got["grad"][:, case.ptr[:-1][on] + j]
    want = acc / cnt[None, :, None]
    assert cnt.min() > 0 and np.count_nonzero(want) > 0 and got["node_gradient"].tobytes() == np.ascontiguousarray(want).tobytes()


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    plan = c.grid.gls_adjoint_plan()
    assert list(plan) == ["lds1", "lds2", "lds4", "global"] and all(v > 0 for v in plan.values()), plan


@pytest.mark.parametrize("name", sorted(LINEAR_MESHES))
def test_linear_exactness(name):
    mesh = M.attach_fields(LINEAR_MESHES[name](), "u", perm="LIN", neumann_plane=None, seed=3)
    c = Case("linear " + name, mesh=mesh)
    assert not c.flag.any() and np.all(c.perm == c.perm[0])
    u, room = GG.linear_field(c.grid, A0, BETA)
    ex = GG.corner_gradients(c.grid, c.perm, c.dmag, c.flag, u, LD, room=room)
    re = GG.corner_gradients(c.grid, c.perm, c.dmag, c.flag, u, np.float64)
    computed = ex["computed"]
    assert computed.any() and np.array_equal(computed, np.asarray(c.grid.boundary_points).astype(np.int64) == 0)
    got = c.device(u, want=("grad", "node_values"))
    beta = np.array(BETA, dtype=LD)
    on = np.repeat(computed, np.diff(c.ptr))
    X = np.asarray(c.grid.point_coords, dtype=np.float64).reshape(-1, 3).astype(LD)
    for key, scale, rm, want, sel in (("grad", "scale", "room_grad", beta, on), ("node_values", "scale_node", "room_node", LD(A0) + X @ beta, computed)):
        d_ref = D.dist(re[key][0], ex[key][0], ex[scale][0])
        assert d_ref <= D.CASE_CAP
        bar = max(SLACK * d_ref, ADJOINT_RTOL)
        err = np.abs(np.asarray(got[key][0], dtype=LD) - want)[sel]
        err80 = np.abs(ex[key][0] - want)[sel]
        allowed = 2 * ex[rm][0][sel] + bar * ex[scale][0][sel]          # (twice the room: tests/test_gls_gradient_model.py's linear_errors)
        print(f"{c.name} {key}: device from the exact answer {float(err.max()):.2e}, the 80-bit model {float(err80.max()):.2e}, "
              f"worst share of what is allowed {float((err / allowed).max()):.2e}")
        assert np.all(err80 <= 2 * ex[rm][0][sel]) and np.all(err <= allowed)
    assert not got["grad"][0][~on].any() and not got["node_values"][0][~computed].any()


def test_local_updates_answer_like_a_fresh_mesh():
    """after update_points(nodes=...) and update_permeability(cells=...) the next call reads the new state: bit for bit a fresh load_mesh()"""
    c = Case("mixed")                       # its own Interpolator: the updates rewrite what is resident
    before = c.device()
    rng = np.random.default_rng(55)
    cells = rng.choice(c.E, size=max(c.E // 10, 2), replace=False)
    nodes = rng.choice(c.P, size=max(c.P // 20, 2), replace=False)
    X0 = np.ascontiguousarray(np.asarray(c.mesh.points, dtype=np.float64))
    X1 = X0.copy()
    X1[nodes] += 0.003 * np.sin(37.0 * X0[nodes] + 1.0)
    K1 = c.perm.copy()
    K1[cells] = c.perm[cells] * 1.5 + np.eye(3).reshape(9) * 0.25
    c.I.update_points(X1[nodes], nodes=nodes)
    c.I.update_permeability(K1[cells], cells=cells)
    after = c.device()
    moved = copy.deepcopy(c.mesh)
    moved.points = X1
    cuts = np.cumsum([len(b) for b in moved.cells])[:-1]
    moved.cell_data["permeability"] = np.split(np.ascontiguousarray(K1), cuts)
    fresh = Case("mixed, fresh", mesh=moved).device(c.u)
    for o in OUTPUTS:
        assert after[o].tobytes() == fresh[o].tobytes(), o
    assert after["grad"].tobytes() != before["grad"].tobytes()


def test_wrappers_return_what_the_launch_wrote():
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    c = get_case("tet")
    want = c.device()
    grad, flux = c.I.corner_gradients("u", c.u, flux=True)
    assert grad.shape == (N_FIELDS, c.nnz, 3) and flux.shape == grad.shape and grad.dtype == np.float64
    assert grad.tobytes() == want["grad"].tobytes() and flux.tobytes() == want["flux"].tobytes()
    g1 = c.I.corner_gradients("u", c.u[1])
    assert g1.shape == (c.nnz, 3) and g1.tobytes() == want["grad"][1].tobytes()
    own = c.I.corner_gradients("u")                                      # the cell variable itself
    assert own.shape == (c.nnz, 3) and np.all(np.isfinite(own)) and np.abs(own).max() > 0
    ng = c.I.node_gradient("u", c.u)
    assert ng.shape == (N_FIELDS, c.P, 3) and ng.tobytes() == want["node_gradient"].tobytes()
    assert c.I.node_gradient("u", c.u[2]).tobytes() == want["node_gradient"][2].tobytes()
    p = int(np.flatnonzero(c.model(np.float64)["computed"])[0])          # the docstring's indexing: node p's cells and their gradients
    assert len(c.esup[c.ptr[p]:c.ptr[p + 1]]) == len(g1[c.ptr[p]:c.ptr[p + 1]]) and np.abs(g1[c.ptr[p]:c.ptr[p + 1]]).max() > 0
    with pytest.raises(ValueError):
        c.I.corner_gradients("u", c.u[:, :-1])
    op = CellToNode(c.I, "u", "gls")
    u = torch.from_numpy(c.u).to(c.dev).requires_grad_()
    out = op.corner_gradients(u)
    assert not out.requires_grad and out.grad_fn is None                 # no autograd through the gradients
    assert tuple(out.shape) == (N_FIELDS, c.nnz, 3) and out.cpu().numpy().tobytes() == want["grad"].tobytes()
    assert op.corner_gradients(u[0]).cpu().numpy().tobytes() == want["grad"][0].tobytes()
    with pytest.raises(TypeError):
        op.corner_gradients(c.u)
    with pytest.raises(TypeError):
        op.corner_gradients(u.detach().float())


def test_a_plan_of_another_method_is_refused():
    from ninpol_amd.interpolator import DevicePlan
    c = get_case("tet")
    for meth in ("idw", "ls"):
        with pytest.raises(ValueError, match="launch_corner_gradients is GLS only"):
            DevicePlan(c.I, "u", meth).launch_corner_gradients(8, 8)


def test_a_two_dimensional_grid_is_refused_and_nothing_is_written():
    import ninpol_amd
    from ninpol_amd import _lib
    torch = _torch()
    mesh = M.attach_fields(M.quad_tri_mesh_2d(4), "u", perm="LIN", neumann_plane=(1, 0.0), seed=5)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    I.grid.to_device(I.device)
    dev = torch.zeros(1 << 12, dtype=torch.float64, device="cuda")
    assert int(I.grid.dim) == 2 and int(I.grid.nnz_esup) * 3 <= 1 << 12
    vp = _lib._vp(dev.data_ptr())
    rc = _lib.load().nin_gls_corner_gradients_device(I.grid._h, 1, vp, vp, vp, vp, vp, None)
    text = _lib.load().nin_last_error().decode()
    assert rc == _lib.NIN_EINVAL and text == "the corner gradients are for 3-D grids only (this grid is 2-D)", (rc, text)
    assert not dev.any().item()


# ---- every system in global-memory scratch ------------------------------------------------------------------------------------------

def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    check_model(c, " forced global")
    a, b = c.device(), c.device()
    for o in OUTPUTS:
        assert a[o].tobytes() == b[o].tobytes(), o
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
