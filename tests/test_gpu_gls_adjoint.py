"""The GLS weights differentiated with respect to the permeability, on the device: DevicePlan.launch_weights_backward / launch_sddmm,
Grid.gls_adjoint_plan, Interpolator.permeability_gradient and the torch op CellToNode(u, K, scale), held to the numpy model of
tests/gls_adjoint_model.py (which tests/test_gls_adjoint_model.py pins against central differences of the oracle).

Every mesh carries the Neumann plane z = 0: Neumann rows, the neumann_ws fold, zero-row corners and Dirichlet rows are all in.  The
random-cloud Delaunay mesh has systems from 0.1 to 322 KiB (slots of the adjoint kernel: 0.3 to 333 KiB): every bin of the adjoint kernel is populated without a switch.

A cell's gradient is a sum of signed terms, one per (node, face row): the error is measured per cell against the model's sum of the
absolute values of those terms."""
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

import gls_adjoint_model as GM  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu

# Device gradient against the model, per cell, relative to the model's absolute-contribution scale.  Measured on an MI355X over the
# four meshes below, all call variants: 5.06e-12 at worst (grad_diff_mag on the Delaunay mesh; grad_perm 3.48e-12 there, 1e-13 to
# 5e-13 on the three others).  The bar is 10 x the worst value, well inside the 1e-9 at which the model itself is pinned
# (it may never be looser than that).
# Those figures are distances from the lstsq MODEL, and on the Delaunay mesh they contain the model's own distance from the exact
# derivative: against the 80-bit model of tests/gls_derivative_exact.py (the same inputs) the lstsq model is 3.48e-12 (grad_perm) and
# 4.19e-12 (grad_diff_mag) away, the device 4.6e-14 and 4.09e-12 (tests/test_gpu_gls_derivative_exact.py, profiles/r17) -- the
# grad_perm figure above is the model's error to three digits, not the kernel's.  On the three other meshes the model is 1.1e-13 to
# 3.1e-13 from exact, the device 8e-15 to 1.3e-14 (grad_perm) and 1.8e-13 to 3.9e-13 (grad_diff_mag).  The bar stays where it is:
# it bounds the distance between the device and this model, and the model's share of it is what it is.
ADJOINT_RTOL = 5.1e-11

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
    """one mesh on the device, its tables on the host, an upstream gradient and the model's answers (computed once, lazily)"""

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
        rng = np.random.default_rng(17)
        self.ghat = rng.uniform(-1.0, 1.0, self.nnz)
        self.gnws = rng.uniform(-1.0, 1.0, self.P)
        self._models = {}

    def model(self, add_neumann=True, with_nws=True, ghat=None, key=None):
        key = key or (add_neumann, with_nws)
        if key not in self._models:
            self._models[key] = GM.gls_adjoint_model(self.grid, self.perm, self.dmag, self.flag, self.ghat if ghat is None else ghat,
                                                     add_neumann=add_neumann, grad_neumann_ws=self.gnws if with_nws else None)
        return self._models[key]

    def device(self, add_neumann=True, with_nws=True, unfolded=True, ghat=None):
        """(grad_perm [E][9], grad_diff_mag [E] or None) from DevicePlan.launch_weights_backward"""
        torch = _torch()
        dev = torch.device("cuda", int(self.I.device))
        g = torch.from_numpy(self.ghat if ghat is None else ghat).to(dev)
        gn = torch.from_numpy(self.gnws).to(dev) if with_nws else None
        gp = torch.full((self.E, 9), float("nan"), dtype=torch.float64, device=dev)
        gd = torch.full((self.E,), float("nan"), dtype=torch.float64, device=dev) if unfolded else None
        self.plan.launch_weights_backward(g.data_ptr(), gp.data_ptr(), gd.data_ptr() if unfolded else 0, gn.data_ptr() if with_nws else 0,
                                          torch.cuda.current_stream(dev).cuda_stream, add_neumann=add_neumann)
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


def scaled_err(a, b, scale):
    """max over cells of |a - b| / scale (a, b: [E] or [E][9], scale [E]); where the scale is 0 both must be exactly 0"""
    a, b = np.asarray(a).reshape(len(scale), -1), np.asarray(b).reshape(len(scale), -1)
    assert np.all(np.isfinite(a)), "the device result is not finite (or was not written)"
    none = scale == 0
    assert np.all(a[none] == 0.0) and np.all(b[none] == 0.0)
    d = np.abs(a - b).max(axis=1)
    return float((d[~none] / scale[~none]).max()) if (~none).any() else 0.0


def check(tag, gp, gd, m):
    e_perm = scaled_err(gp, m["grad_perm"], m["scale_perm"])
    e_dm = scaled_err(gd, m["grad_diff_mag"], m["scale_diff_mag"]) if gd is not None else 0.0
    print(f"{tag}: grad_perm {e_perm:.2e}, grad_diff_mag {e_dm:.2e} of the absolute-contribution scale")
    assert e_perm <= ADJOINT_RTOL and e_dm <= ADJOINT_RTOL, (tag, e_perm, e_dm)


def folded_scale(m, perm):
    return m["scale_perm"] + m["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(perm))


def test_against_the_model(case):
    """grad_perm and grad_diff_mag, add_neumann, dL/dneumann_ws given; the model's forward is the library's own weights"""
    m = case.model()
    assert np.count_nonzero(m["grad_perm"]) > 0 and np.count_nonzero(m["grad_diff_mag"]) > 0
    assert np.count_nonzero(m["neumann_ws"]) > 0 and not m["computed"].all()
    W, nws = case.I.interpolate("u", "gls")
    dense = np.asarray(W.todense())
    ptr, esup = np.asarray(case.grid.esup_ptr), np.asarray(case.grid.esup)
    rows = np.repeat(np.arange(case.P), np.diff(ptr))
    assert np.abs(dense[rows, esup] - m["weights"]).max() <= 1e-10 * np.abs(m["weights"]).max()
    gp, gd = case.device()
    check(case.name, gp, gd, m)


def test_without_add_neumann_and_without_grad_neumann_ws(case):
    m = case.model(add_neumann=False, with_nws=False)
    gp, gd = case.device(add_neumann=False, with_nws=False)
    check(case.name + " add_neumann=False", gp, gd, m)
    # both terms really enter: the Neumann nodes' cells answer differently with them
    full = case.model()
    assert np.abs(full["grad_perm"] - m["grad_perm"]).max() > 1e-6 * np.abs(full["grad_perm"]).max()
    only_nws = case.model(add_neumann=False, with_nws=True)
    assert np.abs(only_nws["grad_perm"] - m["grad_perm"]).max() > 1e-6 * np.abs(full["grad_perm"]).max()
    gp2, gd2 = case.device(add_neumann=False, with_nws=True)
    check(case.name + " add_neumann=False, grad_neumann_ws", gp2, gd2, only_nws)


def test_two_calls_agree_bit_for_bit(case):
    a, b = case.device(), case.device()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    a, b = case.device(unfolded=False), case.device(unfolded=False)
    assert a[0].tobytes() == b[0].tobytes()


def test_folded_is_unfolded_plus_the_chain_rule(case):
    gp, gd = case.device()
    folded, none = case.device(unfolded=False)
    assert none is None
    expect = GM.fold(gp, gd, case.perm)
    scale = folded_scale(case.model(), case.perm)
    assert scaled_err(folded, expect, scale) <= 1e-14        # the same sums, one fused step apart
    assert np.abs(folded - gp).max() > 0


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    plan = c.grid.gls_adjoint_plan()
    counts, sizes = GM.adjoint_bins(c.grid)
    print(f"delaunay: adjoint bins {plan}, systems {sizes.min() / 1024:.1f} .. {sizes.max() / 1024:.1f} KiB")
    assert list(plan) == ["lds1", "lds2", "lds4", "global"] and list(plan.values()) == counts
    assert all(v > 0 for v in plan.values()), plan
    assert sum(plan.values()) == c.P


CHILD = """the hexahedron mesh with every node in the global-scratch class (NIN_GLS_ADJ_FORCE_GLOBAL=1)"""


def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    gp, gd = c.device()
    check("hex, forced global", gp, gd, c.model())
    a = c.device()
    assert a[0].tobytes() == gp.tobytes() and a[1].tobytes() == gd.tobytes()
    print("CHILD OK")


def test_forced_global_class():
    """the same comparison with every system in global-memory scratch, in a fresh process (the switch is read when the bins are made)"""
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


def test_permeability_gradient_against_the_model():
    c = get_case("mixed")
    rng = np.random.default_rng(3)
    v = rng.uniform(-1.0, 1.0, (2, c.P))
    u = rng.uniform(-1.0, 1.0, (2, c.E))
    ptr, esup = np.asarray(c.grid.esup_ptr), np.asarray(c.grid.esup)
    rows = np.repeat(np.arange(c.P), np.diff(ptr))
    for tag, vv, uu, arg in (("k = 2", v, u, u), ("the cell variable", v[0], None, None)):
        if uu is None:
            uu = np.asarray(c.I.cells_data[c.I.variable_to_index["cells"]["u"]])[:c.E]
        ghat = (np.atleast_2d(vv)[:, rows] * np.atleast_2d(uu)[:, esup]).sum(axis=0)
        m = c.model(add_neumann=True, with_nws=False, ghat=ghat, key=("pg", tag))
        got = c.I.permeability_gradient("u", vv, arg)
        assert got.shape == (c.E, 3, 3) and got.dtype == np.float64
        err = scaled_err(got, GM.fold(m["grad_perm"], m["grad_diff_mag"], c.perm), folded_scale(m, c.perm))
        print(f"permeability_gradient, {tag}: {err:.2e}")
        assert err <= ADJOINT_RTOL
    # <v, W(K) u> really moves that way: one central difference through the library's own apply()
    e, k, h = c.E // 2, 4, 1e-5
    base = c.perm.copy()
    vals = []
    try:
        for sgn in (+1, -1):
            Kq = base.copy()
            Kq[e, k] += sgn * h
            c.I.update_permeability(Kq)
            vals.append(float((c.I.apply("u", "gls", values=u)[0] * v).sum()))
    finally:
        c.I.update_permeability(base)
    g = c.I.permeability_gradient("u", v, u)
    fd = (vals[0] - vals[1]) / (2 * h)
    assert abs(fd - g[e, k // 3, k % 3]) <= 1e-6 * np.abs(g).max(), (fd, g[e, k // 3, k % 3])


def test_torch_op():
    """CellToNode(u, K, scale) on the mixed mesh, k = 2 fields"""
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    c = Case("mixed")                       # its own Interpolator: the op rewrites the resident permeability
    dev = torch.device("cuda", int(c.I.device))
    op = CellToNode(c.I, "u", "gls")
    rng = np.random.default_rng(9)
    u_np, v_np = rng.uniform(-1.0, 1.0, (2, c.E)), rng.uniform(-1.0, 1.0, (2, c.P))
    s_np = rng.uniform(0.5, 1.5, c.E)
    v = torch.from_numpy(v_np).to(dev)

    # without K: the module's weights, the kernels of the product alone -- what the op did before it knew K
    u0 = torch.from_numpy(u_np).to(dev).requires_grad_()
    out0 = op(u0)
    direct = torch.empty((2, c.P), dtype=torch.float64, device=dev)
    op.plan.launch_spmv(op.weights.data_ptr(), u0.data_ptr(), 2, direct.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert torch.equal(out0, direct)
    (out0 * v).sum().backward()
    direct_t = torch.empty((2, c.E), dtype=torch.float64, device=dev)
    op.plan.launch_spmv_transpose(op.weights.data_ptr(), v.data_ptr(), 2, direct_t.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert torch.equal(u0.grad, direct_t)
    updates = c.grid.field_updates

    # with K and scale
    K = torch.from_numpy(c.perm.reshape(c.E, 3, 3).copy()).to(dev).requires_grad_()
    scale = torch.from_numpy(s_np).to(dev).requires_grad_()
    u = torch.from_numpy(u_np).to(dev).requires_grad_()
    out = op(u, K, scale)
    assert c.grid.field_updates == updates + 1
    (out * v).sum().backward()
    perm = s_np[:, None] * c.perm                       # one multiplication per entry, as update_permeability forms it
    ptr, esup = np.asarray(c.grid.esup_ptr), np.asarray(c.grid.esup)
    rows = np.repeat(np.arange(c.P), np.diff(ptr))
    ghat = (v_np[:, rows] * u_np[:, esup]).sum(axis=0)
    m = GM.gls_adjoint_model(c.grid, perm, GM.diff_mag_of(perm), c.flag, ghat, add_neumann=True)
    gperm, sc = GM.fold(m["grad_perm"], m["grad_diff_mag"], perm), folded_scale(m, perm)
    eK = scaled_err(K.grad.cpu().numpy(), s_np[:, None] * gperm, s_np * sc)
    eS = scaled_err(scale.grad.cpu().numpy(), (c.perm * gperm).sum(axis=1), np.abs(c.perm).sum(axis=1) * sc)
    print(f"torch: dL/dK {eK:.2e}, dL/dscale {eS:.2e}")
    assert K.grad.shape == K.shape and eK <= ADJOINT_RTOL and eS <= ADJOINT_RTOL
    # d/du: bit for bit the existing path on the same weights
    op.recompute_weights()
    u1 = torch.from_numpy(u_np).to(dev).requires_grad_()
    out1 = op(u1)
    (out1 * v).sum().backward()
    assert torch.equal(out1, out) and torch.equal(u1.grad, u.grad)
    assert not torch.equal(out, out0)                   # (the scaled permeability gives other weights)

    # backward after an intervening update refuses
    K2 = K.detach().clone().requires_grad_()
    out2 = op(u.detach(), K2)
    c.I.update_permeability(K.detach())
    with pytest.raises(RuntimeError, match="field_updates"):
        (out2 * v).sum().backward()
    assert K2.grad is None
    # a differentiable weights tensor on its own
    K3 = K.detach().clone().requires_grad_()
    w, nws = op.weights_of(K3)
    assert w.shape == (c.nnz,) and nws.shape == (c.P,) and w.requires_grad
    # (random coefficients: the weights of a row sum to one, so the plain sum of the weights has no gradient to compare)
    ((w * torch.from_numpy(c.ghat).to(dev)).sum() + (nws * torch.from_numpy(c.gnws).to(dev)).sum()).backward()
    m3 = c.model()
    e3 = scaled_err(K3.grad.cpu().numpy(), GM.fold(m3["grad_perm"], m3["grad_diff_mag"], c.perm), folded_scale(m3, c.perm))
    print(f"torch: weights_of, dL/dK {e3:.2e}")
    assert e3 <= ADJOINT_RTOL

    # IDW does not depend on K: zeros
    op_idw = CellToNode(c.I, "u", "idw")
    K4 = K.detach().clone().requires_grad_()
    s4 = scale.detach().clone().requires_grad_()
    u4 = torch.from_numpy(u_np).to(dev).requires_grad_()
    out4 = op_idw(u4, K4, s4)
    assert torch.equal(out4, op_idw(u4.detach()))
    (out4 * v).sum().backward()
    assert K4.grad.shape == K4.shape and not K4.grad.any() and not s4.grad.any() and u4.grad.abs().sum() > 0
    # argument errors, by update_permeability's rules
    with pytest.raises(TypeError):
        op(u.detach(), c.perm)
    with pytest.raises(ValueError):
        op(u.detach(), K.detach().cpu())
    with pytest.raises(TypeError):
        op(u.detach(), K.detach().float())
    with pytest.raises(ValueError):
        op(u.detach(), K.detach()[:-1])
    with pytest.raises(ValueError):
        op(u.detach(), None, scale.detach())


def test_a_plan_of_another_method_is_refused():
    from ninpol_amd.interpolator import DevicePlan
    c = get_case("tet")
    with pytest.raises(ValueError, match="GLS only"):
        DevicePlan(c.I, "u", "idw").launch_weights_backward(8, 8)


def test_release_scratch_gives_the_adjoint_state_back():
    c = get_case("tet")
    a = c.device()
    c.grid.release_scratch()
    assert not c.grid.has_transpose_index
    b = c.device()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


if __name__ == "__main__":
    _child()
