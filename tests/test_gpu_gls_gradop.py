"""The kept corner-gradient operator on the device: DevicePlan.gradient_operator -> GlsGradientOperator,
Interpolator.gradient_operator -> GradientOperator and CellToNode.gradient_operator -> KeptGradients, on the meshes of
tests/test_gpu_gls_corner_gradients.py (jitter, the Neumann plane z = 0, the ALH tensor; the Delaunay mesh fills every adjoint bin).

  1. Columns, every entry, bit for bit: the cells are coloured so that no two of a colour share a node; the field that is 1 on a colour
     goes through launch_corner_gradients -- which tests/test_gpu_gls_corner_gradients.py holds to the 80-bit model -- and at node p the
     output for the colour of cells[j] must be column j of fetch(), byte for byte, for every node.  The operator's buffer is filled with
     NaN before the factorisation: zero rows are exact zeros that the factorisation wrote.
  2. The two products of three random fields in one launch against the stated sums over fetch(): inside (n_terms + 2) u sum |terms| of
     the 80-bit sums (tests/gls_gradop_model.py derives the bar; nothing in it is measured), and bit for bit the float64 restatement.
  3. flux and node_gradient of the apply path are numpy's stated expressions on the apply path's own grad, bit for bit.
  4. Two calls agree bit for bit, a batch equals its fields one by one (five fields: a chunk of four and one), both products.
  5. After a local update_permeability(cells=), update_points(nodes=) and update_neumann_flags(nodes=), each in turn, the products raise
     NIN_ESTATE and write nothing; after factorize() fetch() is, bit for bit, that of a fresh load_mesh() of the changed mesh.
  6. The wrappers: scipy's rmatvec against to_scipy().T @ v to the bar of 2; torch.autograd.grad of sum(op(u) . cg) and of
     sum(grad . cg + flux . cf) against explicit launch_apply_transpose calls on the cotangent (the flux's folded in by the stated
     expression), bit for bit; forward_ad against op(du); the refusals.
  7. The factorisation with every system in global-memory scratch (a child process): fetch() bit-identical to the LDS run.

apply(u) against launch_corner_gradients(u) on random u has no bar (the two differ by the conditioning of each node's solve); the
worst distance on DESIGN.md 4.21's scale is printed.  Measured on an MI355X: see DESIGN.md 4.22."""
import copy
import ctypes
import hashlib
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
import gls_gradop_model as GO  # noqa: E402
import test_gpu_gls_corner_gradients as CG  # noqa: E402
from gls_exact import LD  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu

N_FIELDS = CG.N_FIELDS
COLOURS_PER_LAUNCH = 8


def _torch():
    import torch
    return torch


class _DevicePointer:
    """n float64 values at a device address, as torch.as_tensor reads them (the CUDA array interface, version 2)"""

    def __init__(self, address, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(address), False), "version": 2, "strides": None}


class Op:
    """a corner-gradients case (CG.Case) with a kept operator on it, the operator fetched once"""

    def __init__(self, case, prefill=True):
        torch = _torch()
        from ninpol_amd.interpolator import GlsGradientOperator
        self.c = c = case
        c.plan.ensure_current()
        self.op = op = GlsGradientOperator(c.grid, plan=c.plan)
        assert op.stale
        if prefill and op.n_values:                                      # the object's own buffer, NaN in every entry before the factorisation
            view = torch.as_tensor(_DevicePointer(op.record_ptrs[1], op.n_values), device=c.dev)
            view.fill_(float("nan"))
            torch.cuda.synchronize(c.dev)
            del view
        op.factorize(c.stream())
        assert not op.stale
        self.gop_ptr, self.gop = op.fetch()
        rng = np.random.default_rng(31)
        self.u = c.u                                                     # [3][E]
        self.v = rng.uniform(-1.0, 1.0, (N_FIELDS, c.nnz, 3))

    def apply(self, u, want=("grad",)):
        torch = _torch()
        c = self.c
        u = np.atleast_2d(u)
        k = u.shape[0]
        shapes = {"grad": (k, c.nnz, 3), "flux": (k, c.nnz, 3), "node_gradient": (k, c.P, 3)}
        bufs = {o: torch.full(shapes[o], float("nan"), dtype=torch.float64, device=c.dev) for o in want}
        ptr = lambda o: bufs[o].data_ptr() if o in bufs else 0          # noqa: E731
        ud = torch.from_numpy(np.ascontiguousarray(u)).to(c.dev)
        self.op.launch_apply(ud.data_ptr(), ptr("grad"), k, ptr("flux"), ptr("node_gradient"), c.stream())
        torch.cuda.synchronize(c.dev)
        return {o: b.cpu().numpy() for o, b in bufs.items()}

    def apply_transpose(self, v):
        torch = _torch()
        c = self.c
        v = np.ascontiguousarray(v).reshape(-1, c.nnz, 3)
        out = torch.full((v.shape[0], c.E), float("nan"), dtype=torch.float64, device=c.dev)
        vd = torch.from_numpy(v).to(c.dev)
        self.op.launch_apply_transpose(vd.data_ptr(), out.data_ptr(), v.shape[0], c.stream())
        torch.cuda.synchronize(c.dev)
        return out.cpu().numpy()


_OPS = {}


def get_op(name):
    if name not in _OPS:
        _OPS[name] = Op(CG.get_case(name))
    return _OPS[name]


@pytest.fixture(params=sorted(CG.MESHES))
def op(request):
    return get_op(request.param)


def test_columns_are_the_corner_gradients_of_the_indicators_bit_for_bit(op):
    c = op.c
    assert np.array_equal(op.gop_ptr, GO.gop_ptr(c.ptr)) and op.gop_ptr.dtype == np.int64 and len(op.gop) == op.gop_ptr[-1]
    assert np.all(np.isfinite(op.gop))                                   # every entry of the NaN-filled buffer was written
    colour = GO.colour_cells(c.ptr, c.esup, c.E)
    fields = GO.indicator_fields(colour)
    grad = np.concatenate([c.device(fields[k:k + COLOURS_PER_LAUNCH], want=("grad",))["grad"]
                           for k in range(0, len(fields), COLOURS_PER_LAUNCH)])
    want = GO.gop_from_fields(c.ptr, c.esup, colour, grad)
    assert np.count_nonzero(want) > 0 and op.gop.tobytes() == want.tobytes()
    computed = c.model(np.float64)["computed"]
    for p in np.flatnonzero(~computed):
        assert not op.gop[op.gop_ptr[p]:op.gop_ptr[p + 1]].any(), p
    print(f"{c.name}: {len(fields)} colours, {len(op.gop)} values, {int(computed.sum())} of {c.P} nodes computed")


def _held(tag, got, exact, mag, n_terms):
    err = np.abs(got.astype(LD) - exact)
    bar = (n_terms + 2) * LD(GO.U64) * mag
    on = bar > 0
    worst = float((err[on] / bar[on]).max()) if on.any() else 0.0
    print(f"{tag}: worst share of the summation bound {worst:.3f}")
    assert np.count_nonzero(exact) > 0 and np.all(err <= bar), tag


def test_products_against_the_fetched_operator(op):
    c = op.c
    got = op.apply(op.u)["grad"]
    _held(c.name + " apply", got, GO.apply(c.ptr, c.esup, op.gop, op.u, LD), GO.apply(c.ptr, c.esup, op.gop, op.u, LD, True),
          GO.apply_terms(c.ptr)[None])
    assert got.tobytes() == GO.apply(c.ptr, c.esup, op.gop, op.u).tobytes()
    gt = op.apply_transpose(op.v)
    _held(c.name + " transposed", gt, GO.apply_transpose(c.ptr, c.esup, op.gop, op.v, c.E, LD),
          GO.apply_transpose(c.ptr, c.esup, op.gop, op.v, c.E, LD, True), GO.transpose_terms(c.ptr, c.esup, c.E)[None])
    assert gt.tobytes() == GO.apply_transpose(c.ptr, c.esup, op.gop, op.v, c.E).tobytes()
    # no bar: the distance from the per-call solve on the 80-bit model's scale, for the record
    exact = c.model(LD)
    direct = c.device(want=("grad",))["grad"]
    print(f"{c.name}: apply(u) from launch_corner_gradients(u), worst of the fields on the model's scale "
          f"{max(D.dist(got[f], direct[f], exact['scale'][f]) for f in range(N_FIELDS)):.2e}; from the 80-bit model "
          f"{max(D.dist(got[f], exact['grad'][f], exact['scale'][f]) for f in range(N_FIELDS)):.2e}")


def test_flux_and_node_gradient_follow_the_applied_gradients_bit_for_bit(op):
    c = op.c
    got = op.apply(op.u, want=("grad", "flux", "node_gradient"))
    K = c.perm[c.esup]
    g = got["grad"]
    want = np.stack([-((K[:, 3 * k + 0] * g[:, :, 0] + K[:, 3 * k + 1] * g[:, :, 1]) + K[:, 3 * k + 2] * g[:, :, 2]) for k in range(3)], axis=2)
    assert np.count_nonzero(want) > 0 and got["flux"].tobytes() == np.ascontiguousarray(want).tobytes()
    cnt = np.diff(c.ptr)
    acc = np.zeros((N_FIELDS, c.P, 3))
    for j in range(int(cnt.max())):
        on = cnt > j
        acc[:, on] += g[:, c.ptr[:-1][on] + j]
    mean = acc / cnt[None, :, None]
    assert cnt.min() > 0 and np.count_nonzero(mean) > 0 and got["node_gradient"].tobytes() == np.ascontiguousarray(mean).tobytes()


def test_two_calls_agree_and_a_batch_equals_its_fields(op):
    c = op.c
    rng = np.random.default_rng(37)
    u5, v5 = rng.uniform(-1, 1, (5, c.E)), rng.uniform(-1, 1, (5, c.nnz, 3))
    want = ("grad", "flux", "node_gradient")
    a, b = op.apply(u5, want), op.apply(u5, want)
    ta, tb = op.apply_transpose(v5), op.apply_transpose(v5)
    assert np.all(np.isfinite(ta)) and ta.tobytes() == tb.tobytes()
    for o in want:
        assert np.all(np.isfinite(a[o])) and a[o].tobytes() == b[o].tobytes(), o
    for f in range(5):
        one = op.apply(u5[f], want)
        for o in want:
            assert one[o][0].tobytes() == a[o][f].tobytes(), (o, f)
        assert op.apply_transpose(v5[f])[0].tobytes() == ta[f].tobytes(), f


def test_a_batch_of_seven_equals_its_fields_one_by_one():
    """a full chunk of four and a chunk of three behind it, both products, on the smallest mesh"""
    op = get_op("tet")
    c = op.c
    seven = lambda x: np.concatenate([x, 0.5 * x, -3.0 * x])[:7]          # noqa: E731  (the module's three fields, and scaled copies)
    u7, v7 = seven(op.u), seven(op.v)
    g = op.apply(u7)["grad"]
    assert g.shape == (7, c.nnz, 3) and g[6].any() and g.tobytes() == np.stack([op.apply(u7[f])["grad"][0] for f in range(7)]).tobytes()
    t = op.apply_transpose(v7)
    assert t.shape == (7, c.E) and t[6].any() and t.tobytes() == np.stack([op.apply_transpose(v7[f])[0] for f in range(7)]).tobytes()


def test_every_bin_is_populated_on_the_delaunay_mesh():
    plan = get_op("delaunay").c.grid.gls_adjoint_plan()
    assert all(v > 0 for v in plan.values()), plan


# ---- staleness ---------------------------------------------------------------------------------------------------------------------------

def _refused(o):
    from ninpol_amd import _lib
    torch = _torch()
    c = o.c
    assert o.op.stale
    ud = torch.from_numpy(c.u).to(c.dev)
    vd = torch.from_numpy(o.v).to(c.dev)
    out_g = torch.zeros((N_FIELDS, c.nnz, 3), dtype=torch.float64, device=c.dev)
    out_u = torch.zeros((N_FIELDS, c.E), dtype=torch.float64, device=c.dev)
    for call in (lambda: o.op.launch_apply(ud.data_ptr(), out_g.data_ptr(), N_FIELDS, stream=c.stream()),
                 lambda: o.op.launch_apply_transpose(vd.data_ptr(), out_u.data_ptr(), N_FIELDS, c.stream())):
        with pytest.raises(_lib.NinpolError) as e:
            call()
        assert e.value.code == _lib.NIN_ESTATE and "call nin_gls_gradop_factorize again" in e.value.text, e.value.text
    torch.cuda.synchronize(c.dev)
    assert not out_g.any().item() and not out_u.any().item()


def _fresh_fetch(mesh):
    return Op(CG.Case("fresh", mesh=mesh), prefill=False).gop


def test_staleness_and_factorize_after_each_local_update():
    c = CG.Case("mixed")                    # its own Interpolator: the updates rewrite what is resident
    o = Op(c)
    before = o.gop
    rng = np.random.default_rng(55)
    mesh = copy.deepcopy(c.mesh)
    cuts = np.cumsum([len(b) for b in mesh.cells])[:-1]
    # the permeability of some cells
    cells = rng.choice(c.E, size=max(c.E // 10, 2), replace=False)
    K1 = c.perm.copy()
    K1[cells] = c.perm[cells] * 1.5 + np.eye(3).reshape(9) * 0.25
    c.I.update_permeability(K1[cells], cells=cells)
    _refused(o)
    o.op.factorize(c.stream())
    mesh.cell_data["permeability"] = np.split(np.ascontiguousarray(K1), cuts)
    after_k = o.op.fetch()[1]
    assert after_k.tobytes() == _fresh_fetch(copy.deepcopy(mesh)).tobytes() and after_k.tobytes() != before.tobytes()
    # the coordinates of some nodes
    nodes = rng.choice(c.P, size=max(c.P // 20, 2), replace=False)
    X0 = np.ascontiguousarray(np.asarray(c.mesh.points, dtype=np.float64))
    X1 = X0.copy()
    X1[nodes] += 0.003 * np.sin(37.0 * X0[nodes] + 1.0)
    c.I.update_points(X1[nodes], nodes=nodes)
    _refused(o)
    o.op.factorize(c.stream())
    mesh.points = X1
    after_x = o.op.fetch()[1]
    assert after_x.tobytes() == _fresh_fetch(copy.deepcopy(mesh)).tobytes() and after_x.tobytes() != after_k.tobytes()
    # the Neumann flags of some nodes of the plane z = 0: computed rows become zero rows, whose blocks must be overwritten with zeros
    f0 = np.array(c.mesh.point_data["neumann_flag_u"], dtype=np.float64)
    flagged = np.flatnonzero(f0 != 0)
    off = flagged[::2]
    assert len(off) > 0
    c.I.update_neumann_flags("u", np.zeros(len(off)), nodes=off)
    _refused(o)
    o.op.factorize(c.stream())
    f1 = f0.copy()
    f1[off] = 0.0
    mesh.point_data["neumann_flag_u"] = f1
    after_f = o.op.fetch()[1]
    assert after_f.tobytes() == _fresh_fetch(copy.deepcopy(mesh)).tobytes() and after_f.tobytes() != after_x.tobytes()
    ptr = o.gop_ptr
    assert any(after_x[ptr[p]:ptr[p + 1]].any() for p in off) and not any(after_f[ptr[p]:ptr[p + 1]].any() for p in off)


# ---- wrappers ----------------------------------------------------------------------------------------------------------------------------

def test_scipy_operator():
    o = get_op("tet")
    c = o.c
    G = c.I.gradient_operator("u")
    assert G.shape == (3 * c.nnz, c.E) and G.dtype == np.float64
    A = G.to_scipy()
    assert A.shape == G.shape and A.nnz == len(o.gop)
    assert np.array_equal(A.toarray(), GO.dense(c.ptr, c.esup, o.gop, c.E))          # the same factorisation, bit for bit
    v = o.v[0].reshape(-1)
    got = G.rmatvec(v)
    exact = GO.apply_transpose(c.ptr, c.esup, o.gop, o.v[0], c.E, LD)
    mag = GO.apply_transpose(c.ptr, c.esup, o.gop, o.v[0], c.E, LD, True)
    _held("rmatvec", got[None], exact, mag, GO.transpose_terms(c.ptr, c.esup, c.E)[None])
    _held("to_scipy().T @ v", (A.T @ v)[None], exact, mag, GO.transpose_terms(c.ptr, c.esup, c.E)[None])
    assert G.matvec(o.u[0]).tobytes() == o.apply(o.u[0])["grad"].tobytes()
    assert G.matmat(o.u.T).T.tobytes() == o.apply(o.u)["grad"].reshape(N_FIELDS, -1).tobytes()
    assert G.rmatmat(o.v.reshape(N_FIELDS, -1).T).T.tobytes() == o.apply_transpose(o.v).tobytes()
    G.update()
    assert G.rmatvec(v).tobytes() == got.tobytes()
    G.release()


def test_torch_operator_backward_and_forward():
    torch = _torch()
    import torch.autograd.forward_ad as fwAD
    from ninpol_amd.torch_ops import CellToNode
    o = get_op("hex")
    c = o.c
    mod = CellToNode(c.I, "u", "gls")
    kept = mod.gradient_operator()
    assert kept.operator.fetch()[1].tobytes() == o.gop.tobytes()
    rng = np.random.default_rng(41)
    cg, cf = rng.uniform(-1, 1, (N_FIELDS, c.nnz, 3)), rng.uniform(-1, 1, (N_FIELDS, c.nnz, 3))
    cgd, cfd = torch.from_numpy(cg).to(c.dev), torch.from_numpy(cf).to(c.dev)
    u = torch.from_numpy(c.u).to(c.dev).requires_grad_()
    out = kept(u)
    assert out.requires_grad and out.detach().cpu().numpy().tobytes() == o.apply(c.u)["grad"].tobytes()
    (gu,) = torch.autograd.grad((out * cgd).sum(), u)
    assert gu.cpu().numpy().tobytes() == o.apply_transpose(cg).tobytes()                # the first explicit call: the cotangent itself
    grad, flux = kept(u, flux=True)
    both = o.apply(c.u, ("grad", "flux"))
    assert grad.detach().cpu().numpy().tobytes() == both["grad"].tobytes() and flux.detach().cpu().numpy().tobytes() == both["flux"].tobytes()
    (gu2,) = torch.autograd.grad((grad * cgd).sum() + (flux * cfd).sum(), u)
    K = c.perm[c.esup].reshape(-1, 3, 3)                                                # the fold, restated: gbar += -K_e^T fbar
    back = np.stack([-((K[:, 0, d] * cf[..., 0] + K[:, 1, d] * cf[..., 1]) + K[:, 2, d] * cf[..., 2]) for d in range(3)], axis=-1)
    assert gu2.cpu().numpy().tobytes() == o.apply_transpose(cg + back).tobytes()        # the second: the folded cotangent
    one = kept(u[1])
    assert tuple(one.shape) == (c.nnz, 3) and one.detach().cpu().numpy().tobytes() == both["grad"][1].tobytes()
    du = torch.from_numpy(rng.uniform(-1, 1, (N_FIELDS, c.E))).to(c.dev)
    with fwAD.dual_level():
        tg, tf = (fwAD.unpack_dual(t).tangent for t in kept(fwAD.make_dual(u.detach(), du), flux=True))
    lin = kept(du, flux=True)
    assert tg.cpu().numpy().tobytes() == lin[0].cpu().numpy().tobytes() and tf.cpu().numpy().tobytes() == lin[1].cpu().numpy().tobytes()
    out2 = mod.corner_gradients(u)                                                       # unchanged: still no graph
    assert not out2.requires_grad
    with pytest.raises(TypeError):
        kept(c.u)


def test_refusals():
    from ninpol_amd import _lib
    from ninpol_amd.interpolator import DevicePlan, GlsGradientOperator
    import ninpol_amd
    torch = _torch()
    c = CG.get_case("tet")
    for meth in ("idw", "ls"):
        with pytest.raises(ValueError, match="gradient_operator is GLS only"):
            DevicePlan(c.I, "u", meth).gradient_operator()
    c.plan.ensure_current()
    raw = GlsGradientOperator(c.grid, plan=c.plan)                       # created, never factorised
    buf = torch.zeros(3 * c.nnz, dtype=torch.float64, device=c.dev)
    for call in (lambda: raw.launch_apply(buf.data_ptr(), buf.data_ptr(), 1, stream=c.stream()),
                 lambda: raw.launch_apply_transpose(buf.data_ptr(), buf.data_ptr(), 1, c.stream()),
                 lambda: raw.fetch()):
        with pytest.raises(_lib.NinpolError) as e:
            call()
        assert e.value.code == _lib.NIN_ESTATE and "has not been factorised" in e.value.text
    with pytest.raises(_lib.NinpolError) as e:
        raw.launch_apply(buf.data_ptr(), buf.data_ptr(), 0)
    assert e.value.code == _lib.NIN_EINVAL and e.value.text == "n must be >= 1"
    torch.cuda.synchronize(c.dev)
    assert not buf.any().item() and raw.stale
    assert raw.nbytes >= 8 * raw.n_values and raw.n_values == int((3 * np.diff(c.ptr) ** 2).sum())
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().nin_gls_gradop_bytes(c.grid._h, ctypes.byref(n)))
    assert n.value == 8 * raw.n_values
    raw.release()
    mesh = M.attach_fields(M.quad_tri_mesh_2d(4), "u", perm="LIN", neumann_plane=(1, 0.0), seed=5)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    I.grid.to_device(I.device)
    with pytest.raises(_lib.NinpolError) as e:
        GlsGradientOperator(I.grid)
    assert e.value.code == _lib.NIN_EINVAL and e.value.text == "the gradient operator is for 3-D grids only (this grid is 2-D)"


# ---- every system in global-memory scratch -------------------------------------------------------------------------------------------

def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = CG.get_case("hex")
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    o = Op(c)
    print("GOP SHA256", hashlib.sha256(o.gop.tobytes()).hexdigest(), len(o.gop))
    print("CHILD OK")


def test_forced_global_class():
    """the hexahedron mesh factorised with every system in global-memory scratch, in a fresh process (the switch is read when the bins
    are made): the operator is, bit for bit, the one the LDS bins give here"""
    o = get_op("hex")
    plan = o.c.grid.gls_adjoint_plan()
    assert plan["global"] < o.c.P, plan
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout
    assert f"GOP SHA256 {hashlib.sha256(o.gop.tobytes()).hexdigest()} {len(o.gop)}" in r.stdout


if __name__ == "__main__":
    _child()
