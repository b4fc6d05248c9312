"""The adjoint of the interpolation operator on the device: Interpolator.apply_transpose, DevicePlan.launch_spmv /
launch_spmv_transpose and the torch op ninpol_amd.torch_ops.CellToNode.  W is the library's own interpolate() result (the
`+ neumann_ws[row]` of the Neumann rows included); the hybrid mesh of every GLS kernel family (the parts of
tests/test_gpu_composite.py, rebuilt here) with a Neumann plane puts every kernel's rows and the Neumann term into the transpose."""
import numpy as np
import pytest

from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

METHODS = ("gls", "idw", "ls")


def _parts():
    return [M.hex_mesh(16, jitter=0.1, seed=1), M.delaunay_tet_mesh(10, seed=4, lattice="random"), M.delaunay_tet_mesh(8, seed=2),
            M.tet_mesh(6, jitter=0.1, seed=3), M.wedge_mesh(6, 5, 4, jitter=0.05, seed=5), M.mixed_mesh(10, 5, 5, jitter=0.1, seed=6),
            M.delaunay_wedge_mesh(12, 6, seed=7, lattice="random"), M.wedge_fan(30, 3), M.wedge_fan(50, 2)]


def _loaded(mesh):
    import ninpol_amd
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    return I


@pytest.fixture(scope="module")
def C():
    parts = _parts()
    for i, p in enumerate(parts):
        M.attach_fields(p, "u", perm="ALH", neumann_plane=(2, 0.0), seed=20 + i)
    mesh = M.composite_mesh(parts)
    I = _loaded(mesh)
    W = {meth: I.interpolate("u", meth) for meth in METHODS}
    return {"mesh": mesh, "I": I, "W": W, "plan": I.grid.gls_plan(), "P": int(I.grid.n_points), "E": int(I.grid.n_elems)}


@pytest.fixture(scope="module")
def small():
    """a mixed hexahedron | pyramid | tetrahedron mesh of about a hundred cells, with a Neumann plane"""
    mesh = M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    return mesh


def _torch():
    import torch
    return torch


def _finite(W):
    """LS on layers of wedges has rows of non-finite weights (singular systems, the reference's too): those rows, the cells they
    touch, and |W| with the non-finite entries zeroed"""
    P, E = W.shape
    rows = np.repeat(np.arange(P), np.diff(W.indptr))
    bad = ~np.isfinite(W.data)
    bad_rows = np.zeros(P, dtype=bool)
    bad_rows[rows[bad]] = True
    bad_cols = np.zeros(E, dtype=bool)
    bad_cols[W.indices[bad]] = True
    A = abs(W)
    A.data = np.where(bad, 0.0, A.data)
    return bad_rows, bad_cols, A


def test_plan_covers_every_kernel_and_the_neumann_term(C):
    """The coverage test_gpu_composite.py asserts, so that the rows of every GLS kernel enter the transpose below; and the Neumann
    term is really there."""
    plan = C["plan"]
    for k in ("hex8", "mfg_tiles", "scratch", "quad4", "mfx_boundary"):
        assert plan[k] > 0, (k, plan)
    for fam in ("mfw_", "small", "block", "mfx_"):
        assert any(v > 0 for k, v in plan.items() if k.startswith(fam)), (fam, plan)
    assert np.count_nonzero(C["W"]["gls"][1]) > 0


@pytest.mark.parametrize("meth", METHODS)
def test_against_scipy(C, meth):
    """apply_transpose(v) against W.T @ v of interpolate()'s W, elementwise; cells without a weight are exactly 0; the cells a
    non-finite weight reaches get scipy's NaN / inf."""
    W, _ = C["W"][meth]
    v = np.random.default_rng(11).uniform(-1.0, 1.0, C["P"])
    x = C["I"].apply_transpose("u", meth, v)
    assert x.shape == (C["E"],) and x.dtype == np.float64
    ref = W.T @ v
    _, bad_cols, A = _finite(W)
    np.testing.assert_array_equal(x[bad_cols], ref[bad_cols])
    good = ~bad_cols
    bound = A.T @ np.abs(v)
    off = np.flatnonzero(good)[~(np.abs(x[good] - ref[good]) <= 1e-13 * bound[good])]
    assert len(off) == 0, (meth, off[:10], x[off[:10]], ref[off[:10]])
    empty = good & ((A.T @ np.ones(C["P"])) == 0)
    assert np.all(x[empty] == 0.0), meth
    assert np.count_nonzero(x[good]) > 0.9 * C["E"], meth


def _adjoint(I, meth, seed=0):
    """<W u, v> = <u, W^T v> to 1e-12 of sum |v| |W| |u|; u is 0 on the cells a non-finite row touches, v on those rows, and
    the sums leave them out"""
    W, _ = I.interpolate("u", meth)
    bad_rows, bad_cols, A = _finite(W)
    rng = np.random.default_rng(seed)
    u = np.where(bad_cols, 0.0, rng.uniform(-1.0, 1.0, I.grid.n_elems))
    v = np.where(bad_rows, 0.0, rng.uniform(-1.0, 1.0, I.grid.n_points))
    Wu, _ = I.apply("u", meth, values=u)
    WTv = I.apply_transpose("u", meth, v)
    lhs, rhs = float(Wu[~bad_rows] @ v[~bad_rows]), float(u[~bad_cols] @ WTv[~bad_cols])
    scale = float(np.abs(v) @ (A @ np.abs(u)))
    assert np.isfinite(lhs) and np.isfinite(rhs), meth
    assert abs(lhs - rhs) <= 1e-12 * scale, (meth, lhs, rhs)
    assert abs(lhs) > 1e-6 * scale, (meth, "vacuous")


@pytest.mark.parametrize("meth", METHODS)
def test_adjoint_identity_hybrid(C, meth):
    """<apply(u), v> = <u, apply_transpose(v)>: for GLS apply() runs the fused cube-node kernel, the transpose the unfused rows."""
    _adjoint(C["I"], meth)


@pytest.mark.parametrize("meth", ("idw", "ls"))
def test_adjoint_identity_2d(meth):
    mesh = M.quad_tri_mesh_2d(8, 6, jitter=0.1, seed=3)
    M.attach_fields(mesh, "u", perm="LIN", neumann_plane=(0, 0.0))
    I = _loaded(mesh)
    assert I.grid.dim == 2
    _adjoint(I, meth, seed=1)


@pytest.mark.parametrize("meth", METHODS)
def test_adjoint_identity_delaunay_wedges(meth):
    mesh = M.delaunay_wedge_mesh(12, 6, seed=7, lattice="random")
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(2, 0.0))
    _adjoint(_loaded(mesh), meth, seed=2)


@pytest.mark.parametrize("meth", METHODS)
def test_batches_and_determinism(C, meth):
    """k = 1, 2, 3, 5 fields (the 4-, 2- and 1-field kernels and the remainder pass): row f of a batch is the single call bit for
    bit, and a repeated call is bitwise identical -- also after the index was released and rebuilt."""
    I = C["I"]
    V = np.random.default_rng(5).standard_normal((5, C["P"]))
    singles = [I.apply_transpose("u", meth, V[f]) for f in range(5)]
    for k in (1, 2, 3, 5):
        X = I.apply_transpose("u", meth, V[:k])
        assert X.shape == (k, C["E"])
        for f in range(k):
            np.testing.assert_array_equal(X[f], singles[f], err_msg=f"{meth} k={k} f={f}")
    np.testing.assert_array_equal(I.apply_transpose("u", meth, V), X)
    I.release_scratch(pinned=False)
    np.testing.assert_array_equal(I.apply_transpose("u", meth, V), X)


def test_dirichlet_rows_contribute_nothing():
    """IDW on a mesh without Neumann flags: the boundary nodes are Dirichlet, their rows empty -- v on them alone gives exactly 0."""
    mesh = M.mixed_mesh(8, 4, 4, jitter=0.1, seed=1)
    M.attach_fields(mesh, "u", perm="ALH")
    I = _loaded(mesh)
    bp = np.asarray(I.grid.boundary_points) != 0
    assert 0 < bp.sum() < len(bp)
    rng = np.random.default_rng(7)
    x = I.apply_transpose("u", "idw", np.where(bp, rng.uniform(1.0, 2.0, len(bp)), 0.0))
    assert np.all(x == 0.0)
    assert np.count_nonzero(I.apply_transpose("u", "idw", np.where(bp, 0.0, 1.0))) > 0


@pytest.mark.parametrize("meth", METHODS)
def test_device_plan_spmv(C, meth, monkeypatch):
    """launch_spmv on the weights of plan.launch(add_neumann=True) is apply() bit for bit (GLS: the unfused apply), and
    launch_spmv_transpose is apply_transpose() bit for bit."""
    torch = _torch()
    if meth == "gls":
        monkeypatch.setenv("NIN_APPLY_NO_FUSION", "1")
    I, P, E = C["I"], C["P"], C["E"]
    dp = I.device_plan("u", meth)
    st = torch.cuda.current_stream().cuda_stream
    w = torch.empty(dp.nnz, dtype=torch.float64, device="cuda")
    nws = torch.empty(P, dtype=torch.float64, device="cuda")
    dp.launch(w.data_ptr(), nws.data_ptr(), st, add_neumann=True)
    rng = np.random.default_rng(9)
    U, V = rng.uniform(-1.0, 1.0, (3, E)), rng.uniform(-1.0, 1.0, (3, P))
    for k in (1, 3):
        u_np, v_np = (U[0], V[0]) if k == 1 else (U, V)
        u, v = torch.from_numpy(u_np).cuda(), torch.from_numpy(v_np).cuda()
        out = torch.empty((k, P) if k > 1 else (P,), dtype=torch.float64, device="cuda")
        x = torch.empty((k, E) if k > 1 else (E,), dtype=torch.float64, device="cuda")
        dp.launch_spmv(w.data_ptr(), u.data_ptr(), k, out.data_ptr(), st)
        dp.launch_spmv_transpose(w.data_ptr(), v.data_ptr(), k, x.data_ptr(), st)
        torch.cuda.synchronize()
        ref, ref_nws = I.apply("u", meth, values=u_np)
        np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"{meth} k={k} forward")
        np.testing.assert_array_equal(nws.cpu().numpy(), ref_nws)
        np.testing.assert_array_equal(x.cpu().numpy(), I.apply_transpose("u", meth, v_np), err_msg=f"{meth} k={k} transpose")


@pytest.mark.parametrize("meth", METHODS)
def test_cell_to_node_gradcheck(small, meth):
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    I = _loaded(small)
    E = I.grid.n_elems
    assert 60 <= E <= 200, E
    op = CellToNode(I, "u", meth)
    assert op.weights.dtype == torch.float64 and tuple(op.weights.shape) == (I.grid.nnz_esup,)
    assert tuple(op.neumann_ws.shape) == (I.grid.n_points,)
    gen = torch.Generator(device="cuda").manual_seed(0)
    u = torch.rand(E, dtype=torch.float64, device="cuda", generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(op, (u,))
    U = torch.rand(2, E, dtype=torch.float64, device="cuda", generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(op, (U,))


@pytest.mark.parametrize("meth", METHODS)
def test_cell_to_node_matches_apply(C, meth, monkeypatch):
    """forward = apply() bit for bit (GLS: the unfused apply); u.grad after (out * v).sum().backward() = apply_transpose(v) bit for
    bit, for one field and for three."""
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    if meth == "gls":
        monkeypatch.setenv("NIN_APPLY_NO_FUSION", "1")
    I, P, E = C["I"], C["P"], C["E"]
    op = CellToNode(I, "u", meth)
    rng = np.random.default_rng(13)
    for shape_u, shape_v in (((E,), (P,)), ((3, E), (3, P))):
        u_np, v_np = rng.uniform(-1.0, 1.0, shape_u), rng.uniform(-1.0, 1.0, shape_v)
        u = torch.from_numpy(u_np).cuda().requires_grad_(True)
        v = torch.from_numpy(v_np).cuda()
        out = op(u)
        ref, ref_nws = I.apply("u", meth, values=u_np)
        np.testing.assert_array_equal(out.detach().cpu().numpy(), ref, err_msg=f"{meth} {shape_u}")
        np.testing.assert_array_equal(op.neumann_ws.cpu().numpy(), ref_nws)
        (out * v).sum().backward()
        np.testing.assert_array_equal(u.grad.cpu().numpy(), I.apply_transpose("u", meth, v_np), err_msg=f"{meth} {shape_u} grad")


def test_cell_to_node_refresh(small, monkeypatch):
    """An in-place permeability edit is seen by refresh() and only there: before it the GLS outputs stay, after it they change and
    equal a new apply()."""
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    monkeypatch.setenv("NIN_APPLY_NO_FUSION", "1")
    I = _loaded(small)
    E = I.grid.n_elems
    op = CellToNode(I, "u", "gls")
    u_np = np.random.default_rng(17).uniform(0.5, 1.5, E)
    u = torch.from_numpy(u_np).cuda()
    before = op(u).cpu().numpy()
    K = I.cells_data[I.variable_to_index["cells"]["permeability"]]
    K[:9 * (E // 2)] *= 3.0            # the first half of the cells, in place
    np.testing.assert_array_equal(op(u).cpu().numpy(), before)
    op.refresh()
    after = op(u).cpu().numpy()
    assert not np.array_equal(after, before)
    ref, _ = I.apply("u", "gls", values=u_np)
    np.testing.assert_array_equal(after, ref)


def test_cell_to_node_rejects_wrong_inputs(small):
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    I = _loaded(small)
    E = I.grid.n_elems
    op = CellToNode(I, "u", "idw")
    with pytest.raises(TypeError):
        op(torch.zeros(E, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        op(np.zeros(E))
    with pytest.raises(ValueError):
        op(torch.zeros(E, dtype=torch.float64))                         # on the CPU
    for shape in ((E + 1,), (2, E - 1), (0, E), (2, 2, E), (I.grid.n_points,)):
        with pytest.raises(ValueError):
            op(torch.zeros(shape, dtype=torch.float64, device="cuda"))
