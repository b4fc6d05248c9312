"""Moving meshes on the device: Interpolator.update_points on grids that hold device arrays (csrc/grid_update.hip).  The yardstick
throughout is a FRESH Interpolator loaded with the moved mesh; comparisons are bit for bit (np.array_equal, NaN patterns equal).
The mesh is the hybrid of every GLS kernel family with a Neumann plane (the parts of tests/test_gpu_transpose.py, rebuilt here)."""
import copy

import numpy as np
import pytest

import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

METHODS = ("gls", "idw", "ls")
GEOMETRY = ("point_coords", "centroids", "faces_centers", "normal_faces", "faces_areas")


def _parts():
    return [M.hex_mesh(16, jitter=0.1, seed=1), M.delaunay_tet_mesh(10, seed=4, lattice="random"), M.delaunay_tet_mesh(8, seed=2),
            M.tet_mesh(6, jitter=0.1, seed=3), M.wedge_mesh(6, 5, 4, jitter=0.05, seed=5), M.mixed_mesh(10, 5, 5, jitter=0.1, seed=6),
            M.delaunay_wedge_mesh(12, 6, seed=7, lattice="random"), M.wedge_fan(30, 3), M.wedge_fan(50, 2)]


def moved(points):
    """a smooth map: a mild shear plus small sine terms; cells keep their orientation whatever their size"""
    X = np.asarray(points, dtype=np.float64)
    Y = X.copy()
    Y[:, 0] += 0.05 * X[:, 1] + 0.01 * np.sin(2.0 * np.pi * X[:, 1])
    Y[:, 1] += 0.03 * X[:, 0] + 0.01 * np.sin(2.0 * np.pi * X[:, 0])
    if X.shape[1] > 2:
        Y[:, 2] += X[:, 2] * (0.04 * X[:, 0] + 0.01 * np.sin(2.0 * np.pi * X[:, 1]))
    return np.ascontiguousarray(Y)


def with_points(mesh, X):
    m = copy.copy(mesh)
    m.points = np.ascontiguousarray(X)
    return m


def _loaded(mesh, grid_build="host"):
    import ninpol_amd
    I = ninpol_amd.Interpolator(grid_build=grid_build)
    I.load_mesh(mesh_obj=mesh)
    return I


def _torch():
    import torch
    return torch


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_csr_same(got, ref, what):
    (W, nws), (Wr, nwsr) = got, ref
    assert W.shape == Wr.shape, what
    assert same(W.indptr, Wr.indptr) and same(W.indices, Wr.indices), (what, "pattern")
    assert same(W.data, Wr.data), (what, "data")
    assert same(nws, nwsr), (what, "neumann_ws")


def assert_grid_same(g, ref, what, names=util.GRID_ARRAYS):
    for k in names:
        assert same(getattr(g, k), getattr(ref, k)), (what, k)
    for k in util.GRID_SCALARS:
        assert int(getattr(g, k)) == int(getattr(ref, k)), (what, k)


@pytest.fixture(scope="module")
def C():
    parts = _parts()
    for i, p in enumerate(parts):
        M.attach_fields(p, "u", perm="ALH", neumann_plane=(2, 0.0), seed=20 + i)
    mesh = M.composite_mesh(parts)
    X0 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64))
    X1 = moved(X0)
    mesh1 = with_points(mesh, X1)
    F = _loaded(mesh1)
    P, E = int(F.grid.n_points), int(F.grid.n_elems)
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-1.0, 1.0, (2, E)), rng.uniform(-1.0, 1.0, (2, P))
    targets = np.sort(rng.choice(P, size=P // 7, replace=False)).astype(np.int64)
    fresh = {"W": {m: F.interpolate("u", m) for m in METHODS},
             "Wt": {m: F.interpolate("u", m, target_points=targets) for m in METHODS},
             "apply": {m: F.apply("u", m, values=u) for m in METHODS},
             "applyT": {m: F.apply_transpose("u", m, v) for m in METHODS}}
    return {"mesh": mesh, "mesh1": mesh1, "X0": X0, "X1": X1, "F": F, "fresh": fresh, "u": u, "v": v, "targets": targets, "P": P, "E": E}


def test_the_mesh_covers_every_kernel_and_really_moves(C):
    plan = C["F"].grid.gls_plan()
    for k in ("hex8", "mfg_tiles", "scratch", "quad4", "mfx_boundary"):
        assert plan[k] > 0, (k, plan)
    for fam in ("mfw_", "small", "block", "mfx_"):
        assert any(n > 0 for k, n in plan.items() if k.startswith(fam)), (fam, plan)
    assert np.count_nonzero(C["fresh"]["W"]["gls"][1]) > 0
    I0 = _loaded(C["mesh"])
    for k in GEOMETRY:
        assert not same(getattr(I0.grid, k), getattr(C["F"].grid, k)), k
    W0 = I0.interpolate("u", "gls")[0]
    assert not same(W0.data, C["fresh"]["W"]["gls"][0].data)


@pytest.mark.parametrize("when", ("before_upload", "after_upload"))
@pytest.mark.parametrize("grid_build", ("host", "device"))
def test_geometry_and_weights_equal_a_fresh_load(C, grid_build, when):
    I = _loaded(C["mesh"], grid_build)
    if when == "after_upload":
        I.interpolate("u", "idw")
        assert I.grid.device >= 0
        np.asarray(I.grid.centroids)            # a host copy of the old geometry exists and must not survive the update
    else:
        assert I.grid.device == -1
    plan_before = I.grid.gls_plan() if when == "after_upload" else None
    I.update_points(C["X1"])
    # host-built and never uploaded: the host builder's code; every other grid holds device arrays: the kernels
    assert I.grid.geometry_updates == (0 if (grid_build, when) == ("host", "before_upload") else 1)
    assert_grid_same(I.grid, C["F"].grid, (grid_build, when))
    for meth in METHODS:
        assert_csr_same(I.interpolate("u", meth), C["fresh"]["W"][meth], (grid_build, when, meth))
    if plan_before is not None:
        assert dict(I.grid.gls_plan()) == dict(plan_before)
    assert dict(I.grid.gls_plan()) == dict(C["F"].grid.gls_plan())
    np.testing.assert_array_equal(I.points_coords, C["X1"])


def test_results_after_an_update(C, oracle_lib):
    """interpolate (all nodes and a subset), apply and apply_transpose after update_points, against the fresh Interpolator bit for
    bit; the GLS plan and the transpose index stay; GLS also against the oracle on the moved mesh, within the suite's bars"""
    I = _loaded(C["mesh"])
    for meth in METHODS:                         # everything resident first: fields, plan, scratch, transpose index
        I.interpolate("u", meth)
    I.apply_transpose("u", "idw", C["v"])
    assert I.grid.has_transpose_index
    plan = dict(I.grid.gls_plan())
    I.update_points(C["X1"])
    assert I.grid.geometry_updates == 1
    assert I.grid.has_transpose_index            # not rebuilt: still the index made before the update
    assert dict(I.grid.gls_plan()) == plan
    fresh = C["fresh"]
    for meth in METHODS:
        assert same(I.apply_transpose("u", meth, C["v"]), fresh["applyT"][meth]), meth
        got, ref = I.apply("u", meth, values=C["u"]), fresh["apply"][meth]
        assert same(got[0], ref[0]) and same(got[1], ref[1]), meth
        assert_csr_same(I.interpolate("u", meth), fresh["W"][meth], meth)
        assert_csr_same(I.interpolate("u", meth, target_points=C["targets"]), fresh["Wt"][meth], (meth, "subset"))
    assert I.grid.has_transpose_index and dict(I.grid.gls_plan()) == plan
    o = oracle_lib.OracleInterpolator("port", threads=8)
    o.load_mesh(C["mesh1"])
    Wo, nwo = o.interpolate("u", "gls")
    W, nws = I.interpolate("u", "gls")
    err = util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data)
    el = util.csr_elementwise_err(W, Wo.indptr, Wo.indices, Wo.data)
    print(f"GLS after update_points vs oracle on the moved mesh: row-scaled {err:.3e}, element-wise {el:.3e}")
    assert err <= util.WEIGHT_RTOL
    assert el <= util.elementwise_rtol("gls")
    assert util.rowscaled_err(nws, nwo) <= util.WEIGHT_RTOL


def test_there_and_back(C):
    I = _loaded(C["mesh"], "device")
    W0 = {m: I.interpolate("u", m) for m in METHODS}
    g0 = {k: np.array(getattr(I.grid, k)) for k in util.GRID_ARRAYS}
    I.update_points(C["X1"])
    I.update_points(C["X0"])
    assert I.grid.geometry_updates == 2
    for k in util.GRID_ARRAYS:
        assert same(getattr(I.grid, k), g0[k]), k
    for m in METHODS:
        assert_csr_same(I.interpolate("u", m), W0[m], m)


@pytest.mark.parametrize("grid_build", ("host", "device"))
def test_release_scratch_between_two_updates(C, grid_build):
    I = _loaded(C["mesh"], grid_build)
    I.interpolate("u", "gls")
    I.update_points(C["X0"] + 0.5 * (C["X1"] - C["X0"]))
    I.release_scratch()
    np.asarray(I.grid.inpoel)                     # (a device-built grid: its mirror goes on fetching after the release)
    I.update_points(C["X1"])
    assert I.grid.geometry_updates == 2
    assert_grid_same(I.grid, C["F"].grid, grid_build)
    I.release_scratch()
    assert_grid_same(I.grid, C["F"].grid, grid_build, GEOMETRY)
    for meth in METHODS:
        assert_csr_same(I.interpolate("u", meth), C["fresh"]["W"][meth], (grid_build, meth))


@pytest.mark.parametrize("meth", METHODS)
def test_device_pointer_path_on_a_side_stream(C, meth):
    """a torch tensor on a non-default stream, then DevicePlan.launch on the same stream: equal to the host-pointer path"""
    torch = _torch()
    from ninpol_amd.interpolator import DevicePlan
    H = _loaded(C["mesh"])
    H.update_points(C["X1"])
    ph = DevicePlan(H, "u", meth)
    wh = torch.empty(ph.nnz, dtype=torch.float64, device="cuda")
    nh = torch.empty(ph.n_points, dtype=torch.float64, device="cuda")
    ph.launch(wh.data_ptr(), nh.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    I = _loaded(C["mesh"])
    plan = DevicePlan(I, "u", meth)
    w = torch.full((plan.nnz,), -7.0, dtype=torch.float64, device="cuda")
    nws = torch.full((plan.n_points,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    x_host = torch.from_numpy(C["X1"])
    with torch.cuda.stream(s):
        x = x_host.to("cuda", non_blocking=False)
        I.update_points(x)
        plan.launch(w.data_ptr(), nws.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert I.grid.geometry_updates == 1
    assert same(w.cpu().numpy(), wh.cpu().numpy()), meth
    assert same(nws.cpu().numpy(), nh.cpu().numpy()), meth
    assert_grid_same(I.grid, C["F"].grid, "device pointer", GEOMETRY)
    np.testing.assert_array_equal(I.points_coords, C["X1"])      # read back from the grid on first use
    assert_csr_same(I.interpolate("u", meth), C["fresh"]["W"][meth], meth)
    with pytest.raises(ValueError, match="shape"):
        I.update_points(x[:-1])
    with pytest.raises(ValueError, match="float64"):
        I.update_points(x.float())


@pytest.fixture(scope="module")
def small():
    mesh = M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    return mesh


@pytest.mark.parametrize("meth", METHODS)
def test_cell_to_node_follows_refresh_only(small, meth, monkeypatch):
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    monkeypatch.setenv("NIN_APPLY_NO_FUSION", "1")
    I = _loaded(small)
    E = I.grid.n_elems
    op = CellToNode(I, "u", meth)
    u = torch.from_numpy(np.random.default_rng(17).uniform(0.5, 1.5, E)).cuda()
    before = op(u).cpu().numpy()
    X1 = moved(small.points)
    I.update_points(torch.from_numpy(X1).cuda())
    assert same(op(u).cpu().numpy(), before)          # nothing refreshes behind the caller's back
    op.refresh()
    after = op(u).cpu().numpy()
    assert not same(after, before)
    fresh_op = CellToNode(_loaded(with_points(small, X1)), "u", meth)
    assert same(after, fresh_op(u).cpu().numpy())
    assert same(op.weights.cpu().numpy(), fresh_op.weights.cpu().numpy())
    gen = torch.Generator(device="cuda").manual_seed(0)
    ug = torch.rand(E, dtype=torch.float64, device="cuda", generator=gen, requires_grad=True)
    assert torch.autograd.gradcheck(op, (ug,))


@pytest.mark.parametrize("columns", (3, 2))
@pytest.mark.parametrize("grid_build", ("host", "device"))
def test_two_dimensional_mesh(grid_build, columns):
    """grid arrays, IDW and LS bit-identical to a fresh load (2-D GLS is unpinned, DESIGN section 7: not asserted)"""
    mesh = M.quad_tri_mesh_2d(12, jitter=0.1, seed=2)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(0, 0.0), seed=2)
    mesh = with_points(mesh, np.asarray(mesh.points)[:, :columns])
    X1 = moved(mesh.points)
    F = _loaded(with_points(mesh, X1))
    I = _loaded(mesh, grid_build)
    I.interpolate("u", "idw")
    I.update_points(X1)
    assert I.grid.geometry_updates == 1
    assert_grid_same(I.grid, F.grid, (grid_build, columns))
    assert I.grid.point_coords.shape == (mesh.points.shape[0], columns)
    for meth in ("idw", "ls"):
        assert_csr_same(I.interpolate("u", meth), F.interpolate("u", meth), (grid_build, columns, meth))
