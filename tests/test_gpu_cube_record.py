"""The cube-node kernel's gather records (csrc/hex8_desc.hpp): one 32-byte record per lane -- node, esup row start, the lane's two
cells, its three faces, the descriptor word -- written once per list entry when the launch plan is built (in list order) or, for a
target list and a dirty launch, on the fly.  The kernel reads nothing else of the connectivity, so what is asked here is that the
records name the right rows whatever the ids look like, that a pass of 16 nodes reads ITS 2 KiB block on every route that indexes the
records by list entry, and that the resident records stay right under every update that leaves the topology alone.

Each case against the oracle at the suite's bars (util.WEIGHT_RTOL), and bit for bit (np.array_equal) where stated."""
import numpy as np
import pytest

import util
import test_gpu_update_fields as UF
import test_gpu_update_local as UL
import test_update_points_local_host as LH
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

PLANE = (2, 0.0)
same, on_device, with_K, _loaded = UF.same, UF.on_device, UF.with_K, UF._loaded
ids_on_device, stream, _buffers, _host, verts_of = UL.ids_on_device, UL.stream, UL._buffers, UL._host, UL.verts_of
with_points, verts_around = LH.with_points, LH.verts_around
FULL = UL.FULL


def _oracle(oracle_lib, mesh):
    o = oracle_lib.OracleInterpolator("port", threads=8)
    o.load_mesh(mesh)
    return o


def _cube_nodes(I):
    """the nodes the plan gives to the cube-node kernel, from a launch of that kernel alone into NaN-filled buffers"""
    from ninpol_amd.interpolator import DevicePlan
    dp = DevicePlan(I, "u", "gls")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NIN_GLS_ONLY", str(list(I.grid.PLAN_KERNELS).index("hex8")))
        b = _buffers(dp, np.nan)
        dp.launch(b[0].data_ptr(), b[1].data_ptr(), stream())
        cube = np.flatnonzero(~np.isnan(_host(b)[1])).astype(np.int64)
    assert len(cube) == I.grid.gls_plan()["hex8"]
    return cube


def _full_list_oracle(oracle_lib, mesh, n_cube=None):
    """the full launch against the oracle, and the target-list route over all cube nodes (records built on the fly, list in node
    order, not the plan's) bit for bit against the same rows of the full launch"""
    o = _oracle(oracle_lib, mesh)
    wo, no = o.prepare("gls", "u")
    I = _loaded(mesh)
    w, nw = I.prepare_interpolator("gls", "u", np.arange(I.grid.n_points))
    rs = util.rowscaled_err(w, wo)
    print(f"full launch: row-scaled {rs:.2e} (bar {util.WEIGHT_RTOL:g})")
    assert rs <= util.WEIGHT_RTOL
    assert util.rowscaled_err(nw, no) <= util.WEIGHT_RTOL
    cube = _cube_nodes(I)
    if n_cube is not None:
        assert len(cube) == n_cube
    assert np.count_nonzero(w[cube]) == 8 * len(cube)
    ws, nws = I.prepare_interpolator("gls", "u", cube)
    assert np.array_equal(ws, w[cube]) and np.array_equal(nws, nw[cube])
    shuffled = np.random.default_rng(5).permutation(cube)
    ws, nws = I.prepare_interpolator("gls", "u", shuffled)
    assert np.array_equal(ws, w[shuffled]) and np.array_equal(nws, nw[shuffled])
    return I, o, cube


# ---- the XCD path at its smallest, and the fused apply on it -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def hex10():
    mesh = M.hex_mesh(10, jitter=0.15, seed=11)
    return M.attach_fields(mesh, "u", perm="ALH", neumann_plane=PLANE, seed=12)


def test_xcd_path_at_its_smallest(oracle_lib, hex10):
    """729 cube nodes are 12 workgroups of 64, launched as 8: one per XCD, each on its own eighth of the list and its own counter,
    a ragged last group (729 = 45 * 16 + 9) and waves whose first ticket is already past their eighth."""
    _full_list_oracle(oracle_lib, hex10, n_cube=729)


def test_fused_apply(oracle_lib, hex10):
    """The apply form of the kernel on the 10^3 mesh: values = W . u with W the weights form's matrix.  A node's value is a sum of
    8 products in another order than scipy's: |difference| <= 16 eps (|W| . |u|) row by row (8 roundings of the sum on either
    side), no more.  neumann_ws bit for bit."""
    I = _loaded(hex10)
    W, neu = I.interpolate("u", "gls")
    o = _oracle(oracle_lib, hex10)
    Wo, _ = o.interpolate("u", "gls")
    assert util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data) <= util.WEIGHT_RTOL
    u = np.concatenate(hex10.cell_data["u"])
    fields = np.stack([u, np.cos(5.0 * u), -u * u])
    vals, nws = I.apply("u", "gls", values=fields)
    assert I.grid.gls_plan()["hex8"] == 729
    eps = np.finfo(np.float64).eps
    for k in range(3):
        ref, bound = W.dot(fields[k]), 16 * eps * abs(W).dot(np.abs(fields[k]))
        worst = np.max(np.abs(vals[k] - ref) - bound)
        print(f"fused apply, field {k}: max |values - W u| {np.abs(vals[k] - ref).max():.2e}, worst margin to the bound {worst:.2e}")
        assert np.all(np.abs(vals[k] - ref) <= bound), k
    assert np.array_equal(np.asarray(nws), np.asarray(neu))


# ---- the record holds no geometry and no permeability --------------------------------------------------------------------------------
NX, NY, NZ = 6, 5, 4


def _node(i, j, k):
    return i + (NX + 1) * (j + (NY + 1) * k)


def _cell(i, j, k):
    return i + NX * (j + NY * k)


# (moved nodes, changed cells) by the number of cube nodes in the dirty set.  A moved node marks the vertices of the cells around it
# -- 3 x 3 x 3 nodes around an interior one, of which at least 2 x 2 x 2 are interior -- and a changed cell its own 8 vertices, of
# which 1 (a corner cell), 2 (an edge cell), 4 or 8 are interior.  So one cube node can only come from a corner: there the moved
# node is the mesh's corner itself.
EDITS = {
    1: ([(0, 0, 0)], [(0, 0, 0)]),
    15: ([(1, 1, 1), (2, 1, 1)], [(5, 4, 3), (5, 4, 1), (0, 0, 0)]),        # 3 x 2 x 2 = 12, + 1 + 2, + 0
    16: ([(1, 1, 1), (5, 4, 3)], [(0, 0, 0), (5, 4, 3)]),                    # 8 + 8, + 0
    17: ([(1, 1, 1), (5, 4, 3)], [(0, 0, 0), (5, 0, 0)]),                    # 8 + 8, + 0 + 1
}


@pytest.fixture(scope="module")
def hex654():
    mesh = M.attach_fields(M.hex_mesh(NX, NY, NZ, jitter=0.1, seed=3), "u", perm="LIN", neumann_plane=PLANE, seed=4)
    K1 = UF.K_of(mesh, "ALH", 9)
    return mesh, K1


@pytest.mark.parametrize("n_cube", sorted(EDITS))
def test_record_holds_no_geometry_and_no_permeability(oracle_lib, hex654, n_cube):
    """update_points(nodes=...) and update_permeability(cells=...) on a resident grid, then the dirty launch (records on the fly for
    n_cube cube nodes: 1, 15, 16, 17 -- less than a pass, a full one, a ragged second) and the full launch (the plan's records, as
    built before the edit): both equal a fresh load_mesh of the edited mesh bit for bit."""
    from ninpol_amd.interpolator import DevicePlan
    mesh, K1 = hex654
    I = _loaded(mesh)
    plan = DevicePlan(I, "u", "gls")
    g = I.grid
    interior = np.flatnonzero(np.asarray(g.boundary_points) == 0)
    assert g.gls_plan()["hex8"] == len(interior) == (NX - 1) * (NY - 1) * (NZ - 1)
    dirty_buf = _buffers(plan, FULL)
    plan.launch(dirty_buf[0].data_ptr(), dirty_buf[1].data_ptr(), stream())
    before = _host(dirty_buf)
    g.clear_dirty(stream())

    nodes = np.array([_node(*t) for t in EDITS[n_cube][0]], dtype=np.int64)
    cells = np.array([_cell(*t) for t in EDITS[n_cube][1]], dtype=np.int64)
    X1 = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64)).copy()
    X1[nodes] += 0.01 * np.random.default_rng(n_cube).uniform(-1.0, 1.0, (len(nodes), 3))      # (a cell is 0.17 .. 0.25 wide)
    K_now = np.ascontiguousarray(np.concatenate(mesh.cell_data["permeability"])).copy()
    K_now[cells] = K1[cells]
    I.update_points(on_device(X1[nodes]), nodes=ids_on_device(nodes))
    I.update_permeability(on_device(K1[cells]), cells=ids_on_device(cells))
    inpoel, esup, esup_ptr = np.array(g.inpoel), np.array(g.esup), np.array(g.esup_ptr)
    dirty = np.union1d(verts_around(inpoel, esup, esup_ptr, nodes), verts_of(inpoel, cells))
    assert np.count_nonzero(np.isin(dirty, interior)) == n_cube
    assert g.dirty_nodes == len(dirty)

    edited = with_points(with_K(mesh, K_now), X1)
    F = DevicePlan(_loaded(edited), "u", "gls")
    fresh = _buffers(F, FULL)
    F.launch(fresh[0].data_ptr(), fresh[1].data_ptr(), stream())
    fw, fn = _host(fresh)
    assert not same(fw, before[0]), "the edit changed nothing"

    assert plan.launch_dirty(dirty_buf[0].data_ptr(), dirty_buf[1].data_ptr(), stream(), clear=False) == len(dirty)
    w, nws = _host(dirty_buf)
    assert same(w, fw) and same(nws, fn), "dirty launch"
    full = _buffers(plan, FULL)
    plan.launch(full[0].data_ptr(), full[1].data_ptr(), stream())
    w, nws = _host(full)
    assert same(w, fw) and same(nws, fn), "full launch on the records built before the edit"

    o = _oracle(oracle_lib, edited)
    wo, no = o.prepare("gls", "u")
    wd, nwd = I.prepare_interpolator("gls", "u", np.arange(g.n_points))
    assert util.rowscaled_err(wd, wo) <= util.WEIGHT_RTOL and util.rowscaled_err(nwd, no) <= util.WEIGHT_RTOL


# ---- ids from all over the tables; rows that start anywhere ---------------------------------------------------------------------------
def test_relabelled_mesh_at_17_cube_nodes(oracle_lib):
    """Node, cell and vertex order permuted (mesh.relabel_mesh, as tests/test_gpu_relabel.py takes it): every record of the 17 -- one
    full pass and one node -- holds ids from all over the tables and a descriptor word of its own."""
    mesh = M.attach_fields(M.hex_mesh(18, 2, 2, jitter=0.15, seed=5), "u", perm="ALH", neumann_plane=PLANE, seed=6)
    r = M.relabel_mesh(mesh, seed=21)
    I, _, cube = _full_list_oracle(oracle_lib, r, n_cube=17)
    assert np.any(np.diff(cube) > 1)


def test_esup_rows_that_start_anywhere(oracle_lib):
    """Hexahedra beside pyramids and tetrahedra: the rows in front of a cube node's are of every length, so its esup row does not
    start on a multiple of 8 (on a hexahedron mesh in generator order many do)."""
    mesh = M.attach_fields(M.mixed_mesh(8, 4, 4, jitter=0.1, seed=3), "u", perm="ALH", neumann_plane=PLANE, seed=4)
    I, _, cube = _full_list_oracle(oracle_lib, mesh)
    starts = np.asarray(I.grid.esup_ptr)[cube]
    assert len(cube) >= 17 and np.count_nonzero(starts % 8) > 0 and len(set((starts % 8).tolist())) > 2
