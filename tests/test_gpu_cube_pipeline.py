"""The cube-node kernel's pass pipeline (kernels_gls_hex8mf.hip): the index levels and the geometry of the NEXT pass are requested
during this one, the geometry into registers in the middle of phase 2, and the permeability of the cell across a face comes from
the lane that owns that cell.  Lists of 1, 15, 16, 17 nodes (less than one pass per wave, a ragged last group), more groups
than resident waves, a shuffled list; the weights and the fused apply; with and without the side stream; interpolate() in
pieces.  Each case against the oracle, and bit for bit against the same nodes of one full launch."""
import numpy as np
import pytest

import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

# resident waves of one full launch: 512 workgroups of 4 waves, 16 nodes a pass
_WAVES = 512 * 4


def _interp():
    import ninpol_amd
    return ninpol_amd.Interpolator(device=0)


def _setup(oracle_lib, dims, seed):
    mesh = M.hex_mesh(*dims, jitter=0.15, seed=seed)
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(1, 0.0), seed=seed + 1)
    o = oracle_lib.OracleInterpolator("port", threads=16)
    o.load_mesh(mesh)
    return mesh, o


def _cube_nodes(I):
    """The interior nodes of a hexahedron mesh: all of them cube nodes (the plan says so)."""
    interior = np.nonzero(np.asarray(I.grid.boundary_points) == 0)[0].astype(np.int64)
    assert I.grid.gls_plan()["hex8"] == len(interior)
    return interior


@pytest.mark.parametrize("side", [True, False])
def test_gpu_cube_pipeline_target_lists(oracle_lib, monkeypatch, side):
    """Target lists that give the cube-node kernel 1, 15, 16, 17 and 16 * 8 * waves + 1 nodes (more than one pass per wave
    on every XCD), and a shuffled list, with boundary nodes mixed in."""
    if not side:
        monkeypatch.setenv("NIN_GLS_NO_SIDE_STREAM", "1")
    mesh, o = _setup(oracle_lib, (36, 35, 34), 21)
    wo, no = o.prepare("gls", "u")
    I = _interp()
    I.load_mesh(mesh_obj=mesh)
    I.grid.to_device(0)
    cube = _cube_nodes(I)
    n_big = 16 * 8 * (_WAVES // 8) + 1
    assert len(cube) >= n_big
    w_all, nw_all = I.prepare_interpolator("gls", "u", np.arange(I.grid.n_points))
    assert util.rowscaled_err(w_all, wo) <= util.WEIGHT_RTOL
    assert util.rowscaled_err(nw_all, no) <= util.WEIGHT_RTOL
    assert np.count_nonzero(w_all[cube]) > 8 * len(cube) - 10
    rng = np.random.default_rng(3)
    boundary = np.nonzero(np.asarray(I.grid.boundary_points) != 0)[0].astype(np.int64)
    lists = {k: np.sort(rng.choice(cube, size=k, replace=False)) for k in (1, 15, 16, 17, n_big)}
    lists["shuffled"] = rng.permutation(np.concatenate([rng.choice(cube, size=4099, replace=False), boundary[:300]]))
    for name, tgt in lists.items():
        n_cube = np.count_nonzero(np.isin(tgt, cube))
        assert n_cube == (len(tgt) if name != "shuffled" else 4099), name
        ws, nws = I.prepare_interpolator("gls", "u", tgt)
        assert util.rowscaled_err(ws, wo[tgt]) <= util.WEIGHT_RTOL, name
        assert util.rowscaled_err(nws, no[tgt]) <= util.WEIGHT_RTOL, name
        assert np.array_equal(ws, w_all[tgt]) and np.array_equal(nws, nw_all[tgt]), name


@pytest.mark.parametrize("dims,n_cube", [((2, 2, 2), 1), ((4, 6, 2), 15), ((5, 5, 2), 16), ((18, 2, 2), 17)])
@pytest.mark.parametrize("side", [True, False])
def test_gpu_cube_pipeline_small_meshes(oracle_lib, monkeypatch, dims, n_cube, side):
    """Whole meshes with 1, 15, 16, 17 cube nodes: the full launch, interpolate(), and the fused apply."""
    if not side:
        monkeypatch.setenv("NIN_GLS_NO_SIDE_STREAM", "1")
    mesh, o = _setup(oracle_lib, dims, 5)
    wo, no = o.prepare("gls", "u")
    Wo, _ = o.interpolate("u", "gls")
    I = _interp()
    I.load_mesh(mesh_obj=mesh)
    I.grid.to_device(0)
    cube = _cube_nodes(I)
    assert len(cube) == n_cube
    w, nw = I.prepare_interpolator("gls", "u", np.arange(I.grid.n_points))
    assert util.rowscaled_err(w, wo) <= util.WEIGHT_RTOL
    assert util.rowscaled_err(nw, no) <= util.WEIGHT_RTOL
    W, _ = I.interpolate("u", "gls")
    assert util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data) <= util.WEIGHT_RTOL
    u = np.concatenate(mesh.cell_data["u"])
    vals, nws = I.apply("u", "gls")
    ref = Wo.dot(u)
    assert np.abs(vals - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())
    assert util.rowscaled_err(nws, no) <= util.WEIGHT_RTOL


def test_gpu_cube_pipeline_fused_apply_and_pieces(oracle_lib, monkeypatch):
    """A mesh with more cube groups than resident waves: the fused apply and interpolate() in pieces, with and without the side
    stream, each equal bit for bit to the other route's and within the suite's tolerance of the oracle."""
    mesh, o = _setup(oracle_lib, (41, 40, 37), 33)
    Wo, nwo = o.interpolate("u", "gls")
    u = np.concatenate(mesh.cell_data["u"])
    fields = np.stack([u, np.sin(3.0 * u)])
    got = {}
    for side in (True, False):
        if side:
            monkeypatch.delenv("NIN_GLS_NO_SIDE_STREAM", raising=False)
        else:
            monkeypatch.setenv("NIN_GLS_NO_SIDE_STREAM", "1")
        for pieces in (False, True):
            if pieces:
                monkeypatch.setenv("NIN_E2E_MIN_NODES", "1024")
            else:
                monkeypatch.delenv("NIN_E2E_MIN_NODES", raising=False)
            I = _interp()
            I.load_mesh(mesh_obj=mesh)
            W, neu = I.interpolate("u", "gls")
            assert I.grid.gls_plan()["hex8"] == 40 * 39 * 36 > 16 * _WAVES
            assert util.csr_rowscaled_err(W, Wo.indptr, Wo.indices, Wo.data) <= util.WEIGHT_RTOL
            many, nws = I.apply("u", "gls", values=fields)
            for k in range(2):
                ref = Wo.dot(fields[k])
                assert np.abs(many[k] - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (side, pieces, k)
            got[side, pieces] = (W.indptr.copy(), W.indices.copy(), W.data.copy(), neu, many, nws)
    for key in got:
        for a, b in zip(got[True, False], got[key]):
            assert np.array_equal(a, b), key
