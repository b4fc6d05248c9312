"""The cube-node kernel's leaner phase 1 (kernels_gls_hex8mf.hip, round 12): a column never forms its rows 0 .. 2, u comes from
q = V_top^T z -- the same mathematics in another summation order, so u changes by rounding.  (The face rows' sign as sign-bit flips
and phase-2 quad sums two columns at a time were measured with the same cases and dropped: DESIGN 4.3.)  Small jittered hexahedron
meshes whose interior nodes are all cube nodes: 27 of them (one full group of 16 and a partial one) and 60 (several passes in a
wave), the second with a Neumann plane AND flagged interior nodes, so that the kernel's own is_neu / add_neumann branch runs; both
values of a face row's side bit occur at every node; the ALH and the FAN permeability; the weights and the fused apply.  Each
against the oracle at the suite's bars for hexahedron cases (util.py)."""
import numpy as np
import pytest

import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

CASES = {"4x4x4": ((4, 4, 4), 27, None), "6x5x4": ((6, 5, 4), 60, (2, 0.0))}


def _interp():
    import ninpol_amd
    return ninpol_amd.Interpolator(device=0)


def _mesh(dims, perm, plane):
    mesh = M.hex_mesh(*dims, jitter=0.15, seed=11)
    M.attach_fields(mesh, "u", perm=perm, neumann_plane=plane, seed=12)
    if plane is not None:
        # every other interior node carries the flag too: boundary nodes never reach the cube-node kernel
        nx, ny, nz = dims
        i, j, k = np.meshgrid(np.arange(1, nx), np.arange(1, ny), np.arange(1, nz), indexing="ij")
        inner = (i + j * (nx + 1) + k * (nx + 1) * (ny + 1)).ravel()
        mesh.point_data["neumann_flag_u"][inner[::2]] = 1.0
    return mesh


def _side_bits(grid, p):
    """The side bits of the 12 face rows of cube node p: is the face's EVEN cell (the colour class of the esup row's first cell,
    hex8_desc.hpp) its first cell?"""
    esup, eptr, fsup, fptr = (np.asarray(getattr(grid, k)) for k in ("esup", "esup_ptr", "fsup", "fsup_ptr"))
    esuf, sptr = np.asarray(grid.esuf), np.asarray(grid.esuf_ptr)
    cells = [int(c) for c in esup[eptr[p]:eptr[p + 1]]]
    pairs = [(int(esuf[sptr[f]]), int(esuf[sptr[f] + 1])) for f in fsup[fptr[p]:fptr[p + 1]]]
    colour = {cells[0]: 0}
    for _ in range(4):
        for a, b in pairs:
            if a in colour and b not in colour:
                colour[b] = 1 - colour[a]
            if b in colour and a not in colour:
                colour[a] = 1 - colour[b]
    assert sorted(colour) == sorted(cells) and all(colour[a] != colour[b] for a, b in pairs)
    return {colour[a] == 0 for a, _ in pairs}


_CACHE = {}


def _case(oracle_lib, name, perm):
    """mesh, oracle results and a loaded Interpolator, once per (mesh, permeability); nothing in it is written to afterwards"""
    if (name, perm) not in _CACHE:
        dims, n_cube, plane = CASES[name]
        mesh = _mesh(dims, perm, plane)
        o = oracle_lib.OracleInterpolator("port", threads=16)
        o.load_mesh(mesh)
        wo, no = o.prepare("gls", "u")
        Wo, _ = o.interpolate("u", "gls")
        I = _interp()
        I.load_mesh(mesh_obj=mesh)
        I.grid.to_device(0)
        cube = np.nonzero(np.asarray(I.grid.boundary_points) == 0)[0].astype(np.int64)
        assert I.grid.gls_plan()["hex8"] == len(cube) == n_cube
        _CACHE[name, perm] = dict(name=name, perm=perm, mesh=mesh, I=I, cube=cube, wo=wo, no=no, Wo=Wo, plane=plane)
    return _CACHE[name, perm]


@pytest.mark.parametrize("perm", ["ALH", "FAN"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_cube_diet_weights(oracle_lib, name, perm):
    """The weights and neumann_ws of every node, the cube nodes' on their own, and both side bits at every cube node."""
    case = _case(oracle_lib, name, perm)
    I, cube, wo, no = case["I"], case["cube"], case["wo"], case["no"]
    for p in cube:
        assert _side_bits(I.grid, int(p)) == {True, False}, int(p)
    w, nw = I.prepare_interpolator("gls", "u", np.arange(I.grid.n_points))
    e_w, e_n = util.rowscaled_err(w[cube], wo[cube]), util.rowscaled_err(nw[cube], no[cube])
    e_el = util.elementwise_err(w[cube], wo[cube])
    print(f"cube diet {case['name']} {case['perm']}: weights {e_w:.3e}, neumann_ws {e_n:.3e} (bound {util.WEIGHT_RTOL:.1e}), "
          f"element-wise {e_el:.3e} (bound {util.elementwise_rtol('gls', case['perm']):.1e})")
    assert np.count_nonzero(w[cube]) == 8 * len(cube)
    assert e_w <= util.WEIGHT_RTOL and e_n <= util.WEIGHT_RTOL
    assert e_el <= util.elementwise_rtol("gls", case["perm"])
    assert util.rowscaled_err(w, wo) <= util.WEIGHT_RTOL and util.rowscaled_err(nw, no) <= util.WEIGHT_RTOL
    if case["plane"] is not None:
        assert np.count_nonzero(nw[cube]) == (len(cube) + 1) // 2       # the flagged interior nodes: the kernel's is_neu branch


@pytest.mark.parametrize("perm", ["ALH", "FAN"])
def test_gpu_cube_diet_apply(oracle_lib, perm):
    """The apply form of the kernel (DevicePlan.launch_apply, one field, the 6 x 5 x 4 mesh) against the oracle's W . u."""
    case = _case(oracle_lib, "6x5x4", perm)
    import torch
    from ninpol_amd.interpolator import DevicePlan
    I, Wo, no = case["I"], case["Wo"], case["no"]
    plan = DevicePlan(I, "u", "gls")
    u = np.concatenate(case["mesh"].cell_data["u"])
    u_d = torch.from_numpy(np.ascontiguousarray(u[None, :])).cuda()
    vals = torch.zeros((1, plan.n_points), dtype=torch.float64, device="cuda")
    nws = torch.zeros(plan.n_points, dtype=torch.float64, device="cuda")
    plan.launch_apply(u_d.data_ptr(), 1, vals.data_ptr(), nws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ref = Wo.dot(u)
    err = np.abs(vals.cpu().numpy()[0] - ref).max() / max(1.0, np.abs(ref).max())
    print(f"cube diet apply {case['perm']}: |W u - oracle| {err:.3e}")
    assert err <= util.WEIGHT_RTOL
    assert util.rowscaled_err(nws.cpu().numpy(), no) <= util.WEIGHT_RTOL
