"""Twins for tests/test_gpu_device_grid_features.py and tests/test_gpu_device_grid_derivatives.py: one mesh loaded into two
Interpolators, grid_build="host" and grid_build="device", driven through the same calls with the same inputs and compared by bytes.

Both builders produce identical arrays (tests/test_gpu_grid_device.py) and every kernel is deterministic, so whatever the host-built
twin returns -- which the feature's own tests hold to the 80-bit models, the oracle and fresh loads -- the device-built twin must return
bit for bit.  What differs is the residency code behind the device-built grid: its host arrays come over on first use
(HostGrid::have, DeviceMirror::fetch), nin_grid_to_device adopts its device arrays, and the first call that needs inpoel / etype / inpofa /
faces_areas on the device borrows them from the mirror (ensure_update_inputs -> lend_geometry_inputs).  Which of those branches a call
takes depends on the STATE of the mirror when it runs; `enter` below reaches each state by construction (they cannot be observed from
Python)."""
import numpy as np

import test_gpu_grid_device as GD
import test_gpu_update_points as UP

ARRAYS, SCALARS = GD.ARRAYS, GD.SCALARS
GEOMETRY = UP.GEOMETRY

# The state of the device-built twin's host mirror before the operation under test:
#   cold           nothing was read from I.grid on the host beyond what load_mesh() and the first interpolate() read themselves: the
#                  first ensure_update_inputs borrows the four arrays from the mirror
#   partial        point_coords, inpofa and faces_areas were read: the mirror is alive, three bits of `have` are set, and a geometry update
#                  must clear the two that are geometry
#   full           every array was read: have == A_ALL, the mirror is gone (it freed the buffers it owned) and ensure_update_inputs
#                  uploads from the host arrays, as on a host-built grid
#   lent_released  one whole-mesh update_points() (which borrows the four arrays), then release_scratch(): the borrowed buffers stay
#                  while the mirror still reads them
#   pre_adoption   nothing at all, not even the first interpolate(): the grid holds device arrays but is not yet "on the device"
#                  (the caller moves nodes from host arrays first: nin_grid_scatter_points' branch for such a grid)
#   re_uploaded    Grid.to_device() twice before any field is resident: the second call does not adopt -- everything comes to the
#                  host, the device copy is freed and uploaded again
STATES = ("cold", "partial", "full", "lent_released", "pre_adoption", "re_uploaded")
PARTIAL = ("point_coords", "inpofa", "faces_areas")


def _torch():
    import torch
    return torch


def load(mesh, grid_build, **kw):
    import ninpol_amd
    I = ninpol_amd.Interpolator(grid_build=grid_build, **kw)
    I.load_mesh(mesh_obj=mesh)
    return I


def twins(mesh, **kw):
    """(host-built, device-built) Interpolators of one mesh"""
    return load(mesh, "host", **kw), load(mesh, "device", **kw)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def enter(H, D, state, variable="u"):
    """bring the device-built twin D to `state`; the host-built twin H makes the same calls"""
    assert state in STATES, state
    torch = _torch()
    if state == "pre_adoption":
        assert H.grid.device < 0 and D.grid.device < 0
        return
    if state == "re_uploaded":
        for I in (H, D):
            I.grid.to_device(I.device)
            I.grid.to_device(I.device)
            assert I.grid.device == I.device
        return
    for I in (H, D):
        I.interpolate(variable, "idw")
    if state == "partial":
        for k in PARTIAL:
            assert same(getattr(H.grid, k), getattr(D.grid, k)), k
    elif state == "full":
        for k in ARRAYS:
            assert same(getattr(H.grid, k), getattr(D.grid, k)), k
    elif state == "lent_released":
        for I in (H, D):
            X = np.ascontiguousarray(np.asarray(I.points_coords, dtype=np.float64))
            I.update_points(torch.from_numpy(X).to(torch.device("cuda", I.device)))     # the same coordinates: the same mesh
            torch.cuda.synchronize()
            I.grid.release_scratch()
            assert I.grid.geometry_updates == 1


def assert_lazy_arrays_same(H, D, what, edges=False):
    """every host array and scalar of the device-built twin, read now, is the host-built twin's: where a stale `have` bit shows"""
    for k in SCALARS:
        assert int(getattr(H.grid, k)) == int(getattr(D.grid, k)), (what, k)
    for k in ARRAYS + (("inedel", "inpoed") if edges else ()):
        a, b = getattr(H.grid, k), getattr(D.grid, k)
        assert a.size > 0 and same(a, b), (what, k)
    if edges:
        assert H.grid.n_edges == D.grid.n_edges > 0, what


def assert_csr_same(got, ref, what):
    (W, nws), (Wr, nwsr) = got, ref
    assert W.shape == Wr.shape, what
    assert same(W.indptr, Wr.indptr) and same(W.indices, Wr.indices), (what, "pattern")
    assert same(W.data, Wr.data), (what, "data")
    assert same(nws, nwsr), (what, "neumann_ws")
