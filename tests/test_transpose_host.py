"""CPU-side tests of the adjoint entry points (no GPU needed): nin_spmv_device, nin_spmv_transpose_device and
nin_apply_transpose_fields_host refuse a host-only grid and bad arguments with the documented codes, and
Interpolator.apply_transpose validates its arguments before it touches a device."""
import ctypes

import numpy as np
import pytest

from ninpol_amd import mesh as M

IDW = 1   # NIN_METHOD_IDW


@pytest.fixture(scope="module")
def lib():
    from ninpol_amd import build as nbuild
    nbuild.build()
    from ninpol_amd import _lib
    return _lib


@pytest.fixture
def host_interp(lib):
    """an Interpolator whose grid was built on the host and never uploaded"""
    import ninpol_amd
    mesh = M.hex_mesh(3)
    M.attach_fields(mesh, "u", neumann_plane=(2, 0.0))
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    assert I.grid.device == -1
    return I


def _buffers(I, k=1):
    g = I.grid
    return (np.zeros(g.nnz_esup), np.zeros(k * g.n_elems), np.zeros(k * g.n_points))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _calls(L, g, w, cells, nodes, k):
    """the three entry points with the given arguments (None = NULL)"""
    p = lambda a: None if a is None else _p(a)
    return {
        "nin_spmv_device": lambda: L.nin_spmv_device(g, p(w), p(cells), k, p(nodes), None),
        "nin_spmv_transpose_device": lambda: L.nin_spmv_transpose_device(g, p(w), p(nodes), k, p(cells), None),
        "nin_apply_transpose_fields_host": lambda: L.nin_apply_transpose_fields_host(g, IDW, p(nodes), k, p(cells)),
    }


def _assert_code(L, rc, code, what):
    assert rc == code, (what, rc)
    assert L.nin_last_error().decode().strip(), (what, "no error text")


def test_host_only_grid_is_enodevice(lib, host_interp):
    L = lib.load()
    w, cells, nodes = _buffers(host_interp)
    for name, call in _calls(L, host_interp.grid._h, w, cells, nodes, 1).items():
        _assert_code(L, call(), lib.NIN_ENODEVICE, name)


@pytest.mark.parametrize("which", ["grid", "weights", "nodes", "cells"])
def test_null_arguments_are_einval(lib, host_interp, which):
    L = lib.load()
    w, cells, nodes = _buffers(host_interp)
    g = host_interp.grid._h
    if which == "grid":
        g = None
    elif which == "weights":
        w = None
    elif which == "nodes":
        nodes = None
    else:
        cells = None
    for name, call in _calls(L, g, w, cells, nodes, 1).items():
        if which == "weights" and name == "nin_apply_transpose_fields_host":
            continue   # (computes its own weights: no weight pointer)
        _assert_code(L, call(), lib.NIN_EINVAL, (name, which))


@pytest.mark.parametrize("k", [0, -2])
def test_no_fields_is_einval(lib, host_interp, k):
    L = lib.load()
    w, cells, nodes = _buffers(host_interp)
    for name, call in _calls(L, host_interp.grid._h, w, cells, nodes, k).items():
        _assert_code(L, call(), lib.NIN_EINVAL, (name, k))


def test_apply_transpose_validates_before_the_device(lib, host_interp):
    """Wrong shape, unknown method, unknown variable: ValueError, and the grid stays on the host (on a machine without a GPU a
    device call would raise NinpolError(NIN_ENODEVICE) instead)."""
    I = host_interp
    P, E = I.grid.n_points, I.grid.n_elems
    bad = [("u", "idw", np.zeros(E)),                  # cell-sized, not node-sized
           ("u", "idw", np.zeros((2, P + 1))),
           ("u", "idw", np.zeros((0, P))),
           ("u", "idw", np.zeros((2, 2, P))),
           ("u", "kriging", np.zeros(P)),
           ("nope", "gls", np.zeros(P))]
    for variable, method, values in bad:
        with pytest.raises(ValueError):
            I.apply_transpose(variable, method, values)
        assert I.grid.device == -1, (variable, method, np.shape(values))


def test_apply_transpose_needs_a_mesh(lib):
    import ninpol_amd
    with pytest.raises(ValueError, match="Grid not initialized"):
        ninpol_amd.Interpolator().apply_transpose("u", "idw", np.zeros(3))


def test_device_plan_has_the_spmv_wrappers():
    from ninpol_amd.interpolator import DevicePlan
    assert callable(DevicePlan.launch_spmv) and callable(DevicePlan.launch_spmv_transpose)
