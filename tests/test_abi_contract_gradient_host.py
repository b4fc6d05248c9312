"""The two entry points of the GLS corner gradients, without a device: the rows tests/test_abi_contract_host.py keeps for every
status-returning entry point -- a NULL grid, a host-only grid -- what the library declares, lists and builds for them, and every
refusal with its text: NULL pointers, n_fields < 1, a 2-D grid (answered before the grid's residency, so a host-only grid shows it),
a plan of IDW or LS."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import test_abi_contract_host as C
import test_update_fields_host as UH
from ninpol_amd import mesh as M

lib = UH.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (entry point, its arguments after the grid, tail of the text on a host-only grid): the form of test_abi_contract_host.TABLE
TABLE = (
    ("nin_gls_corner_gradients_device", (1, "buf", "buf", "buf", "buf", "buf", None), C.KERNELS),
    ("nin_gls_corner_gradients_host", ("buf", 1, "buf", "buf", "buf", "buf"), C.KERNELS),
)
NULL_ARGUMENT, N_FIELDS = "NULL argument", "n_fields must be >= 1"
TWO_D = "the corner gradients are for 3-D grids only (this grid is 2-D)"


@pytest.fixture(scope="module")
def host(lib):
    return C.Host(lib)


def test_declared_listed_and_built(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    L = lib.load()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name, _, _ in TABLE:
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in ninpol_amd.h"
        assert hasattr(L, name)
    assert list(L.nin_gls_corner_gradients_device.argtypes) == [vp, i32, vp, vp, vp, vp, vp, vp]
    assert list(L.nin_gls_corner_gradients_host.argtypes) == [vp, vp, i32, vp, vp, vp, vp]


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_null_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL and text == NULL_ARGUMENT, (name, rc, text)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_host_only_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, host.g, spec)
    assert rc == lib.NIN_ENODEVICE, (name, rc, text)
    assert text == C.NOT_ON_DEVICE + tail, (name, text)
    assert not host.buf.any()                                            # a refused call wrote nothing


def test_null_pointers_and_counts(lib, host):
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    text = lambda: L.nin_last_error().decode()                           # noqa: E731
    for call, want in ((lambda: L.nin_gls_corner_gradients_device(host.g, 1, None, b, b, b, b, None), NULL_ARGUMENT),
                       (lambda: L.nin_gls_corner_gradients_device(host.g, 1, b, None, b, b, b, None), NULL_ARGUMENT),
                       (lambda: L.nin_gls_corner_gradients_device(host.g, 0, b, b, None, None, None, None), N_FIELDS),
                       (lambda: L.nin_gls_corner_gradients_device(host.g, -1, b, b, b, b, b, None), N_FIELDS),
                       (lambda: L.nin_gls_corner_gradients_device(host.g, 0, None, b, b, b, b, None), NULL_ARGUMENT),        # NULL first
                       (lambda: L.nin_gls_corner_gradients_host(host.g, None, 1, b, b, b, b), NULL_ARGUMENT),
                       (lambda: L.nin_gls_corner_gradients_host(host.g, b, 1, None, b, b, b), NULL_ARGUMENT),
                       (lambda: L.nin_gls_corner_gradients_host(host.g, b, 0, b, None, None, None), N_FIELDS),
                       (lambda: L.nin_gls_corner_gradients_host(host.g, b, -3, b, b, b, b), N_FIELDS)):
        assert call() == lib.NIN_EINVAL
        assert text() == want
    # the three optional outputs may be NULL: the refusal is then the grid's, not theirs
    assert L.nin_gls_corner_gradients_device(host.g, 1, b, b, None, None, None, None) == lib.NIN_ENODEVICE
    assert L.nin_gls_corner_gradients_host(host.g, b, 1, b, None, None, None) == lib.NIN_ENODEVICE
    assert not host.buf.any()


def test_a_two_dimensional_grid_is_refused(lib, host):
    L = host.L
    I = UH.loaded(M.attach_fields(M.quad_tri_mesh_2d(4), "u", perm="LIN", neumann_plane=(1, 0.0), seed=5))
    assert int(I.grid.dim) == 2
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    for call in (lambda: L.nin_gls_corner_gradients_device(I.grid._h, 1, b, b, b, b, b, None),
                 lambda: L.nin_gls_corner_gradients_host(I.grid._h, b, 1, b, b, b, b)):
        assert call() == lib.NIN_EINVAL
        assert L.nin_last_error().decode() == TWO_D
    # the count is answered before the dimension
    assert L.nin_gls_corner_gradients_device(I.grid._h, 0, b, b, b, b, b, None) == lib.NIN_EINVAL and L.nin_last_error().decode() == N_FIELDS
    assert not host.buf.any()


@pytest.mark.parametrize("method", ("idw", "ls"))
def test_a_plan_of_idw_or_ls_is_refused(method):
    from ninpol_amd.interpolator import DevicePlan
    plan = DevicePlan.__new__(DevicePlan)          # (constructing one needs a device; the gate looks at the method alone)
    plan.method = method
    with pytest.raises(ValueError) as e:
        plan.launch_corner_gradients(8, 8)
    assert str(e.value) == (f"the weights of '{method}' are not the solution of a system that has cell gradients: "
                            "launch_corner_gradients is GLS only")


def test_python_surface_without_a_device():
    from ninpol_amd.interpolator import DevicePlan, Interpolator
    from ninpol_amd.torch_ops import CellToNode
    assert str(inspect.signature(DevicePlan.launch_corner_gradients)) == \
        "(self, u_ptr, grad_ptr, n_fields=1, node_values_ptr=0, flux_ptr=0, node_gradient_ptr=0, stream=0)"
    assert str(inspect.signature(Interpolator.corner_gradients)) == "(self, variable, values=None, flux=False)"
    assert str(inspect.signature(Interpolator.node_gradient)) == "(self, variable, values=None)"
    assert str(inspect.signature(CellToNode.corner_gradients)) == "(self, u)"
    assert "esup_ptr" in Interpolator.corner_gradients.__doc__ and "not a projection" in Interpolator.node_gradient.__doc__
    assert "NO autograd" in CellToNode.corner_gradients.__doc__
    with pytest.raises(ValueError, match="Grid not initialized"):
        Interpolator().corner_gradients("u")       # no mesh loaded
