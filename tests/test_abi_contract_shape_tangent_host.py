"""The two entry points of the GLS tangent in the node coordinates, without a device: the rows tests/test_abi_contract_host.py keeps
for every status-returning entry point -- a NULL grid, a host-only grid -- and what the library declares, lists and builds for them."""
import ctypes
import os
import re

import pytest

import test_abi_contract_host as C
import test_update_fields_host as UH

lib = UH.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (entry point, its arguments after the grid, tail of the text on a host-only grid): the form of test_abi_contract_host.TABLE
TABLE = (
    ("nin_gls_weights_tangent_points_device", (1, 1, "buf", "buf", "buf", None), C.KERNELS),
    ("nin_gls_points_tangent_host", ("buf", "buf", 1, "buf", "buf"), C.KERNELS),
)


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
    assert list(L.nin_gls_weights_tangent_points_device.argtypes) == [vp, i32, i32, vp, vp, vp, vp]
    assert list(L.nin_gls_points_tangent_host.argtypes) == [vp, vp, vp, i32, vp, vp]


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_null_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_host_only_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, host.g, spec)
    assert rc == lib.NIN_ENODEVICE, (name, rc, text)
    assert text == C.NOT_ON_DEVICE + tail, (name, text)
    assert not host.buf.any()                                            # a refused call wrote nothing


def test_null_and_zero_arguments(lib, host):
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    for call in (lambda: L.nin_gls_weights_tangent_points_device(host.g, 1, 1, None, b, b, None),
                 lambda: L.nin_gls_weights_tangent_points_device(host.g, 1, 1, b, None, b, None),
                 lambda: L.nin_gls_weights_tangent_points_device(host.g, 1, 0, b, b, b, None),
                 lambda: L.nin_gls_points_tangent_host(host.g, None, b, 1, b, b),
                 lambda: L.nin_gls_points_tangent_host(host.g, b, None, 1, b, b),
                 lambda: L.nin_gls_points_tangent_host(host.g, b, b, 1, None, b),
                 lambda: L.nin_gls_points_tangent_host(host.g, b, b, 1, b, None),
                 lambda: L.nin_gls_points_tangent_host(host.g, b, b, 0, b, b)):
        assert call() == lib.NIN_EINVAL
    # neumann_ws of the device call is optional: without it the call gets as far as the grid's residency
    assert L.nin_gls_weights_tangent_points_device(host.g, 1, 1, b, b, None, None) == lib.NIN_ENODEVICE
    assert L.nin_grid_scalar(host.g, b"gls_shape_tangent_bytes") == 0
    assert L.nin_grid_scalar(host.g, b"gls_shape_contrib_bytes") == 0 and L.nin_grid_scalar(host.g, b"gls_adjoint_contrib_bytes") == 0
    assert not host.buf.any()


def test_python_surface_without_a_device():
    import inspect
    from ninpol_amd.interpolator import DevicePlan, Interpolator
    sig = inspect.signature(DevicePlan.launch_weights_tangent_points)
    assert list(sig.parameters) == ["self", "tangent_points_ptr", "tangent_csr_ptr", "n_tangents", "tangent_neumann_ws_ptr", "stream", "add_neumann"]
    assert [sig.parameters[k].default for k in ("n_tangents", "tangent_neumann_ws_ptr", "stream", "add_neumann")] == [1, 0, 0, True]
    sig = inspect.signature(Interpolator.points_tangent)
    assert list(sig.parameters) == ["self", "variable", "dX", "cell_values"] and sig.parameters["cell_values"].default is None
