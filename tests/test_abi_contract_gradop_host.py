"""The entry points of the kept corner-gradient operator (nin_gls_gradop_*), without a device: what the library
declares, lists and builds for them, and every refusal that needs no device with its text -- NULL arguments, n < 1 before a NULL-free
call's other answers, a 2-D grid (answered before the grid's residency, so a host-only grid shows it), a host-only 3-D grid, a plan of
IDW or LS -- and the Python surface."""
import ctypes
import inspect
import os
import re

import pytest

import test_abi_contract_host as C
import test_update_fields_host as UH
from ninpol_amd import mesh as M

lib = UH.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("nin_gls_gradop_bytes", "nin_gls_gradop_create", "nin_gls_gradop_factorize", "nin_gls_gradop_apply", "nin_gls_gradop_apply_transpose",
         "nin_gls_gradop_records", "nin_gls_gradop_stamp", "nin_gls_gradop_factorize_host", "nin_gls_gradop_apply_host",
         "nin_gls_gradop_apply_transpose_host", "nin_gls_gradop_fetch_host")
NULL_ARGUMENT, COUNT = "NULL argument", "n must be >= 1"
TWO_D = "the gradient operator is for 3-D grids only (this grid is 2-D)"


@pytest.fixture(scope="module")
def host(lib):
    return C.Host(lib)


def test_declared_listed_and_built(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    L = lib.load()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    for name in NAMES:
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in ninpol_amd.h"
        assert hasattr(L, name)
    assert "nin_gls_gradop_destroy" in lib.EXPORTS and re.search(r"\bvoid\s+nin_gls_gradop_destroy\s*\(", header)
    assert list(L.nin_gls_gradop_apply.argtypes) == [vp, i32, vp, vp, vp, vp, vp]
    assert list(L.nin_gls_gradop_apply_transpose.argtypes) == [vp, i32, vp, vp, vp]
    assert list(L.nin_gls_gradop_apply_host.argtypes) == [vp, i32, vp, vp, vp, vp]
    assert list(L.nin_gls_gradop_bytes.argtypes) == [vp, ctypes.POINTER(i64)]
    assert L.nin_gls_gradop_destroy.restype is None
    build = open(os.path.join(ROOT, "ninpol_amd", "build.py")).read()
    assert '("kernels_gls_gradop.hip", "hipcc", ["-ffp-contract=off"])' in build and '"abi_gradop.hip"' in build


def test_a_null_object_or_argument_is_refused(lib, host):
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    n64, h = ctypes.c_int64(-7), ctypes.c_void_p(12345)
    for call in (lambda: L.nin_gls_gradop_bytes(None, ctypes.byref(n64)),
                 lambda: L.nin_gls_gradop_bytes(host.g, None),
                 lambda: L.nin_gls_gradop_create(None, ctypes.byref(h)),
                 lambda: L.nin_gls_gradop_create(host.g, None),
                 lambda: L.nin_gls_gradop_factorize(None, None),
                 lambda: L.nin_gls_gradop_factorize_host(None),
                 lambda: L.nin_gls_gradop_apply(None, 1, b, b, b, b, None),
                 lambda: L.nin_gls_gradop_apply(None, 0, b, b, b, b, None),                   # NULL before the count
                 lambda: L.nin_gls_gradop_apply_transpose(None, 1, b, b, None),
                 lambda: L.nin_gls_gradop_apply_host(None, 1, b, b, None, None),
                 lambda: L.nin_gls_gradop_apply_transpose_host(None, 1, b, b),
                 lambda: L.nin_gls_gradop_records(None, ctypes.byref(h), ctypes.byref(h), ctypes.byref(n64), None),
                 lambda: L.nin_gls_gradop_stamp(None, b),
                 lambda: L.nin_gls_gradop_fetch_host(None, b, b)):
        assert call() == lib.NIN_EINVAL
        assert L.nin_last_error().decode() == NULL_ARGUMENT
    assert h.value is None                                               # create clears its output before it refuses
    assert n64.value == -7 and not host.buf.any()
    L.nin_gls_gradop_destroy(None)                                       # a no-op


def test_dimension_before_residency(lib, host):
    """a host-only 2-D grid is refused for its dimension, a host-only 3-D grid for its residency: the order of DESIGN.md 4.21"""
    L = host.L
    I = UH.loaded(M.attach_fields(M.quad_tri_mesh_2d(4), "u", perm="LIN", neumann_plane=(1, 0.0), seed=5))
    assert int(I.grid.dim) == 2
    n64, h = ctypes.c_int64(-7), ctypes.c_void_p()
    for call in (lambda: L.nin_gls_gradop_bytes(I.grid._h, ctypes.byref(n64)), lambda: L.nin_gls_gradop_create(I.grid._h, ctypes.byref(h))):
        assert call() == lib.NIN_EINVAL
        assert L.nin_last_error().decode() == TWO_D
    for call in (lambda: L.nin_gls_gradop_bytes(host.g, ctypes.byref(n64)), lambda: L.nin_gls_gradop_create(host.g, ctypes.byref(h))):
        assert call() == lib.NIN_ENODEVICE
        assert L.nin_last_error().decode() == C.NOT_ON_DEVICE + C.FIRST
    assert n64.value == -7 and h.value is None


@pytest.mark.parametrize("method", ("idw", "ls"))
def test_a_plan_of_idw_or_ls_is_refused(method):
    from ninpol_amd.interpolator import DevicePlan
    plan = DevicePlan.__new__(DevicePlan)          # (constructing one needs a device; the gate looks at the method alone)
    plan.method = method
    with pytest.raises(ValueError) as e:
        plan.gradient_operator()
    assert str(e.value) == (f"the weights of '{method}' are not the solution of a system that has cell gradients: "
                            "gradient_operator is GLS only")


def test_python_surface_without_a_device():
    import scipy.sparse.linalg as spla
    from ninpol_amd.interpolator import DevicePlan, GlsGradientOperator, GradientOperator, Interpolator
    assert str(inspect.signature(DevicePlan.gradient_operator)) == "(self, stream=0)"
    assert str(inspect.signature(Interpolator.gradient_operator)) == "(self, variable)"
    assert str(inspect.signature(GlsGradientOperator.launch_apply)) == "(self, u_ptr, grad_ptr, n=1, flux_ptr=0, node_gradient_ptr=0, stream=0)"
    assert str(inspect.signature(GlsGradientOperator.launch_apply_transpose)) == "(self, gbar_ptr, ubar_ptr, n=1, stream=0)"
    for name in ("nbytes", "stale", "n_values", "record_ptrs", "stamp"):
        assert isinstance(inspect.getattr_static(GlsGradientOperator, name), property), name
    for name in ("factorize", "fetch", "release", "is_current"):
        assert callable(getattr(GlsGradientOperator, name)), name
    assert issubclass(GradientOperator, spla.LinearOperator)
    for name in ("_matvec", "_rmatvec", "_matmat", "_rmatmat", "update", "to_scipy", "release"):
        assert callable(getattr(GradientOperator, name)), name
    op = GlsGradientOperator.__new__(GlsGradientOperator)               # a released object is one without its handle
    op._h, op.plan, op.grid = None, None, None
    for call in (lambda: op.factorize(), lambda: op.launch_apply(8, 8), lambda: op.launch_apply_transpose(8, 8), lambda: op.fetch(),
                 lambda: op.nbytes, lambda: op.stale):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "this GlsGradientOperator was released"
    with pytest.raises(ValueError, match="Grid not initialized"):
        Interpolator().gradient_operator("u")       # no mesh loaded
