"""The entry points of the kept GLS Jacobian in the node coordinates (nin_gls_xjacobian_*), without a device: what the
library declares, lists and builds for them, and the rows tests/test_abi_contract_host.py keeps for every status-returning entry point
-- NULL arguments, a host-only grid, a direction count below one.  An object exists only for a grid on a device, so on a host-only
grid the one call that takes the grid is nin_gls_xjacobian_create; every other entry point is given the NULL object."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import test_abi_contract_host as C
import test_update_fields_host as UH

lib = UH.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("nin_gls_xjacobian_create", "nin_gls_xjacobian_linearize", "nin_gls_xjacobian_apply", "nin_gls_xjacobian_apply_transpose",
               "nin_gls_xjacobian_records", "nin_gls_xjacobian_stamp", "nin_gls_xjacobian_destroy", "nin_gls_xjacobian_linearize_host",
               "nin_gls_xjacobian_apply_host", "nin_gls_xjacobian_apply_transpose_host", "nin_gls_xjacobian_fetch_host")
# (entry point, its arguments after the grid, tail of the text on a host-only grid): the form of test_abi_contract_host.TABLE
TABLE = (
    ("nin_gls_xjacobian_create", ("vp",), C.FIRST),
)
# (entry point, its arguments after the object): every one refuses the NULL object, and n < 1 where it takes a count
OBJECT_CALLS = (
    ("nin_gls_xjacobian_linearize", ("buf", "buf", None)),
    ("nin_gls_xjacobian_apply", (1, "buf", "buf", None)),
    ("nin_gls_xjacobian_apply_transpose", (1, "buf", "buf", None)),
    ("nin_gls_xjacobian_records", ("vp", "vp", "vp", "i64")),
    ("nin_gls_xjacobian_stamp", ("buf",)),
    ("nin_gls_xjacobian_linearize_host", ("buf", "buf")),
    ("nin_gls_xjacobian_apply_host", (1, "buf", "buf")),
    ("nin_gls_xjacobian_apply_transpose_host", (1, "buf", "buf")),
    ("nin_gls_xjacobian_fetch_host", ("buf", "buf", "buf")),
)


@pytest.fixture(scope="module")
def host(lib):
    return C.Host(lib)


def test_declared_listed_and_built(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", header), f"{name} is not declared in ninpol_amd.h"
        assert hasattr(L, name), f"{name} is not exported by the library"
    assert re.search(r"typedef\s+struct\s+nin_gls_xjacobian\s+nin_gls_xjacobian\s*;", header)
    vp, i32, pvp, pi64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)
    assert list(L.nin_gls_xjacobian_create.argtypes) == [vp, pvp]
    assert list(L.nin_gls_xjacobian_linearize.argtypes) == [vp, vp, vp, vp]
    assert list(L.nin_gls_xjacobian_apply.argtypes) == [vp, i32, vp, vp, vp]
    assert list(L.nin_gls_xjacobian_apply_transpose.argtypes) == [vp, i32, vp, vp, vp]
    assert list(L.nin_gls_xjacobian_records.argtypes) == [vp, pvp, pvp, pvp, pi64]
    assert list(L.nin_gls_xjacobian_stamp.argtypes) == [vp, vp]
    assert list(L.nin_gls_xjacobian_destroy.argtypes) == [vp] and L.nin_gls_xjacobian_destroy.restype is None
    assert list(L.nin_gls_xjacobian_linearize_host.argtypes) == [vp, vp, vp]
    assert list(L.nin_gls_xjacobian_apply_host.argtypes) == [vp, i32, vp, vp]
    assert list(L.nin_gls_xjacobian_apply_transpose_host.argtypes) == [vp, i32, vp, vp]
    assert list(L.nin_gls_xjacobian_fetch_host.argtypes) == [vp, vp, vp, vp]
    from ninpol_amd import build as nbuild
    units = {u[0]: u for u in nbuild.UNITS}
    assert units["kernels_gls_shape_jacobian.hip"][1:] == ("hipcc", [])         # no extra flags
    assert "abi_jacobian_points.hip" in units


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_null_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_host_only_grid(lib, host, name, spec, tail):
    host.vp.value = 0xdead
    rc, text = host.call(name, host.g, spec)
    assert rc == lib.NIN_ENODEVICE, (name, rc, text)
    assert text == C.NOT_ON_DEVICE + tail, (name, text)
    assert host.vp.value is None and not host.buf.any()                    # nothing is left behind, a refused call wrote nothing
    from ninpol_amd.interpolator import GlsShapeJacobian
    with pytest.raises(lib.NinpolError) as e:
        GlsShapeJacobian(host.I.grid)
    assert e.value.code == lib.NIN_ENODEVICE
    assert host.L.nin_grid_device(host.g) == -1


@pytest.mark.parametrize("name,spec", OBJECT_CALLS, ids=[t[0] for t in OBJECT_CALLS])
def test_null_object(lib, host, name, spec):
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)
    assert not host.buf.any() and host.vp.value is None and host.i64.value == 0


def test_null_and_zero_arguments(lib, host):
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    assert L.nin_gls_xjacobian_create(host.g, None) == lib.NIN_EINVAL
    # n < 1 is refused before anything else is looked at, in the words of the kept Jacobian in K
    for n in (0, -1):
        for call, sibling in ((lambda: L.nin_gls_xjacobian_apply(None, n, b, b, None), lambda: L.nin_gls_jacobian_apply(None, n, b, None, b, None)),
                              (lambda: L.nin_gls_xjacobian_apply_transpose(None, n, b, b, None),
                               lambda: L.nin_gls_jacobian_apply_transpose(None, n, b, b, None, None)),
                              (lambda: L.nin_gls_xjacobian_apply_host(None, n, b, b), lambda: L.nin_gls_jacobian_apply_host(None, n, b, None, b)),
                              (lambda: L.nin_gls_xjacobian_apply_transpose_host(None, n, b, b),
                               lambda: L.nin_gls_jacobian_apply_transpose_host(None, n, b, b, None))):
            rc, text = call(), L.nin_last_error().decode()
            rc_k, text_k = sibling(), L.nin_last_error().decode()
            assert rc == rc_k == lib.NIN_EINVAL and text == text_k == "n must be >= 1", (n, rc, text, rc_k, text_k)
    L.nin_gls_xjacobian_destroy(None)                                      # a NULL object is a no-op
    assert L.nin_grid_scalar(host.g, b"gls_shape_tangent_bytes") == 0
    assert L.nin_grid_scalar(host.g, b"gls_shape_contrib_bytes") == 0 and L.nin_grid_scalar(host.g, b"gls_adjoint_contrib_bytes") == 0
    assert not host.buf.any()


def test_python_surface_without_a_device():
    import scipy.sparse.linalg as spla
    import torch
    from ninpol_amd.interpolator import DevicePlan, GlsShapeJacobian, Interpolator, PointsJacobian
    from ninpol_amd.torch_ops import CellToNode, Linearization
    sig = inspect.signature(DevicePlan.linearize_points)
    assert list(sig.parameters) == ["self", "u_ptr", "neumann_values_ptr", "stream"]
    assert [sig.parameters[k].default for k in ("neumann_values_ptr", "stream")] == [0, 0]
    sig = inspect.signature(GlsShapeJacobian.launch_jvp)
    assert list(sig.parameters) == ["self", "dX_ptr", "out_ptr", "n", "stream"] and [sig.parameters[k].default for k in ("n", "stream")] == [1, 0]
    sig = inspect.signature(GlsShapeJacobian.launch_vjp)
    assert list(sig.parameters) == ["self", "v_ptr", "grad_points_ptr", "n", "stream"] and [sig.parameters[k].default for k in ("n", "stream")] == [1, 0]
    assert list(inspect.signature(GlsShapeJacobian.relinearize).parameters) == ["self", "u_ptr", "neumann_values_ptr", "stream"]
    for name in ("nbytes", "stamp"):
        assert isinstance(getattr(GlsShapeJacobian, name), property)
    for name in ("fetch", "is_current", "release", "__del__"):
        assert callable(getattr(GlsShapeJacobian, name))
    sig = inspect.signature(Interpolator.points_jacobian)
    assert list(sig.parameters) == ["self", "variable", "cell_values", "neumann_values"]
    assert issubclass(PointsJacobian, spla.LinearOperator) and not hasattr(PointsJacobian, "to_scipy")
    assert "to_scipy" in PointsJacobian.__doc__ and "to_scipy" in Interpolator.points_jacobian.__doc__      # (and say that there is none)
    for name in ("_matvec", "_rmatvec", "_matmat", "_rmatmat", "release"):
        assert name in vars(PointsJacobian)
    sig = inspect.signature(CellToNode.linearize)
    assert list(sig.parameters) == ["self", "u", "K", "scale", "points", "neumann_values", "wrt"] and sig.parameters["wrt"].default == "K"
    assert list(inspect.signature(Linearization.jvp).parameters) == ["self", "du", "dK", "dscale", "dpoints"]
    # the checks that need no device: a plan of another method, a NULL u, an unknown wrt
    plan = DevicePlan.__new__(DevicePlan)      # (constructing one needs a device: the checks come first and need none)
    for method in ("idw", "ls"):
        plan.method = method
        with pytest.raises(ValueError, match="do depend on the node coordinates, but they are not differentiated"):
            plan.linearize_points(8)
    plan.method = "gls"
    with pytest.raises(ValueError, match="u_ptr"):
        plan.linearize_points(0)
    op = CellToNode.__new__(CellToNode)        # (constructing one needs a device)
    for k, v in (("n_elems", 27), ("n_points", 64), ("device", torch.device("cuda", 0))):
        object.__setattr__(op, k, v)
    with pytest.raises(ValueError, match="wrt must be"):
        op.linearize(torch.zeros(27, dtype=torch.float64), wrt="X")
    for method in ("idw", "ls"):
        plan.method = method
        object.__setattr__(op, "plan", plan)
        with pytest.raises(ValueError, match="not differentiated"):
            op.linearize(torch.zeros(27, dtype=torch.float64), wrt="points")
    # a linearisation refuses the directions it holds no derivative for, in the words of the wrt="scale" refusal
    lin = Linearization.__new__(Linearization)
    lin.op, lin.wrt, lin.K, lin.scale = op, "points", None, None
    for kw in ("dK", "dscale"):
        with pytest.raises(ValueError, match='a linearisation taken with wrt="points" holds no derivative in K: ' + kw + ' must be None'):
            lin.jvp(**{kw: torch.zeros(27, dtype=torch.float64)})
    lin.wrt = "K"
    with pytest.raises(ValueError, match="dpoints must be None"):
        lin.jvp(dpoints=torch.zeros((64, 3), dtype=torch.float64))


def test_points_jacobian_validates_before_the_device(lib):
    I = C.Host(lib).I
    P, E = I.grid.n_points, I.grid.n_elems
    for variable, u, b in (("u", np.zeros(P), None), ("u", np.zeros((1, E)), None), ("u", None, np.zeros(E)), ("u", np.zeros(E), np.zeros((1, P))),
                           ("nope", None, None)):
        with pytest.raises(ValueError):
            I.points_jacobian(variable, u, b)
        assert I.grid.device == -1, (variable, np.shape(u), np.shape(b))
