"""CPU-side tests of the resident GLS Jacobian's entry points (no GPU needed): the new symbols are declared, listed and exported; a
host-only grid is refused with NIN_ENODEVICE and bad arguments with NIN_EINVAL; DevicePlan.linearize, Interpolator.permeability_jacobian
and CellToNode.linearize validate their arguments before they touch a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ninpol_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nin_gls_jacobian_create", "nin_gls_jacobian_linearize", "nin_gls_jacobian_apply", "nin_gls_jacobian_apply_transpose",
               "nin_gls_jacobian_contrib", "nin_gls_jacobian_stamp", "nin_gls_jacobian_destroy", "nin_gls_jacobian_linearize_host",
               "nin_gls_jacobian_apply_host", "nin_gls_jacobian_apply_transpose_host", "nin_gls_jacobian_fetch_host")


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
    M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(2, 0.0))
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    assert I.grid.device == -1
    return I


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _assert_code(L, rc, code, what):
    assert rc == code, (what, rc)
    assert L.nin_last_error().decode().strip(), (what, "no error text")


def test_the_entry_points_are_declared_listed_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ninpol_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/ninpol_amd.h"
        assert name in lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(L, name), f"{name} is not exported by the library"
    assert re.search(r"typedef\s+struct\s+nin_gls_jacobian\s+nin_gls_jacobian\s*;", header)
    Lb = lib.load()
    vp, i32, pvp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)
    assert list(Lb.nin_gls_jacobian_create.argtypes) == [vp, pvp]
    assert list(Lb.nin_gls_jacobian_linearize.argtypes) == [vp, vp, vp, vp]
    assert list(Lb.nin_gls_jacobian_apply.argtypes) == [vp, i32, vp, vp, vp, vp]
    assert list(Lb.nin_gls_jacobian_apply_transpose.argtypes) == [vp, i32, vp, vp, vp, vp]
    assert list(Lb.nin_gls_jacobian_contrib.argtypes) == [vp, pvp, pvp]
    assert list(Lb.nin_gls_jacobian_stamp.argtypes) == [vp, vp]
    assert list(Lb.nin_gls_jacobian_destroy.argtypes) == [vp] and Lb.nin_gls_jacobian_destroy.restype is None
    assert list(Lb.nin_gls_jacobian_linearize_host.argtypes) == [vp, vp, vp]
    assert list(Lb.nin_gls_jacobian_apply_host.argtypes) == [vp, i32, vp, vp, vp]
    assert list(Lb.nin_gls_jacobian_apply_transpose_host.argtypes) == [vp, i32, vp, vp, vp]
    assert list(Lb.nin_gls_jacobian_fetch_host.argtypes) == [vp, vp, vp]


def test_the_jacobian_units_are_built():
    from ninpol_amd import build as nbuild
    units = {u[0]: u for u in nbuild.UNITS}
    assert units["kernels_gls_jacobian.hip"][1:] == ("hipcc", [])         # no extra flags
    assert "abi_jacobian.hip" in units


def test_host_only_grid_is_enodevice(lib, host_interp):
    L, g = lib.load(), host_interp.grid
    h = ctypes.c_void_p(0xdead)
    _assert_code(L, L.nin_gls_jacobian_create(g._h, ctypes.byref(h)), lib.NIN_ENODEVICE, "create")
    assert h.value is None                                                # nothing is left behind
    assert "not on a device" in L.nin_last_error().decode()
    L.nin_gls_jacobian_destroy(None)                                      # a NULL object is a no-op
    from ninpol_amd.interpolator import GlsJacobian
    with pytest.raises(lib.NinpolError) as e:
        GlsJacobian(g)
    assert e.value.code == lib.NIN_ENODEVICE
    assert g._scalar("gls_adjoint_contrib_bytes") == 0 and g.device == -1


def test_null_arguments_and_direction_counts_are_einval(lib, host_interp):
    L, g = lib.load(), host_interp.grid
    E, P, K = np.zeros(g.n_elems), np.zeros(g.n_points), np.zeros(9 * g.n_elems)
    h, a, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    stamp = np.zeros(3, dtype=np.int64)
    bad = {
        "create, grid": lambda: L.nin_gls_jacobian_create(None, ctypes.byref(h)),
        "create, out": lambda: L.nin_gls_jacobian_create(g._h, None),
        "linearize, object": lambda: L.nin_gls_jacobian_linearize(None, _p(E), None, None),
        "apply, object": lambda: L.nin_gls_jacobian_apply(None, 1, _p(K), None, _p(P), None),
        "apply, n = 0": lambda: L.nin_gls_jacobian_apply(None, 0, _p(K), None, _p(P), None),
        "apply_transpose, object": lambda: L.nin_gls_jacobian_apply_transpose(None, 1, _p(P), _p(K), None, None),
        "apply_transpose, n = -1": lambda: L.nin_gls_jacobian_apply_transpose(None, -1, _p(P), _p(K), None, None),
        "contrib, object": lambda: L.nin_gls_jacobian_contrib(None, ctypes.byref(a), ctypes.byref(b)),
        "stamp, object": lambda: L.nin_gls_jacobian_stamp(None, _p(stamp)),
        "linearize_host, object": lambda: L.nin_gls_jacobian_linearize_host(None, _p(E), None),
        "apply_host, n = 0": lambda: L.nin_gls_jacobian_apply_host(None, 0, _p(K), None, _p(P)),
        "apply_transpose_host, object": lambda: L.nin_gls_jacobian_apply_transpose_host(None, 1, _p(P), _p(K), None),
        "fetch_host, object": lambda: L.nin_gls_jacobian_fetch_host(None, _p(K), _p(E)),
    }
    for what, call in bad.items():
        _assert_code(L, call(), lib.NIN_EINVAL, what)
    L.nin_gls_jacobian_apply(None, 0, _p(K), None, _p(P), None)
    assert "n must be >= 1" in L.nin_last_error().decode()


def test_permeability_jacobian_validates_before_the_device(lib, host_interp):
    I = host_interp
    P, E = I.grid.n_points, I.grid.n_elems
    bad = [("u", np.zeros(P), None),                          # node-sized cell values
           ("u", np.zeros((1, E)), None),                     # one field only
           ("u", np.zeros((2, E)), None),
           ("u", None, np.zeros(E)),                          # cell-sized neumann values
           ("u", np.zeros(E), np.zeros((1, P))),
           ("u", np.array(["a"] * E), None),                  # not numbers
           ("nope", None, None)]
    for variable, u, b in bad:
        with pytest.raises(ValueError):
            I.permeability_jacobian(variable, u, b)
        assert I.grid.device == -1, (variable, np.shape(u), np.shape(b))


def test_permeability_jacobian_needs_a_mesh_and_a_permeability(lib):
    import ninpol_amd
    with pytest.raises(ValueError, match="Grid not initialized"):
        ninpol_amd.Interpolator().permeability_jacobian("u")
    mesh = M.hex_mesh(2)
    mesh.cell_data = {"u": [np.zeros(len(b.data)) for b in mesh.cells]}
    mesh.point_data = {"neumann_flag_u": np.zeros(len(mesh.points)), "neumann_u": np.zeros(len(mesh.points))}
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    with pytest.raises(ValueError, match="permeability"):
        I.permeability_jacobian("u")


def test_the_python_surface():
    from ninpol_amd.interpolator import DevicePlan, GlsJacobian, HostMatrix, PermeabilityJacobian
    import scipy.sparse.linalg as spla
    sig = inspect.signature(DevicePlan.linearize)
    assert list(sig.parameters) == ["self", "u_ptr", "neumann_values_ptr", "stream"]
    assert [sig.parameters[k].default for k in ("neumann_values_ptr", "stream")] == [0, 0]
    sig = inspect.signature(GlsJacobian.launch_jvp)
    assert list(sig.parameters) == ["self", "dperm_ptr", "out_ptr", "n", "ddm_ptr", "stream"]
    assert [sig.parameters[k].default for k in ("n", "ddm_ptr", "stream")] == [1, 0, 0]
    sig = inspect.signature(GlsJacobian.launch_vjp)
    assert list(sig.parameters) == ["self", "v_ptr", "grad_perm_ptr", "n", "grad_dm_ptr", "stream"]
    assert [sig.parameters[k].default for k in ("n", "grad_dm_ptr", "stream")] == [1, 0, 0]
    assert list(inspect.signature(GlsJacobian.relinearize).parameters) == ["self", "u_ptr", "neumann_values_ptr", "stream"]
    for name in ("contrib_ptr", "fold_ptr", "stamp"):
        assert isinstance(getattr(GlsJacobian, name), property)
    for name in ("is_current", "release", "__del__"):
        assert callable(getattr(GlsJacobian, name))
    assert callable(HostMatrix.release)        # (the lifetime model GlsJacobian follows)
    assert issubclass(PermeabilityJacobian, spla.LinearOperator)
    for name in ("_matvec", "_rmatvec", "_matmat", "_rmatmat", "to_scipy", "release"):
        assert name in vars(PermeabilityJacobian)


def test_a_plan_of_another_method_is_refused_before_the_device():
    from ninpol_amd.interpolator import DevicePlan
    plan = DevicePlan.__new__(DevicePlan)      # (constructing one needs a device: the checks come first and need none)
    for method in ("idw", "ls"):
        plan.method = method
        with pytest.raises(ValueError, match="GLS only"):
            plan.linearize(8)
    plan.method = "gls"
    with pytest.raises(ValueError, match="u_ptr"):
        plan.linearize(0)


def test_cell_to_node_linearize_validates_before_the_device():
    import torch
    from ninpol_amd.torch_ops import CellToNode
    op = CellToNode.__new__(CellToNode)        # (constructing one needs a device)
    for k, v in (("n_elems", 27), ("n_points", 64), ("device", torch.device("cuda", 0))):
        object.__setattr__(op, k, v)
    with pytest.raises(TypeError, match="torch.Tensor"):
        op.linearize(np.zeros(27))
    with pytest.raises(TypeError, match="float64"):
        op.linearize(torch.zeros(27, dtype=torch.float32))
    for shape in ((26,), (1, 27), (2, 27), ()):
        with pytest.raises(ValueError, match="shape"):
            op.linearize(torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError, match="must be on"):
        op.linearize(torch.zeros(27, dtype=torch.float64))        # a host tensor
