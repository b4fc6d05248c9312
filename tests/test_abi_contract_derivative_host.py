"""The derivative layer of the GLS weights, without a device: what tests/test_abi_contract_host.py keeps for every status-returning
entry point -- a NULL grid, a host-only grid -- for the two entry points of the tangent; what the entry points of the two kept
Jacobians answer before they look at an object (tests/test_gls_jacobian_host.py and tests/test_gls_reduced_jacobian_host.py hold the
rest); and the Python surface over them: signatures, import paths, the text of a released object."""
import ctypes
import inspect

import numpy as np
import pytest

import test_abi_contract_host as C
import test_update_fields_host as UH

lib = UH.lib

# (entry point, its arguments after the grid, tail of the text on a host-only grid): the form of test_abi_contract_host.TABLE
TABLE = (
    ("nin_gls_weights_tangent_device", (1, 1, "buf", "buf", "buf", "buf", None), C.KERNELS),
    ("nin_gls_permeability_tangent_host", ("buf", "buf", 1, "buf", "buf"), C.KERNELS),
)
NULL_ARGUMENT, N_FIRST = "NULL argument", "n must be >= 1"


@pytest.fixture(scope="module")
def host(lib):
    return C.Host(lib)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_null_grid(lib, host, name, spec, tail):
    assert name in lib.EXPORTS
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_host_only_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, host.g, spec)
    assert rc == lib.NIN_ENODEVICE, (name, rc, text)
    assert text == C.NOT_ON_DEVICE + tail, (name, text)
    assert not host.buf.any()                                            # a refused call wrote nothing


def test_tangent_null_arguments_and_counts(lib, host):
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    text = lambda: L.nin_last_error().decode()
    for call, want in ((lambda: L.nin_gls_weights_tangent_device(host.g, 1, 1, None, None, b, None, None), NULL_ARGUMENT),
                       (lambda: L.nin_gls_weights_tangent_device(host.g, 1, 1, b, None, None, None, None), NULL_ARGUMENT),
                       (lambda: L.nin_gls_weights_tangent_device(host.g, 1, 0, b, None, b, None, None), "n_tangents must be >= 1"),
                       (lambda: L.nin_gls_weights_tangent_device(host.g, 1, -1, b, b, b, b, None), "n_tangents must be >= 1"),
                       (lambda: L.nin_gls_weights_tangent_device(host.g, 1, 0, None, None, b, None, None), NULL_ARGUMENT),   # NULL first
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, None, b, 1, b, b), NULL_ARGUMENT),
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, b, None, 1, b, b), NULL_ARGUMENT),
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, b, b, 1, None, b), NULL_ARGUMENT),
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, b, b, 1, b, None), NULL_ARGUMENT),
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, b, b, 0, b, b), "n_fields must be >= 1"),
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, b, b, -1, b, b), "n_fields must be >= 1"),
                       (lambda: L.nin_gls_permeability_tangent_host(host.g, b, b, 0, b, None), NULL_ARGUMENT)):              # NULL first
        assert call() == lib.NIN_EINVAL
        assert text() == want
    # the optional arguments may be NULL: the refusal is the grid's, not theirs
    assert L.nin_gls_weights_tangent_device(host.g, 1, 1, b, None, b, None, None) == lib.NIN_ENODEVICE
    assert not host.buf.any()


def test_jacobian_apply_counts_come_before_null_arguments(lib, host):
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    text = lambda: L.nin_last_error().decode()
    applies = {   # every apply entry point of the two kept Jacobians, as a call of (object, n)
        "nin_gls_jacobian_apply": lambda J, n: L.nin_gls_jacobian_apply(J, n, b, None, b, None),
        "nin_gls_jacobian_apply_transpose": lambda J, n: L.nin_gls_jacobian_apply_transpose(J, n, b, b, None, None),
        "nin_gls_jacobian_apply_host": lambda J, n: L.nin_gls_jacobian_apply_host(J, n, b, None, b),
        "nin_gls_jacobian_apply_transpose_host": lambda J, n: L.nin_gls_jacobian_apply_transpose_host(J, n, b, b, None),
        "nin_gls_rjacobian_apply": lambda J, n: L.nin_gls_rjacobian_apply(J, n, b, b, None),
        "nin_gls_rjacobian_apply_transpose": lambda J, n: L.nin_gls_rjacobian_apply_transpose(J, n, b, b, None),
        "nin_gls_rjacobian_apply_host": lambda J, n: L.nin_gls_rjacobian_apply_host(J, n, b, b),
        "nin_gls_rjacobian_apply_transpose_host": lambda J, n: L.nin_gls_rjacobian_apply_transpose_host(J, n, b, b),
    }
    for name, call in applies.items():
        for n in (0, -1):
            assert call(None, n) == lib.NIN_EINVAL and text() == N_FIRST, (name, n, text())     # n < 1 before the NULL object
        assert call(None, 1) == lib.NIN_EINVAL and text() == NULL_ARGUMENT, (name, text())
    assert not host.buf.any()


def test_jacobian_create_on_a_host_only_grid(lib, host):
    L = host.L
    h = ctypes.c_void_p(0xdead)
    assert L.nin_gls_jacobian_create(host.g, ctypes.byref(h)) == lib.NIN_ENODEVICE
    assert L.nin_last_error().decode() == C.NOT_ON_DEVICE + C.FIRST and h.value is None
    for m in (1, 3, 6):
        h = ctypes.c_void_p(0xdead)
        assert L.nin_gls_rjacobian_create(host.g, m, ctypes.byref(h)) == lib.NIN_ENODEVICE
        assert L.nin_last_error().decode() == C.NOT_ON_DEVICE + C.FIRST and h.value is None
    # the parameter count is answered before the grid is looked at, the NULL arguments before either
    h = ctypes.c_void_p(0xdead)
    assert L.nin_gls_rjacobian_create(host.g, 2, ctypes.byref(h)) == lib.NIN_EINVAL
    assert L.nin_last_error().decode() == "n_params must be 1, 3 or 6, not 2" and h.value is None
    assert L.nin_gls_rjacobian_create(host.g, 2, None) == lib.NIN_EINVAL and L.nin_last_error().decode() == NULL_ARGUMENT
    assert L.nin_gls_jacobian_create(None, None) == lib.NIN_EINVAL and L.nin_last_error().decode() == NULL_ARGUMENT


def test_jacobian_getters_with_null_outputs(lib, host):
    """a NULL output is answered before the object is read: `obj` is some non-NULL address, never a Jacobian"""
    L = host.L
    obj = host.buf.ctypes.data_as(ctypes.c_void_p)
    a, b, m = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xdead), ctypes.c_int(-7)
    for call in (lambda: L.nin_gls_jacobian_stamp(obj, None),
                 lambda: L.nin_gls_jacobian_stamp(None, None),
                 lambda: L.nin_gls_rjacobian_stamp(obj, None),
                 lambda: L.nin_gls_rjacobian_stamp(None, None),
                 lambda: L.nin_gls_jacobian_contrib(obj, None, ctypes.byref(b)),
                 lambda: L.nin_gls_jacobian_contrib(obj, ctypes.byref(a), None),
                 lambda: L.nin_gls_jacobian_contrib(None, None, None),
                 lambda: L.nin_gls_rjacobian_buffer(obj, None, ctypes.byref(m)),
                 lambda: L.nin_gls_rjacobian_buffer(obj, ctypes.byref(a), None),
                 lambda: L.nin_gls_rjacobian_buffer(None, None, None)):
        assert call() == lib.NIN_EINVAL
        assert L.nin_last_error().decode() == NULL_ARGUMENT
    assert (a.value, b.value, m.value) == (0xdead, 0xdead, -7)            # a refused call wrote nothing
    assert not host.buf.any()


# str(inspect.signature(...)) of every public method; the properties by name
SURFACE = {
    "GlsJacobian": ({"__init__": "(self, grid, plan=None)",
                     "relinearize": "(self, u_ptr, neumann_values_ptr=0, stream=0)",
                     "launch_jvp": "(self, dperm_ptr, out_ptr, n=1, ddm_ptr=0, stream=0)",
                     "launch_vjp": "(self, v_ptr, grad_perm_ptr, n=1, grad_dm_ptr=0, stream=0)",
                     "is_current": "(self)", "fetch": "(self)", "release": "(self)"}, ("contrib_ptr", "fold_ptr", "stamp")),
    "GlsReducedJacobian": ({"__init__": "(self, grid, n_params=1, plan=None)",
                            "relinearize": "(self, u_ptr, basis_ptr=0, basis_per_cell=True, neumann_values_ptr=0, stream=0)",
                            "launch_jvp": "(self, dtheta_ptr, out_ptr, n=1, stream=0)",
                            "launch_vjp": "(self, v_ptr, grad_theta_ptr, n=1, stream=0)",
                            "is_current": "(self)", "fetch": "(self)", "release": "(self)"}, ("buffer_ptr", "stamp")),
    "PermeabilityJacobian": ({"__init__": "(self, jac)", "to_scipy": "(self)", "release": "(self)"}, ()),
    "ReducedPermeabilityJacobian": ({"__init__": "(self, jac)", "to_scipy": "(self)", "release": "(self)"}, ()),
    "DevicePlan": ({
        "launch_weights_backward": "(self, grad_csr_ptr, grad_perm_ptr, grad_diff_mag_ptr=0, grad_neumann_ws_ptr=0, stream=0, add_neumann=True)",
        "launch_weights_backward_points": "(self, grad_csr_ptr, grad_points_ptr, grad_neumann_ws_ptr=0, stream=0, add_neumann=True)",
        "launch_weights_tangent": "(self, tangent_perm_ptr, tangent_csr_ptr, n_tangents=1, tangent_diff_mag_ptr=0, tangent_neumann_ws_ptr=0, "
                                  "stream=0, add_neumann=True)",
        "linearize": "(self, u_ptr, neumann_values_ptr=0, stream=0)",
        "linearize_reduced": "(self, u_ptr, n_params=1, basis_ptr=0, basis_per_cell=True, neumann_values_ptr=0, stream=0)"}, ()),
}


def test_python_surface_without_a_device():
    from ninpol_amd import interpolator
    from ninpol_amd.interpolator import (DevicePlan, GlsJacobian, GlsReducedJacobian, PermeabilityJacobian,  # noqa: F401
                                         ReducedPermeabilityJacobian, REDUCED_N_PARAMS, reduced_basis)
    assert REDUCED_N_PARAMS == (1, 3, 6) and callable(reduced_basis)
    for cls_name, (methods, properties) in SURFACE.items():
        cls = getattr(interpolator, cls_name)
        for name, sig in methods.items():
            assert str(inspect.signature(getattr(cls, name))) == sig, (cls_name, name)
        for name in properties:
            assert isinstance(inspect.getattr_static(cls, name), property), (cls_name, name)
        if cls_name != "DevicePlan":       # nothing public beyond the table (scipy's own members of a LinearOperator aside)
            import scipy.sparse.linalg as spla
            public = {n for n in dir(cls) if not n.startswith("_")} - set(dir(spla.LinearOperator))
            assert public == set(methods) - {"__init__"} | set(properties), (cls_name, public)
        for name in methods:
            assert getattr(cls, name).__doc__ or name in ("__init__", "release"), (cls_name, name)


def test_a_released_jacobian_says_so():
    from ninpol_amd.interpolator import GlsJacobian, GlsReducedJacobian
    for cls, text, calls in ((GlsJacobian, "this GlsJacobian was released",
                              (lambda J: J.launch_jvp(8, 8), lambda J: J.launch_vjp(8, 8), lambda J: J.relinearize(8),
                               lambda J: J.stamp, lambda J: J.is_current(), lambda J: J.contrib_ptr, lambda J: J.fold_ptr)),
                             (GlsReducedJacobian, "this GlsReducedJacobian was released",
                              (lambda J: J.launch_jvp(8, 8), lambda J: J.launch_vjp(8, 8), lambda J: J.relinearize(8),
                               lambda J: J.stamp, lambda J: J.is_current(), lambda J: J.buffer_ptr))):
        J = cls.__new__(cls)               # (constructing one needs a device: a released object is one without its handle)
        J._h, J.plan, J.grid, J.n_params = None, None, None, 1
        for call in calls:
            with pytest.raises(ValueError) as e:
                call(J)
            assert str(e.value) == text
        J.release()                        # a second release is a no-op
        assert J._h is None
