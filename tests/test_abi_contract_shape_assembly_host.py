"""The entry points of the assembled GLS Jacobian in the node coordinates (nin_gls_xjacobian_pattern, _pattern_copy, _assemble,
_pattern_host, _assemble_host), without a device: what the library declares, lists and builds for them, the NULL rows
in the form tests/test_abi_contract_shape_jacobian_host.py keeps for their siblings, and the Python surface by inspection.  An object
exists only for a grid on a device, so every entry point is given the NULL object."""
import ctypes
import inspect
import os
import re

import pytest

import test_abi_contract_host as C
import test_update_fields_host as UH

lib = UH.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("nin_gls_xjacobian_pattern", "nin_gls_xjacobian_pattern_copy", "nin_gls_xjacobian_assemble", "nin_gls_xjacobian_pattern_host",
               "nin_gls_xjacobian_assemble_host")
# (entry point, its arguments after the object): every one refuses the NULL object
OBJECT_CALLS = (
    ("nin_gls_xjacobian_pattern", ("i64", "vp", "vp", None)),
    ("nin_gls_xjacobian_pattern_copy", ("buf", "buf", None)),
    ("nin_gls_xjacobian_assemble", ("buf", None)),
    ("nin_gls_xjacobian_pattern_host", ("buf", "buf", "i64")),
    ("nin_gls_xjacobian_assemble_host", ("buf",)),
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
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in ninpol_amd.h"
        assert hasattr(L, name), f"{name} is not exported by the library"
    vp, pvp, pi64 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)
    assert list(L.nin_gls_xjacobian_pattern.argtypes) == [vp, pi64, pvp, pvp, vp]
    assert list(L.nin_gls_xjacobian_pattern_copy.argtypes) == [vp, vp, vp, vp]
    assert list(L.nin_gls_xjacobian_assemble.argtypes) == [vp, vp, vp]
    assert list(L.nin_gls_xjacobian_pattern_host.argtypes) == [vp, vp, vp, pi64]
    assert list(L.nin_gls_xjacobian_assemble_host.argtypes) == [vp, vp]
    # the C types of the declarations: int64 row pointers, int32 columns
    assert re.search(r"nin_gls_xjacobian_pattern\s*\(\s*nin_gls_xjacobian\s*\*J,\s*int64_t\s*\*n_blocks,\s*const\s+int64_t\s*\*\*dev_block_ptr,\s*"
                     r"const\s+int32_t\s*\*\*dev_block_col,\s*void\s*\*stream\)", header)
    assert re.search(r"nin_gls_xjacobian_pattern_host\s*\(\s*nin_gls_xjacobian\s*\*J,\s*int64_t\s*\*block_ptr,\s*int32_t\s*\*block_col,\s*"
                     r"int64_t\s*\*n_blocks\)", header)
    from ninpol_amd import build as nbuild
    units = {u[0]: u for u in nbuild.UNITS}
    assert units["kernels_gls_shape_assemble.hip"][1:] == ("hipcc", [])         # no extra flags, like its sibling
    assert units["kernels_gls_shape_jacobian.hip"][1:] == ("hipcc", [])
    assert os.path.exists(os.path.join(ROOT, "ninpol_amd", "csrc", "kernels_gls_shape_assemble.hip"))


@pytest.mark.parametrize("name,spec", OBJECT_CALLS, ids=[t[0] for t in OBJECT_CALLS])
def test_null_object(lib, host, name, spec):
    host.i64.value, host.vp.value = 0, None
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)
    assert not host.buf.any() and host.vp.value is None and host.i64.value == 0       # nothing was written


def test_null_outputs_and_the_siblings_words(lib, host):
    """a NULL output beside a non-NULL (never dereferenced) object is refused before the object is looked at; _pattern and _assemble on
    the NULL object answer in the words of nin_gls_xjacobian_records and nin_gls_xjacobian_apply"""
    L = host.L
    b = host.buf.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0xdead0)          # (an address no call may follow: every call below is refused on its NULL pointer first)
    n, p1, p2 = ctypes.c_int64(0), ctypes.c_void_p(None), ctypes.c_void_p(None)
    calls = (
        lambda: L.nin_gls_xjacobian_pattern(fake, None, ctypes.byref(p1), ctypes.byref(p2), None),
        lambda: L.nin_gls_xjacobian_pattern(fake, ctypes.byref(n), None, ctypes.byref(p2), None),
        lambda: L.nin_gls_xjacobian_pattern(fake, ctypes.byref(n), ctypes.byref(p1), None, None),
        lambda: L.nin_gls_xjacobian_pattern_copy(fake, None, b, None),
        lambda: L.nin_gls_xjacobian_pattern_copy(fake, b, None, None),
        lambda: L.nin_gls_xjacobian_pattern_host(fake, None, b, ctypes.byref(n)),
        lambda: L.nin_gls_xjacobian_pattern_host(fake, b, b, None),
        lambda: L.nin_gls_xjacobian_assemble(fake, None, None),
        lambda: L.nin_gls_xjacobian_assemble_host(fake, None),
    )
    for i, call in enumerate(calls):
        rc, text = call(), L.nin_last_error().decode()
        assert rc == lib.NIN_EINVAL and text.startswith("NULL"), (i, rc, text)
    assert n.value == 0 and p1.value is None and p2.value is None and not host.buf.any()
    for call, sibling in ((lambda: L.nin_gls_xjacobian_pattern(None, ctypes.byref(n), ctypes.byref(p1), ctypes.byref(p2), None),
                           lambda: L.nin_gls_xjacobian_records(None, ctypes.byref(p1), ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(n))),
                          (lambda: L.nin_gls_xjacobian_assemble(None, b, None), lambda: L.nin_gls_xjacobian_apply(None, 1, b, b, None)),
                          (lambda: L.nin_gls_xjacobian_assemble_host(None, b), lambda: L.nin_gls_xjacobian_apply_host(None, 1, b, b))):
        rc, text = call(), L.nin_last_error().decode()
        rc_s, text_s = sibling(), L.nin_last_error().decode()
        assert rc == rc_s == lib.NIN_EINVAL and text == text_s, (rc, text, rc_s, text_s)
    assert L.nin_grid_device(host.g) == -1 and not host.buf.any()


def test_python_surface_without_a_device():
    import scipy.sparse.linalg as spla
    from ninpol_amd.interpolator import GlsShapeJacobian, Interpolator, PointsJacobian
    from ninpol_amd.torch_ops import Linearization
    assert list(inspect.signature(GlsShapeJacobian.pattern).parameters) == ["self", "stream"]
    assert inspect.signature(GlsShapeJacobian.pattern).parameters["stream"].default == 0
    assert list(inspect.signature(GlsShapeJacobian.fetch_pattern).parameters) == ["self"]
    sig = inspect.signature(GlsShapeJacobian.launch_assemble)
    assert list(sig.parameters) == ["self", "values_ptr", "stream"] and sig.parameters["stream"].default == 0
    sig = inspect.signature(GlsShapeJacobian.launch_pattern_copy)
    assert list(sig.parameters) == ["self", "block_ptr_ptr", "block_col_ptr", "stream"] and sig.parameters["stream"].default == 0
    assert list(inspect.signature(GlsShapeJacobian.fetch_assembled).parameters) == ["self"]
    assert list(inspect.signature(PointsJacobian.assemble).parameters) == ["self"] and "assemble" in vars(PointsJacobian)
    assert issubclass(PointsJacobian, spla.LinearOperator) and not hasattr(PointsJacobian, "to_scipy")
    # the docstrings name to_scipy, say why this one differs, and no longer say "never assembled"
    for doc in (PointsJacobian.__doc__, Interpolator.points_jacobian.__doc__):
        assert "to_scipy" in doc and "assemble()" in doc and "never assembled" not in doc
    assert list(inspect.signature(Linearization.assemble).parameters) == ["self"]
    lin = Linearization.__new__(Linearization)       # (constructing one needs a device: the check comes first and needs none)
    for wrt in ("K", "scale"):
        lin.wrt = wrt
        with pytest.raises(ValueError, match='wrt="points"'):
            lin.assemble()
