"""The entry points of the dirty relinearisation of the kept GLS Jacobians (nin_gls_*jacobian_linearize_dirty*, nin_grid_mark_dirty_device,
DESIGN.md 4.20), without a device: what the library declares, lists and builds for them, and the rows tests/test_abi_contract_host.py
keeps for every status-returning entry point -- NULL arguments, a host-only grid.  An object exists only for a grid on a device, so
every entry point that takes an object is given the NULL one; the one call that takes the grid is nin_grid_mark_dirty_device."""
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

NEW_SYMBOLS = ("nin_gls_jacobian_linearize_dirty", "nin_gls_rjacobian_linearize_dirty", "nin_gls_xjacobian_linearize_dirty",
               "nin_gls_jacobian_linearize_dirty_host", "nin_gls_rjacobian_linearize_dirty_host", "nin_gls_xjacobian_linearize_dirty_host",
               "nin_grid_mark_dirty_device")
# (entry point, its arguments after the grid, tail of the text on a host-only grid): the form of test_abi_contract_host.TABLE
TABLE = (
    ("nin_grid_mark_dirty_device", ("ids", 1, 2, 0, None), C.FIRST),
    ("nin_grid_mark_dirty_device", ("ids", 1, 2, 1, None), C.FIRST),
)
# (entry point, its arguments after the object): every one refuses the NULL object, and a NULL u
OBJECT_CALLS = (
    ("nin_gls_jacobian_linearize_dirty", ("buf", "buf", None, 1, "i64")),
    ("nin_gls_rjacobian_linearize_dirty", ("buf", "buf", "buf", 1, None, 1, "i64")),
    ("nin_gls_xjacobian_linearize_dirty", ("buf", "buf", None, 1, "i64")),
    ("nin_gls_jacobian_linearize_dirty_host", ("buf", "buf", 1, "i64")),
    ("nin_gls_rjacobian_linearize_dirty_host", ("buf", "buf", "buf", 1, 1, "i64")),
    ("nin_gls_xjacobian_linearize_dirty_host", ("buf", "buf", 1, "i64")),
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
    vp, i32, i64, pi64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    assert list(L.nin_gls_jacobian_linearize_dirty.argtypes) == [vp, vp, vp, vp, i32, pi64]
    assert list(L.nin_gls_rjacobian_linearize_dirty.argtypes) == [vp, vp, vp, vp, i32, vp, i32, pi64]
    assert list(L.nin_gls_xjacobian_linearize_dirty.argtypes) == [vp, vp, vp, vp, i32, pi64]
    assert list(L.nin_gls_jacobian_linearize_dirty_host.argtypes) == [vp, vp, vp, i32, pi64]
    assert list(L.nin_gls_rjacobian_linearize_dirty_host.argtypes) == [vp, vp, vp, vp, i32, i32, pi64]
    assert list(L.nin_gls_xjacobian_linearize_dirty_host.argtypes) == [vp, vp, vp, i32, pi64]
    assert list(L.nin_grid_mark_dirty_device.argtypes) == [vp, vp, i32, i64, i32, vp]
    from ninpol_amd import build as nbuild
    units = {u[0]: u for u in nbuild.UNITS}
    assert units["jacobian_dirty.hip"][1:] == ("hipcc", [])                    # no extra flags
    assert "abi_jacobian_dirty.hip" in units
    # the adjoint kernel's unit is the one the earlier derivative pull requests built: the new code is not in it
    src = open(os.path.join(ROOT, "ninpol_amd", "csrc", "kernels_gls_adjoint.hip")).read()
    assert "dirty" not in src


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=["nodes", "cells"])
def test_null_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=["nodes", "cells"])
def test_host_only_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, host.g, spec)
    assert rc == lib.NIN_ENODEVICE, (name, rc, text)
    assert text == C.NOT_ON_DEVICE + tail, (name, text)
    assert host.L.nin_grid_device(host.g) == -1 and host.L.nin_grid_dirty_nodes(host.g) == 0
    # a negative count is refused before the device is asked for, in the words of the scatters
    rc, text = host.call(name, host.g, (spec[0], spec[1], -1) + spec[3:])
    rc_s, text_s = host.call("nin_fields_scatter_flags_device", host.g, ("ids", 1, -1, "buf", 0, None))
    assert rc == rc_s == lib.NIN_EINVAL and text == text_s == "negative n", (rc, text, rc_s, text_s)


@pytest.mark.parametrize("name,spec", OBJECT_CALLS, ids=[t[0] for t in OBJECT_CALLS])
def test_null_object(lib, host, name, spec):
    host.i64.value = 77
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)
    assert not host.buf.any() and host.i64.value == 0                         # *n_rows is zeroed, nothing else is written


def test_python_surface_without_a_device(lib):
    from ninpol_amd.grid import Grid
    from ninpol_amd.interpolator import (DevicePlan, GlsDirtyJacobian, GlsDirtyReducedJacobian, GlsJacobian, GlsReducedJacobian,
                                         GlsShapeJacobian, Interpolator, PermeabilityJacobian, PointsJacobian, ReducedPermeabilityJacobian,
                                         UpdatablePermeabilityJacobian, UpdatableReducedPermeabilityJacobian)
    # the public names of GlsJacobian, GlsReducedJacobian and the two permeability operators are a closed set that
    # tests/test_abi_contract_derivative_host.py pins: what DevicePlan.linearize*() and Interpolator.permeability_jacobian() return are
    # subclasses that add the one new method each; the shape classes are open and carry theirs themselves
    assert issubclass(GlsDirtyJacobian, GlsJacobian) and issubclass(GlsDirtyReducedJacobian, GlsReducedJacobian)
    assert issubclass(UpdatablePermeabilityJacobian, PermeabilityJacobian)
    assert issubclass(UpdatableReducedPermeabilityJacobian, ReducedPermeabilityJacobian)
    for cls, new in ((GlsDirtyJacobian, "relinearize_dirty"), (GlsDirtyReducedJacobian, "relinearize_dirty"),
                     (UpdatablePermeabilityJacobian, "update"), (UpdatableReducedPermeabilityJacobian, "update")):
        base = cls.__mro__[-3] if new == "relinearize_dirty" else [b for b in cls.__mro__ if b.__name__.endswith("PermeabilityJacobian")][1]
        assert {n for n in dir(cls) if not n.startswith("_")} - {n for n in dir(base) if not n.startswith("_")} == {new}, cls
        assert getattr(cls, new).__doc__ and cls.__doc__
    for name in ("GlsDirtyJacobian", "GlsDirtyReducedJacobian"):
        assert name in inspect.getsource(DevicePlan)                      # (constructing one needs a device)
    for name in ("UpdatablePermeabilityJacobian", "UpdatableReducedPermeabilityJacobian"):
        assert name in inspect.getsource(Interpolator.permeability_jacobian)
    for cls in (GlsDirtyJacobian, GlsShapeJacobian):
        sig = inspect.signature(cls.relinearize_dirty)
        assert list(sig.parameters) == list(inspect.signature(cls.relinearize).parameters) + ["clear"]
        assert sig.parameters["clear"].default is True
    sig = inspect.signature(GlsDirtyReducedJacobian.relinearize_dirty)
    assert list(sig.parameters) == list(inspect.signature(GlsReducedJacobian.relinearize).parameters) + ["clear"]
    assert sig.parameters["clear"].default is True and sig.parameters["basis_per_cell"].default is True
    for cls in (UpdatablePermeabilityJacobian, UpdatableReducedPermeabilityJacobian, PointsJacobian):
        sig = inspect.signature(cls.update)
        assert list(sig.parameters) == ["self", "cell_values", "neumann_values", "clear"]
        assert [p.default for p in list(sig.parameters.values())[1:]] == [None, None, True]
    sig = inspect.signature(Grid.mark_dirty)
    assert list(sig.parameters) == ["self", "cells", "nodes", "stream"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, None, 0]
    # the argument checks that need no device come first; a host-only grid is then refused in the library's words
    g = C.Host(lib).I.grid
    for kw in ({}, {"cells": [0], "nodes": [0]}):
        with pytest.raises(ValueError, match="exactly one of cells= and nodes="):
            g.mark_dirty(**kw)
    with pytest.raises(lib.NinpolError) as e:
        g.mark_dirty(nodes=np.array([0, 1]))
    assert e.value.code == lib.NIN_ENODEVICE and g.device == -1
    # an operator that no Interpolator made has nothing to update from
    op = UpdatablePermeabilityJacobian.__new__(UpdatablePermeabilityJacobian)
    with pytest.raises(ValueError, match="update\\(\\) needs an operator made by"):
        op.update()
