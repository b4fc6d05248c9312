"""The readiness checks of the weight launches on a grid that IS on the device, in the order the C ABI keeps them -- flags set, method
known, GLS has a permeability -- through every entry point that runs them.  hex_mesh(3); every call here is refused, so no kernel is
launched.  The codes and texts are the ones the library gave before its host code was split into units."""
import ctypes

import numpy as np
import pytest

from ninpol_amd import mesh as M
import test_update_fields_host as UH

pytestmark = pytest.mark.gpu

lib = UH.lib
NO_FLAGS = "nin_fields_set has not been called"
NO_METHOD = "unknown method 7"
NO_PERM = "GLS needs permeability and diff_mag"
GLS, BAD = 0, 7

# entry point -> its arguments after the grid, given the method; "dev": a device buffer, "buf": a host buffer
WITH_METHOD = {
    "nin_weights_device": lambda m: (m, None, 0, 1, "dev", "dev", None),
    "nin_weights_dirty_device": lambda m: (m, 1, "dev", "dev", None, 1, "i64"),
    "nin_weights_host": lambda m: (m, None, 0, 1, "buf", "buf"),
    "nin_interpolate_csr_host": lambda m: (m, "buf", "buf", "buf", "i64", "buf"),
    "nin_apply_device": lambda m: (m, "dev", 1, "dev", "dev", None),
    "nin_apply_fields_host": lambda m: (m, "buf", 1, "buf", "buf"),
    "nin_apply_host": lambda m: (m, "buf", "buf", "buf"),
    "nin_apply_transpose_fields_host": lambda m: (m, "buf", 1, "buf"),
}
GLS_ONLY = {   # the adjoint: GLS by definition, so no method to be unknown
    "nin_gls_weights_backward_device": (1, "dev", "dev", "dev", "dev", None),
    "nin_gls_permeability_gradient_host": ("buf", "buf", 1, "buf"),
}


class OnDevice:
    def __init__(self, _lib, n):
        import torch
        self.lib, self.L = _lib, _lib.load()
        mesh = M.hex_mesh(n)
        M.attach_fields(mesh, "u", perm="LIN", neumann_plane=(2, 0.0), seed=5)
        self.I = UH.loaded(mesh)
        self.g = self.I.grid._h
        self.P = int(self.I.grid.n_points)
        assert self.L.nin_grid_to_device(self.g, 0) == 0, self.L.nin_last_error().decode()
        self.buf = np.zeros(1 << 16)
        self.dev = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
        self.i64 = ctypes.c_int64(0)

    def set_flags_only(self):
        flags = np.zeros(self.P)
        assert self.L.nin_fields_set(self.g, None, None, flags.ctypes.data_as(ctypes.c_void_p), None) == 0, self.L.nin_last_error().decode()

    def refused(self, name, spec, code, text, h=None):
        args = [self.buf.ctypes.data_as(ctypes.c_void_p) if a == "buf" else ctypes.c_void_p(self.dev.data_ptr()) if a == "dev" else
                ctypes.byref(self.i64) if a == "i64" else a for a in spec]
        rc = getattr(self.L, name)(self.g if h is None else h, *args)
        got = self.L.nin_last_error().decode()
        assert (rc, got) == (code, text), (name, rc, got)

    def all_refused(self, with_method, gls_only):
        """with_method: (method, code, text) for the entry points that take one; gls_only: (code, text) for the adjoint's, or None"""
        for name, spec in WITH_METHOD.items():
            self.refused(name, spec(with_method[0]), *with_method[1:])
        for name, spec in GLS_ONLY.items():
            if gls_only:
                self.refused(name, spec, *gls_only)
        assert not self.buf.any() and not self.dev.any().item()            # nothing was written


def test_readiness_checks_in_order(lib):
    E = lib
    d = OnDevice(lib, 3)
    assert d.P == 64 and d.L.nin_grid_device(d.g) == 0
    assert d.I.grid.gls_plan()["hex8"] == 8                                # cube nodes: nin_apply_device takes its fused path with GLS
    # a host matrix of a known method can be made before the fields are set; an unknown method is refused there already
    m, none = ctypes.c_void_p(), ctypes.c_void_p()
    assert d.L.nin_hostmatrix_create(d.g, GLS, ctypes.byref(m)) == 0 and m.value
    assert d.L.nin_hostmatrix_create(d.g, BAD, ctypes.byref(none)) == E.NIN_EINVAL and d.L.nin_last_error().decode() == NO_METHOD
    hm = {"nin_hostmatrix_update": (1, None, "i64", "i64", "i64"), "nin_hostmatrix_full": ("buf", "buf", "buf", "buf", "i64", None)}
    try:
        # freshly uploaded: the flags check comes first, whatever the method
        d.all_refused((GLS, E.NIN_ESTATE, NO_FLAGS), (E.NIN_ESTATE, NO_FLAGS))
        d.all_refused((BAD, E.NIN_ESTATE, NO_FLAGS), None)
        for name, spec in hm.items():
            d.refused(name, spec, E.NIN_ESTATE, NO_FLAGS, h=m)
        # flags set, no permeability
        d.set_flags_only()
        d.all_refused((BAD, E.NIN_EINVAL, NO_METHOD), None)
        d.all_refused((GLS, E.NIN_ESTATE, NO_PERM), (E.NIN_ESTATE, NO_PERM))
        for name, spec in hm.items():
            d.refused(name, spec, E.NIN_ESTATE, NO_PERM, h=m)
    finally:
        d.L.nin_hostmatrix_destroy(m)


def test_readiness_checks_of_the_pipelined_interpolate(lib, monkeypatch):
    """nin_interpolate_csr_host runs the checks itself when the grid's interpolate() is pipelined (>= 256 nodes, and NIN_E2E_MIN_NODES
    read when the grid goes to the device)"""
    monkeypatch.setenv("NIN_E2E_MIN_NODES", "256")
    d = OnDevice(lib, 6)
    assert d.P == 343
    name, spec = "nin_interpolate_csr_host", WITH_METHOD["nin_interpolate_csr_host"]
    d.refused(name, spec(GLS), lib.NIN_ESTATE, NO_FLAGS)
    d.refused(name, spec(BAD), lib.NIN_ESTATE, NO_FLAGS)
    d.set_flags_only()
    d.refused(name, spec(BAD), lib.NIN_EINVAL, NO_METHOD)
    d.refused(name, spec(GLS), lib.NIN_ESTATE, NO_PERM)
