"""What the status-returning entry points of the C ABI answer without a device: one table of 31 entry points, each called with a NULL
grid and with a host-only grid (hex_mesh(3) with fields, every other argument a valid non-NULL buffer), the return code and the text of
nin_last_error() pinned per entry.  nin_grid_to_device and nin_grid_create_on_device are left out: what they answer depends on whether
the machine has a GPU.  (The nin_hostmatrix_* calls take a matrix, which no host-only grid can make.)"""
import ctypes

import numpy as np
import pytest

from ninpol_amd import mesh as M
import test_update_fields_host as UH

lib = UH.lib

NOT_ON_DEVICE = "grid is not on a device"
FIRST = " (call nin_grid_to_device first)"
OR_UPDATE_POINTS = " (call nin_grid_to_device first, or nin_grid_update_points with a host array)"
OR_FIELDS_SET = " (call nin_grid_to_device first, or nin_fields_set with host arrays)"
OR_SCATTER_POINTS = " (call nin_grid_to_device first, or nin_grid_scatter_points with host arrays)"
WEIGHTS = ": the weight kernels are HIP only"
KERNELS = ": the kernels are HIP only"
BARE = ""
TAILS = (FIRST, OR_UPDATE_POINTS, OR_FIELDS_SET, OR_SCATTER_POINTS, WEIGHTS, KERNELS, BARE)

# (entry point, its arguments after the grid as names of the buffers below or plain integers, tail of the text on a host-only grid --
# None: the call succeeds)
TABLE = (
    ("nin_grid_update_points", ("xyz", 3), None),
    ("nin_grid_update_points_device", ("xyz", 3, None), OR_UPDATE_POINTS),
    ("nin_fields_set", ("buf", "buf", "buf", "buf"), FIRST),
    ("nin_fields_set_permeability_device", ("buf", "buf", None), OR_FIELDS_SET),
    ("nin_fields_get_permeability", ("buf", "buf"), FIRST),
    ("nin_weights_device", (0, None, 0, 0, "buf", "buf", None), WEIGHTS),
    ("nin_fields_scatter_permeability_device", ("ids", 1, 2, "buf", "buf", None), FIRST),
    ("nin_fields_set_flags_device", ("buf", 0, None), OR_FIELDS_SET),
    ("nin_fields_scatter_flags_device", ("ids", 1, 2, "buf", 0, None), FIRST),
    ("nin_fields_get_flags", ("buf",), FIRST),
    ("nin_grid_scatter_points_device", ("ids", 1, 2, "xyz", 3, None), OR_SCATTER_POINTS),
    ("nin_grid_scatter_points", ("ids", 2, "xyz", 3), None),
    ("nin_weights_dirty_device", (0, 1, "buf", "buf", None, 1, "i64"), WEIGHTS),
    ("nin_grid_dirty_reset", (0, None), FIRST),
    ("nin_weights_host", (0, None, 0, 0, "buf", "buf"), WEIGHTS),
    ("nin_csr_compact_host", ("buf", "buf", "buf", "buf", "i64", None), BARE),
    ("nin_interpolate_csr_host", (0, "buf", "buf", "buf", "i64", "buf"), WEIGHTS),
    ("nin_hostmatrix_create", (0, "vp"), FIRST),
    ("nin_grid_release_scratch", (), None),
    ("nin_apply_device", (0, "buf", 1, "buf", "buf", None), WEIGHTS),
    ("nin_apply_fields_host", (0, "buf", 1, "buf", "buf"), WEIGHTS),
    ("nin_apply_host", (0, "buf", "buf", "buf"), WEIGHTS),
    ("nin_spmv_device", ("buf", "buf", 1, "buf", None), KERNELS),
    ("nin_spmv_transpose_device", ("buf", "buf", 1, "buf", None), KERNELS),
    ("nin_apply_transpose_fields_host", (0, "buf", 1, "buf"), WEIGHTS),
    ("nin_gls_plan_flops", ("buf", "buf", "buf"), FIRST),
    ("nin_gls_weights_backward_device", (1, "buf", "buf", "buf", "buf", None), KERNELS),
    ("nin_sddmm_device", ("buf", "buf", 1, "buf", None), KERNELS),
    ("nin_gls_permeability_gradient_host", ("buf", "buf", 1, "buf"), KERNELS),
    ("nin_gls_adjoint_plan", ("buf",), FIRST),
    ("nin_gls_plan", ("buf",), FIRST),
)
GETTERS = (("nin_grid_device", -1), ("nin_grid_geometry_updates", 0), ("nin_grid_has_transpose_index", 0), ("nin_grid_field_updates", 0),
           ("nin_grid_flag_updates", 0), ("nin_grid_dirty_nodes", 0))


class Host:
    """the host-only grid and the buffers the calls are given"""

    def __init__(self, _lib):
        self.L = _lib.load()
        mesh = M.hex_mesh(3)
        M.attach_fields(mesh, "u", perm="LIN", neumann_plane=(2, 0.0), seed=5)
        self.I = UH.loaded(mesh)
        self.g = self.I.grid._h
        P = int(self.I.grid.n_points)
        assert P == 64
        self.xyz = np.zeros(P * 3)                                   # the grid's own coordinates: the two calls that succeed move nothing
        assert self.L.nin_grid_array_copy(self.g, b"point_coords", self.xyz.ctypes.data_as(ctypes.c_void_p), P * 3) == 0
        self.coords = self.xyz.copy()
        self.ids = np.array([0, 1], dtype=np.int64)
        self.buf = np.zeros(1 << 16)                                 # room for any output of a 64-node mesh
        self.i64 = ctypes.c_int64(0)
        self.vp = ctypes.c_void_p(None)

    def args(self, spec):
        out = []
        for a in spec:
            if a in ("xyz", "ids", "buf"):
                out.append(getattr(self, a).ctypes.data_as(ctypes.c_void_p))
            elif a in ("i64", "vp"):
                out.append(ctypes.byref(getattr(self, a)))
            else:
                out.append(a)
        return out

    def call(self, name, g, spec):
        rc = getattr(self.L, name)(g, *self.args(spec))
        return rc, self.L.nin_last_error().decode()


@pytest.fixture(scope="module")
def host(lib):
    return Host(lib)


def test_the_table_is_the_one_the_contract_names():
    names = [t[0] for t in TABLE]
    assert len(names) == 31 and len(set(names)) == 31
    assert sum(t[2] is None for t in TABLE) == 3 and sum(t[2] is not None for t in TABLE) == 28
    assert {t[2] for t in TABLE if t[2] is not None} == set(TAILS) and len(set(TAILS)) == 7
    assert not {"nin_grid_to_device", "nin_grid_create_on_device"} & set(names)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_null_grid(lib, host, name, spec, tail):
    assert name in lib.EXPORTS
    rc, text = host.call(name, None, spec)
    assert rc == lib.NIN_EINVAL, (name, rc, text)
    assert text.startswith("NULL"), (name, text)


@pytest.mark.parametrize("name,spec,tail", TABLE, ids=[t[0] for t in TABLE])
def test_host_only_grid(lib, host, name, spec, tail):
    rc, text = host.call(name, host.g, spec)
    if tail is None:
        assert rc == lib.NIN_OK, (name, rc, text)
        return
    assert rc == lib.NIN_ENODEVICE, (name, rc, text)
    assert text == NOT_ON_DEVICE + tail, (name, text)


def test_getters_and_what_the_calls_left_behind(lib, host):
    # (after the table above in file order; on its own the assertions hold as well)
    for name, spec, tail in TABLE:
        host.call(name, host.g, spec)
    for name, value in GETTERS:
        assert getattr(host.L, name)(None) == value, name
        assert getattr(host.L, name)(host.g) == value, name
    assert not host.buf.any() and host.i64.value == 0 and host.vp.value is None      # a refused call wrote nothing
    assert np.array_equal(host.xyz, host.coords)
    back = np.zeros_like(host.coords)
    assert host.L.nin_grid_array_copy(host.g, b"point_coords", back.ctypes.data_as(ctypes.c_void_p), back.size) == 0
    assert np.array_equal(back, host.coords)                                          # the two successful calls moved nothing
