"""CPU-side tests of the GLS adjoint's entry points (no GPU needed): the new symbols are declared, listed and exported; a host-only grid
is refused with NIN_ENODEVICE and bad arguments with NIN_EINVAL; DevicePlan.launch_weights_backward, Interpolator.permeability_gradient
and CellToNode validate their arguments before they touch a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from ninpol_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nin_gls_weights_backward_device", "nin_sddmm_device", "nin_gls_adjoint_plan", "nin_gls_permeability_gradient_host")


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
    Lb = lib.load()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert list(Lb.nin_gls_weights_backward_device.argtypes) == [vp, i32, vp, vp, vp, vp, vp]
    assert list(Lb.nin_sddmm_device.argtypes) == [vp, vp, vp, i32, vp, vp]
    assert list(Lb.nin_gls_adjoint_plan.argtypes) == [vp, vp]
    assert list(Lb.nin_gls_permeability_gradient_host.argtypes) == [vp, vp, vp, i32, vp]


def test_the_adjoint_unit_is_built():
    from ninpol_amd import build as nbuild
    assert "kernels_gls_adjoint.hip" in [u[0] for u in nbuild.UNITS]


def test_host_only_grid_is_enodevice(lib, host_interp):
    L, g = lib.load(), host_interp.grid
    nnz, E, P = np.zeros(g.nnz_esup), np.zeros(g.n_elems), np.zeros(g.n_points)
    K, counts = np.zeros(9 * g.n_elems), np.zeros(4, dtype=np.int64)
    _assert_code(L, L.nin_gls_weights_backward_device(g._h, 1, _p(nnz), None, _p(K), None, None), lib.NIN_ENODEVICE, "backward")
    _assert_code(L, L.nin_sddmm_device(g._h, _p(E), _p(P), 1, _p(nnz), None), lib.NIN_ENODEVICE, "sddmm")
    _assert_code(L, L.nin_gls_adjoint_plan(g._h, _p(counts)), lib.NIN_ENODEVICE, "plan")
    _assert_code(L, L.nin_gls_permeability_gradient_host(g._h, _p(P), _p(E), 1, _p(K)), lib.NIN_ENODEVICE, "host gradient")
    with pytest.raises(lib.NinpolError) as e:
        g.gls_adjoint_plan()
    assert e.value.code == lib.NIN_ENODEVICE


def test_null_arguments_and_field_counts_are_einval(lib, host_interp):
    L, g = lib.load(), host_interp.grid
    nnz, E, P = np.zeros(g.nnz_esup), np.zeros(g.n_elems), np.zeros(g.n_points)
    K, counts = np.zeros(9 * g.n_elems), np.zeros(4, dtype=np.int64)
    bad = {
        "backward, grid": lambda: L.nin_gls_weights_backward_device(None, 1, _p(nnz), None, _p(K), None, None),
        "backward, grad_csr": lambda: L.nin_gls_weights_backward_device(g._h, 1, None, None, _p(K), None, None),
        "backward, grad_perm": lambda: L.nin_gls_weights_backward_device(g._h, 1, _p(nnz), None, None, None, None),
        "sddmm, grid": lambda: L.nin_sddmm_device(None, _p(E), _p(P), 1, _p(nnz), None),
        "sddmm, u": lambda: L.nin_sddmm_device(g._h, None, _p(P), 1, _p(nnz), None),
        "sddmm, v": lambda: L.nin_sddmm_device(g._h, _p(E), None, 1, _p(nnz), None),
        "sddmm, grad": lambda: L.nin_sddmm_device(g._h, _p(E), _p(P), 1, None, None),
        "sddmm, k = 0": lambda: L.nin_sddmm_device(g._h, _p(E), _p(P), 0, _p(nnz), None),
        "plan, grid": lambda: L.nin_gls_adjoint_plan(None, _p(counts)),
        "plan, counts": lambda: L.nin_gls_adjoint_plan(g._h, None),
        "host gradient, grid": lambda: L.nin_gls_permeability_gradient_host(None, _p(P), _p(E), 1, _p(K)),
        "host gradient, v": lambda: L.nin_gls_permeability_gradient_host(g._h, None, _p(E), 1, _p(K)),
        "host gradient, u": lambda: L.nin_gls_permeability_gradient_host(g._h, _p(P), None, 1, _p(K)),
        "host gradient, out": lambda: L.nin_gls_permeability_gradient_host(g._h, _p(P), _p(E), 1, None),
        "host gradient, k = -1": lambda: L.nin_gls_permeability_gradient_host(g._h, _p(P), _p(E), -1, _p(K)),
    }
    for what, call in bad.items():
        _assert_code(L, call(), lib.NIN_EINVAL, what)


def test_permeability_gradient_validates_before_the_device(lib, host_interp):
    I = host_interp
    P, E = I.grid.n_points, I.grid.n_elems
    bad = [("u", np.zeros(E), None),                          # cell-sized, not node-sized
           ("u", np.zeros((2, P + 1)), None),
           ("u", np.zeros((0, P)), None),
           ("u", np.zeros((2, 2, P)), None),
           ("u", np.zeros(P), np.zeros(P)),                   # cell_values node-sized
           ("u", np.zeros((2, P)), np.zeros(E)),              # one cell field beside two node fields
           ("u", np.zeros(P), np.zeros((1, E))),
           ("nope", np.zeros(P), None)]
    for variable, v, u in bad:
        with pytest.raises(ValueError):
            I.permeability_gradient(variable, v, u)
        assert I.grid.device == -1, (variable, np.shape(v), np.shape(u))


def test_permeability_gradient_needs_a_mesh_and_a_permeability(lib):
    import ninpol_amd
    with pytest.raises(ValueError, match="Grid not initialized"):
        ninpol_amd.Interpolator().permeability_gradient("u", np.zeros(3))
    mesh = M.hex_mesh(2)
    mesh.cell_data = {"u": [np.zeros(len(b.data)) for b in mesh.cells]}
    mesh.point_data = {"neumann_flag_u": np.zeros(len(mesh.points)), "neumann_u": np.zeros(len(mesh.points))}
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    with pytest.raises(ValueError, match="permeability"):
        I.permeability_gradient("u", np.zeros(I.grid.n_points))


def test_the_python_surface():
    from ninpol_amd.grid import Grid
    from ninpol_amd.interpolator import DevicePlan
    sig = inspect.signature(DevicePlan.launch_weights_backward)
    assert list(sig.parameters) == ["self", "grad_csr_ptr", "grad_perm_ptr", "grad_diff_mag_ptr", "grad_neumann_ws_ptr", "stream", "add_neumann"]
    assert [sig.parameters[k].default for k in ("grad_diff_mag_ptr", "grad_neumann_ws_ptr", "stream", "add_neumann")] == [0, 0, 0, True]
    assert callable(DevicePlan.launch_sddmm) and callable(Grid.gls_adjoint_plan)
    assert Grid.ADJOINT_BINS == ("lds1", "lds2", "lds4", "global")
    # the forward plan table is what it was
    assert len(Grid.PLAN_KERNELS) == 22


def test_a_plan_of_another_method_is_refused_before_the_device():
    from ninpol_amd.interpolator import DevicePlan
    plan = DevicePlan.__new__(DevicePlan)      # (constructing one needs a device: the check comes first and needs none)
    plan.method = "idw"
    with pytest.raises(ValueError, match="GLS only"):
        plan.launch_weights_backward(8, 8)


def test_the_bins_of_the_model_are_the_headers():
    """tests/gls_adjoint_model.adjoint_bins restates csrc/gls_adjoint.hpp: the budgets and the slot formula are parsed from it"""
    import gls_adjoint_model as GM
    src = open(os.path.join(ROOT, "ninpol_amd", "csrc", "gls_adjoint.hpp")).read()
    budgets = tuple(int(x) for x in re.search(r"b == 0 \? (\d+) : b == 1 \? (\d+) : b == 2 \? (\d+) : 0", src).groups())
    assert budgets == inspect.signature(GM.adjoint_bins).parameters["budgets"].default
    assert "m * n + 3 * n + 2 * m + ((ne + 3 * nf + 1) >> 1)" in src
    import ninpol_amd
    mesh = M.attach_fields(M.delaunay_tet_mesh(6, seed=4, lattice="random"), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    counts, sizes = GM.adjoint_bins(I.grid)
    assert all(c > 0 for c in counts), counts           # every bin of the GPU test's mesh, without a switch
    assert sizes.max() > budgets[-1] and sum(counts) == I.grid.n_points
