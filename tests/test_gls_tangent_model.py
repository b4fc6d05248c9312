"""The numpy model of the GLS tangent (tests/gls_tangent_model.py) pinned on the CPU: along a direction dK its tangent is the central
difference of the ORACLE's stored weights and neumann_ws at K +- h dK (diff_mag recomputed from the perturbed K, so the chain through
eta is in it), and it is dual to the adjoint model of tests/gls_adjoint_model.py.  The meshes, the ALH permeability and the Neumann
plane are those of tests/test_gls_adjoint_model.py; every step is checked not to cross a tie of eta = max(0, diff_mag_a, diff_mag_b).

Also here, because they need no GPU: the two new entry points of the C ABI answer a grid that is not on a device as their backward
siblings do."""
import ctypes

import numpy as np
import pytest

import gls_adjoint_model as GM
import gls_tangent_model as TM
from test_gls_adjoint_model import FD_RTOL, MESHES, oracle_case, stored
from ninpol_amd import mesh as M

H = 1e-5              # the central-difference step
DUALITY_RTOL = 1e-12  # of sum |fold(Kbar, etabar) . dK|: both models solve with lstsq; measured 5e-16 to 4.6e-15


@pytest.fixture(scope="module", params=sorted(MESHES))
def case(request, oracle_lib):
    make, _ = MESHES[request.param]
    o, perm, dmag, flag, rows = oracle_case(oracle_lib, make)
    dK = np.random.default_rng(1).uniform(-1, 1, (len(perm), 9))
    model = TM.gls_tangent_model(o.grid, perm, dmag, flag, dK)
    return {"name": request.param, "o": o, "perm": perm, "dmag": dmag, "flag": flag, "rows": rows, "dK": dK, "model": model}


def test_tangent_is_the_central_difference_of_the_oracle(case):
    o, perm, dK, m = case["o"], case["perm"], case["dK"], case["model"]
    perm_row, dmag_row = case["rows"]
    E = len(perm)
    fc = GM.face_cells(o.grid)
    fc = fc[fc[:, 1] >= 0]
    side = np.sign(case["dmag"][fc[:, 0]] - case["dmag"][fc[:, 1]])
    got = []
    try:
        for sgn in (+1, -1):
            K = perm + sgn * H * dK
            dm = GM.diff_mag_of(K)
            assert np.array_equal(np.sign(dm[fc[:, 0]] - dm[fc[:, 1]]), side), "the step crosses a max() tie"
            assert np.array_equal(dm > 0, case["dmag"] > 0)
            o.cells_data[perm_row][:E * 9] = K.reshape(-1)
            o.cells_data[dmag_row][:E] = dm
            got.append(stored(o))
    finally:
        o.cells_data[perm_row][:E * 9] = perm.reshape(-1)
        o.cells_data[dmag_row][:E] = case["dmag"]
    fd_w = (got[0][0] - got[1][0]) / (2 * H)
    fd_n = (got[0][1] - got[1][1]) / (2 * H)
    scale = np.abs(m["tangent"]).max()
    e_w = np.abs(fd_w - m["tangent"]).max() / scale
    e_n = np.abs(fd_n - m["tangent_neumann_ws"]).max() / scale
    print(f"{case['name']}: max|FD - model| / max|model| = {e_w:.2e} (weights), {e_n:.2e} (neumann_ws); max|dW| = {scale:.3e}")
    assert scale > 0 and e_w <= FD_RTOL and e_n <= FD_RTOL


def test_duality_with_the_adjoint_model(case):
    o, perm, dK, m = case["o"], case["perm"], case["dK"], case["model"]
    rng = np.random.default_rng(17)
    ghat = rng.uniform(-1.0, 1.0, len(o.grid.esup))
    gnws = rng.uniform(-1.0, 1.0, o.grid.n_points)
    adj = GM.gls_adjoint_model(o.grid, perm, case["dmag"], case["flag"], ghat, add_neumann=True, grad_neumann_ws=gnws)
    kbar = GM.fold(adj["grad_perm"], adj["grad_diff_mag"], perm)
    lhs = ghat @ m["tangent"] + gnws @ m["tangent_neumann_ws"]
    rhs = (kbar * dK).sum()
    bar = np.abs(kbar * dK).sum()
    print(f"{case['name']}: duality gap {abs(lhs - rhs) / bar:.2e} of sum|Kbar . dK| = {bar:.3e}")
    assert bar > 0 and abs(lhs - rhs) <= DUALITY_RTOL * bar
    # unfolded: diff_mag an input of its own
    ddm = np.random.default_rng(2).uniform(-1, 1, len(perm))
    mu = TM.gls_tangent_model(o.grid, perm, case["dmag"], case["flag"], dK, ddm=ddm)
    lhs = ghat @ mu["tangent"] + gnws @ mu["tangent_neumann_ws"]
    rhs = (adj["grad_perm"] * dK).sum() + adj["grad_diff_mag"] @ ddm
    bar = np.abs(adj["grad_perm"] * dK).sum() + np.abs(adj["grad_diff_mag"] * ddm).sum()
    print(f"{case['name']}: unfolded duality gap {abs(lhs - rhs) / bar:.2e}")
    assert abs(lhs - rhs) <= DUALITY_RTOL * bar


def test_the_model_is_not_vacuous(case):
    o, perm, dK, m = case["o"], case["perm"], case["dK"], case["model"]
    ptr = np.asarray(o.grid.esup_ptr)
    assert np.count_nonzero(m["tangent_neumann_ws"]) > 0
    zero_rows = [p for p in range(len(ptr) - 1) if ptr[p + 1] > ptr[p] and not m["tangent"][ptr[p]:ptr[p + 1]].any()]
    assert zero_rows and not m["computed"][zero_rows].any() and not m["scale"][zero_rows].any()
    assert np.all(m["scale"][m["computed"]] > 0)
    # the eta chain matters
    flat = TM.gls_tangent_model(o.grid, perm, case["dmag"], case["flag"], dK, ddm=np.zeros(len(perm)))
    assert np.abs(flat["tangent"] - m["tangent"]).max() > 1e-6 * np.abs(m["tangent"]).max()
    # the unfolded form with the folded direction given explicitly is the folded form
    explicit = TM.gls_tangent_model(o.grid, perm, case["dmag"], case["flag"], dK, ddm=TM.fold_direction(perm, dK))
    assert np.array_equal(explicit["tangent"], m["tangent"]) and np.array_equal(explicit["tangent_neumann_ws"], m["tangent_neumann_ws"])
    # add_neumann = False: the rows of the Neumann nodes lose dnws
    plain = TM.gls_tangent_model(o.grid, perm, case["dmag"], case["flag"], dK, add_neumann=False)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    assert np.allclose(plain["tangent"] + m["tangent_neumann_ws"][rows], m["tangent"], rtol=0, atol=1e-13 * np.abs(m["tangent"]).max())


def test_error_codes_are_the_backward_siblings():
    """a grid that is not on a device: NIN_ENODEVICE from both, as from the backward calls; argument errors come first"""
    import ninpol_amd
    from ninpol_amd import _lib
    from ninpol_amd import build as nbuild
    nbuild.build()
    L = _lib.load()
    mesh = M.attach_fields(M.hex_mesh(2), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    h = I.grid._h
    assert I.grid.device < 0
    buf = (ctypes.c_double * 8)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    back = L.nin_gls_weights_backward_device(h, 1, a, None, a, None, None)
    assert back == _lib.NIN_ENODEVICE
    assert L.nin_gls_weights_tangent_device(h, 1, 1, a, None, a, None, None) == back
    assert "not on a device" in L.nin_last_error().decode()
    assert L.nin_gls_permeability_tangent_host(h, a, a, 1, a, a) == L.nin_gls_permeability_gradient_host(h, a, a, 1, a) == back
    for args in ((None, 1, 1, a, None, a, None, None), (h, 1, 1, None, None, a, None, None), (h, 1, 1, a, None, None, None, None),
                 (h, 1, 0, a, None, a, None, None)):
        assert L.nin_gls_weights_tangent_device(*args) == _lib.NIN_EINVAL
    for args in ((None, a, a, 1, a, a), (h, None, a, 1, a, a), (h, a, None, 1, a, a), (h, a, a, 1, None, a), (h, a, a, 1, a, None),
                 (h, a, a, 0, a, a)):
        assert L.nin_gls_permeability_tangent_host(*args) == _lib.NIN_EINVAL
    assert I.grid._scalar("gls_adjoint_contrib_bytes") == 0
