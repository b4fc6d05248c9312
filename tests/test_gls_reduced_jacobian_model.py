"""The numpy model of the reduced GLS Jacobian (tests/gls_reduced_jacobian_model.py) pinned on the CPU: J_theta . dtheta
is the central difference of the ORACLE's node values W u + neumann_ws b along theta -- K +- h sum_m dtheta_m B_m, diff_mag recomputed
from the perturbed K -- at the bar of tests/test_gls_jacobian_model.py, for the three built-in bases and a random per-cell one on that
file's four meshes; and <v, J_theta dtheta> = <J_theta^T v, dtheta> through the model."""
import numpy as np
import pytest

import gls_adjoint_model as GM
import gls_jacobian_model as JM
import gls_reduced_jacobian_model as RM
from test_gls_adjoint_model import FD_RTOL, oracle_case, stored
from test_gls_jacobian_model import DUALITY_RTOL, H, MESHES

BASES = ("scale", "diagonal", "symmetric", "random3")


def basis_of(name, perm):
    if name == "random3":
        return np.random.default_rng(41).uniform(-1.0, 1.0, (len(perm), 3, 9))
    return RM.builtin_basis(name, perm)


@pytest.fixture(scope="module", params=sorted(MESHES))
def case(request, oracle_lib):
    o, perm, dmag, flag, rows = oracle_case(oracle_lib, MESHES[request.param])
    E, P = len(perm), o.grid.n_points
    rng = np.random.default_rng(29)
    c = {"name": request.param, "o": o, "perm": perm, "dmag": dmag, "flag": flag, "rows": rows,
         "u": rng.uniform(-1.0, 1.0, E), "b": rng.uniform(-1.0, 1.0, P), "v": rng.uniform(-1.0, 1.0, P)}
    c["full_vjp"] = JM.vjp_model(o.grid, perm, dmag, flag, c["u"], c["v"], b=c["b"])      # (does not depend on the basis)
    c["B"] = {name: basis_of(name, perm) for name in BASES}
    c["dtheta"] = {name: np.random.default_rng(5).uniform(-1.0, 1.0, c["B"][name].shape[:2]) for name in BASES}
    # A central difference is no derivative across a tie of eta = max(0, diff_mag_a, diff_mag_b).  To first order a step h |dtheta| <= h
    # moves diff_mag_e by at most reach_e = h |fold_e| sum_m |tr B_(e,m)|; on the two cells of a face whose diff_mags are closer than
    # twice the sum of their reaches (a handful of faces on the Delaunay mesh) the direction is zero.  The test still checks the step.
    fc = GM.face_cells(o.grid)
    fc = fc[fc[:, 1] >= 0]
    gap = np.abs(dmag[fc[:, 0]] - dmag[fc[:, 1]])
    for name in BASES:
        B = c["B"][name]
        reach = H * np.abs(GM.diff_mag_derivative(perm)) * np.abs(B[:, :, 0] + B[:, :, 4] + B[:, :, 8]).sum(axis=1)
        near = fc[gap < 2.0 * (reach[fc[:, 0]] + reach[fc[:, 1]])]
        assert len(np.unique(near)) <= E // 100
        c["dtheta"][name][np.unique(near)] = 0.0
    c["jvp"] = {name: RM.jvp_model(o.grid, perm, dmag, flag, c["u"], c["B"][name], c["dtheta"][name], b=c["b"]) for name in BASES}
    return c


def test_the_builtin_bases():
    perm = np.random.default_rng(1).uniform(1.0, 2.0, (4, 9))
    assert np.array_equal(RM.builtin_basis("scale", perm), perm.reshape(4, 1, 9))
    D, S = RM.builtin_basis("diagonal", perm), RM.builtin_basis("symmetric", perm)
    assert D.shape == (4, 3, 9) and S.shape == (4, 6, 9)
    th = np.arange(1.0, 7.0)
    K = RM.direction(S[:1], th[None])[0].reshape(3, 3)
    assert np.array_equal(K, np.array([[1.0, 4.0, 5.0], [4.0, 2.0, 6.0], [5.0, 6.0, 3.0]]))      # xx, yy, zz, xy, xz, yz
    assert np.array_equal(RM.direction(D[:1], th[None, :3])[0].reshape(3, 3), np.diag(th[:3]))
    assert np.array_equal(RM.per_cell(S[0], 4), S) and np.array_equal(RM.per_cell(S[0].reshape(6, 3, 3), 4), S)
    assert np.array_equal(RM.per_cell(S.reshape(4, 6, 3, 3), 4), S)


@pytest.mark.parametrize("basis", BASES)
def test_jvp_is_the_central_difference_of_the_oracle_along_theta(case, basis):
    o, perm, u, b = case["o"], case["perm"], case["u"], case["b"]
    perm_row, dmag_row = case["rows"]
    E = len(perm)
    dK = RM.direction(case["B"][basis], case["dtheta"][basis])
    esup = np.asarray(o.grid.esup).astype(np.int64)
    ptr = np.asarray(o.grid.esup_ptr).astype(np.int64)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
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
            d, nws = stored(o)
            got.append(np.bincount(rows, weights=d * u[esup], minlength=len(ptr) - 1) + nws * b)
    finally:
        o.cells_data[perm_row][:E * 9] = perm.reshape(-1)
        o.cells_data[dmag_row][:E] = case["dmag"]
    fd = (got[0] - got[1]) / (2 * H)
    want = case["jvp"][basis]["value"]
    top = np.abs(want).max()
    err = np.abs(fd - want).max() / top
    print(f"{case['name']} {basis}: max|FD - model| / max|J_theta dtheta| = {err:.2e}; max|J_theta dtheta| = {top:.3e}")
    assert top > 0 and err <= FD_RTOL


@pytest.mark.parametrize("basis", BASES)
def test_duality_through_the_model(case, basis):
    o, perm, dmag, flag = case["o"], case["perm"], case["dmag"], case["flag"]
    B, dth = case["B"][basis], case["dtheta"][basis]
    adj = RM.vjp_model(o.grid, perm, dmag, flag, case["u"], B, case["v"], b=case["b"], full=case["full_vjp"])
    assert adj["grad_theta"].shape == dth.shape == adj["scale"].shape
    lhs, rhs = case["v"] @ case["jvp"][basis]["value"], (adj["grad_theta"] * dth).sum()
    bar = np.abs(B * case["full_vjp"]["folded"][:, None, :] * dth[:, :, None]).sum()      # sum |terms|
    print(f"{case['name']} {basis}: duality gap {abs(lhs - rhs) / bar:.2e} of sum|terms| = {bar:.3e}")
    assert bar > 0 and abs(lhs - rhs) <= DUALITY_RTOL * bar


def test_the_model_is_not_vacuous(case):
    vals = [case["jvp"][name]["value"] for name in BASES]
    for a in range(len(BASES)):
        assert (case["jvp"][BASES[a]]["scale"] == 0).any() and np.abs(vals[a]).max() > 0
        for b in range(a):
            assert np.abs(vals[a] - vals[b]).max() > 1e-6 * np.abs(vals[a]).max()      # the bases really differ
    adj = RM.vjp_model(case["o"].grid, case["perm"], case["dmag"], case["flag"], case["u"], case["B"]["symmetric"], case["v"],
                       b=case["b"], full=case["full_vjp"])
    assert np.count_nonzero(case["full_vjp"]["grad_diff_mag"]) > 0 and (adj["scale"] > 0).any()
