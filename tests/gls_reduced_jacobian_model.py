"""A numpy model of the GLS Jacobian in a reduced parametrisation of the permeability: glue over
tests/gls_jacobian_model.py, which stays as it is.

The permeability moves along M parameters per cell, perm_e = sum_m theta_(e,m) B_(e,m), B [E][M][9] row-major like perm.
  J_theta . dtheta  = J . dK with dK_e = sum_m dtheta_(e,m) B_(e,m): jvp_model of the full Jacobian, folded, its row scale unchanged
  J_theta^T . v     = <B_(e,m), (J^T v)_e> with the folded (J^T v): `grad_theta` [E][M], and `scale` [E][M] = sum_k |B_(e,m)[k]| times the
                      folded cell scale of tests/test_gpu_gls_jacobian.py (scale_perm + scale_diff_mag |d diff_mag / d K_dd|)

Not a test module (no test_ prefix): tests/test_gls_reduced_jacobian_model.py pins it on the CPU, tests/test_gpu_gls_reduced_jacobian.py
holds the device kernels to it."""
import numpy as np

import gls_adjoint_model as GM
import gls_jacobian_model as JM

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # "symmetric": xx, yy, zz, xy, xz, yz


def builtin_basis(name, perm):
    """the three built-in bases as [E][M][9]: "scale" (the permeability itself, M = 1), "diagonal" (e_d e_d^T, M = 3), "symmetric"
    (xx, yy, zz, then e_i e_j^T + e_j e_i^T for xy, xz, yz, M = 6)"""
    perm = np.asarray(perm, dtype=float).reshape(-1, 9)
    E = len(perm)
    if name == "scale":
        return perm.reshape(E, 1, 9).copy()
    if name == "diagonal":
        B = np.zeros((3, 3, 3))
        for d in range(3):
            B[d, d, d] = 1.0
    elif name == "symmetric":
        B = np.zeros((6, 3, 3))
        for m, (i, j) in enumerate(PAIRS):
            B[m, i, j] = B[m, j, i] = 1.0
    else:
        raise ValueError(name)
    return np.ascontiguousarray(np.broadcast_to(B.reshape(1, -1, 9), (E, len(B), 9)))


def per_cell(B, E):
    """a basis [E][M][9] from [E][M][9], [E][M][3][3], [M][9] or [M][3][3]"""
    B = np.asarray(B, dtype=float)
    if B.ndim >= 3 and B.shape[0] == E and B.shape[2:] in ((9,), (3, 3)):
        return B.reshape(E, B.shape[1], 9)
    return np.broadcast_to(B.reshape(1, B.shape[0], 9), (E, B.shape[0], 9))


def direction(B, dtheta):
    """dK [E][9] = sum_m dtheta[e][m] B[e][m]"""
    return np.einsum("emk,em->ek", B, np.asarray(dtheta, dtype=float).reshape(B.shape[:2]))


def jvp_model(grid, perm, diff_mag, neumann_flag, u, B, dtheta, b=None, tangent=None):
    """J_theta . dtheta: gls_jacobian_model.jvp_model along dK = B . dtheta (`value`, `scale`, `tangent`)"""
    B = per_cell(B, len(perm))
    return JM.jvp_model(grid, perm, diff_mag, neumann_flag, u, direction(B, dtheta), b=b, tangent=tangent)


def vjp_model(grid, perm, diff_mag, neumann_flag, u, B, v, b=None, full=None):
    """J_theta^T . v: `grad_theta` [E][M] = the folded J^T v contracted with B, and `scale` [E][M]; `full`: gls_jacobian_model.vjp_model's
    answer (given: not computed again -- it does not depend on the basis)"""
    B = per_cell(B, len(perm))
    m = full if full is not None else JM.vjp_model(grid, perm, diff_mag, neumann_flag, u, v, b=b)
    cell = m["scale_perm"] + m["scale_diff_mag"] * np.abs(GM.diff_mag_derivative(perm))
    return {"grad_theta": np.einsum("emk,ek->em", B, m["folded"]), "scale": np.abs(B).sum(axis=2) * cell[:, None], "full": m}
