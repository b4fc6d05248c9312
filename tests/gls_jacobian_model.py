"""A numpy model of the GLS Jacobian in the permeability applied both ways: glue over tests/gls_tangent_model.py and
tests/gls_adjoint_model.py, which stay as they are.

For a cell field u [E] and optional node values b [P] the node values are F_p(K) = sum_i d_i(K) u[c_i] + nws_p(K) b_p, with d the
stored weights (add_neumann = 1) and nws the row's neumann_ws.
  J . dK   from the tangent model: sum_i tangent[eb + i] u[c_i] + tangent_neumann_ws[p] b_p, with the row scale
           scale_p (sum_i |u[c_i]| + |b_p|) of the tangent model's scale_p -- a row's value is a sum of differences of two terms
  J^T . v  from the adjoint model with grad_csr[pos] = v_p u[esup[pos]] and grad_neumann_ws = v b: grad_perm [E][9], grad_diff_mag
           [E] with its scale_perm / scale_diff_mag, and fold() for the folded form

Not a test module (no test_ prefix): tests/test_gls_jacobian_model.py pins it on the CPU, tests/test_gpu_gls_jacobian.py holds the
device kernels to it."""
import numpy as np

import gls_adjoint_model as GM
import gls_tangent_model as TM


def _rows(grid):
    ptr = np.asarray(grid.esup_ptr).astype(np.int64)
    return ptr, np.asarray(grid.esup).astype(np.int64), np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def jvp_model(grid, perm, diff_mag, neumann_flag, u, dK, b=None, ddm=None, tangent=None):
    """`value` [P] = J . dK (ddm [E]: d diff_mag as an input of its own; None: folded) and `scale` [P], the room a row's error is
    measured against (0 on a row without a tangent); `tangent`: the tangent model's answer (given: not computed again -- it depends on
    the direction alone, not on u or b)"""
    ptr, esup, rows = _rows(grid)
    P = len(ptr) - 1
    u = np.asarray(u, dtype=float)
    m = tangent if tangent is not None else TM.gls_tangent_model(grid, perm, diff_mag, neumann_flag, dK, ddm=ddm, add_neumann=True)
    value = np.bincount(rows, weights=m["tangent"] * u[esup], minlength=P)
    room = np.bincount(rows, weights=np.abs(u[esup]), minlength=P)
    if b is not None:
        b = np.asarray(b, dtype=float)
        value = value + m["tangent_neumann_ws"] * b
        room = room + np.abs(b)
    return {"value": value, "scale": m["scale"] * room, "tangent": m}


def vjp_model(grid, perm, diff_mag, neumann_flag, u, v, b=None):
    """J^T . v: `grad_perm` [E][9] with diff_mag held fixed and `grad_diff_mag` [E], `folded` [E][9] the gradient in K alone, and the
    adjoint model's `scale_perm` / `scale_diff_mag` [E]"""
    ptr, esup, rows = _rows(grid)
    u, v = np.asarray(u, dtype=float), np.asarray(v, dtype=float)
    adj = GM.gls_adjoint_model(grid, perm, diff_mag, neumann_flag, v[rows] * u[esup], add_neumann=True,
                               grad_neumann_ws=None if b is None else v * np.asarray(b, dtype=float))
    return {"grad_perm": adj["grad_perm"], "grad_diff_mag": adj["grad_diff_mag"], "folded": GM.fold(adj["grad_perm"], adj["grad_diff_mag"], perm),
            "scale_perm": adj["scale_perm"], "scale_diff_mag": adj["scale_diff_mag"]}
