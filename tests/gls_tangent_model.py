"""A numpy model of the directional derivative of the GLS weights in the permeability, node by node over the dense
system of tests/gls_adjoint_model.py (its `assemble`, its geometry), numpy.linalg.lstsq for every projection.

Per computed node, with y = argmin |c - A y|, r = c - A y, rho = r.r, w_i = r_i / rho on the cell rows and the stored entry
d_i = w_i + nws (nws = w_{ne-1} on a Neumann node, when add_neumann), and a direction dK (9 per cell) with ddm (per cell; given, or
folded: ddm_e = 2 (1 - 3 / tr K_e) 3 / tr K_e^2 tr dK_e):
  dA     -(dK_a N) on cell a's columns and +(dK_b N) on cell b's in the K.N row of an internal face; -/+ dtau U in its tau.T2 row with
         dtau = -ln|T2| tau ddm_pick (pick: the cell the forward's max() takes eta from, nobody: 0); -(dK_a N) in a Neumann boundary row
  dr     = -P_perp (dA y) - (A^+)^T (dA^T r)          (r = P_perp c)
  drho   = 2 r.dr,   dw_i = dr_i / rho - r_i drho / rho^2,   dnws = dw_{ne-1} on a Neumann node,   dd_i = dw_i + (add_neumann ? dnws : 0)
A node with the forward's zero row has tangent 0.

Not a test module (no test_ prefix): tests/test_gls_tangent_model.py pins it against central differences of the oracle and against the
adjoint model, tests/test_gpu_gls_tangent.py holds the device kernel to it."""
import numpy as np

from gls_adjoint_model import _Geometry, assemble, diff_mag_derivative


def fold_direction(perm, dK):
    """ddm [E] of a direction dK [E][9] through the table's diff_mag = (1 - 3 / tr K)^2"""
    dK = np.asarray(dK, dtype=float).reshape(-1, 9)
    return diff_mag_derivative(perm) * ((dK[:, 0] + dK[:, 4]) + dK[:, 8])


def gls_tangent_model(grid, perm, diff_mag, neumann_flag, dK, ddm=None, add_neumann=True):
    """The tangent of the stored weights `tangent` [nnz_esup] and of neumann_ws `tangent_neumann_ws` [P] along dK [E][9] (ddm [E], or
    None: folded from perm), with the forward's `weights`, `neumann_ws`, `computed` [P], and `scale` [P]: per row
    max_i (|dr_i| / rho + |r_i| |drho| / rho^2) + |dnws| -- a tangent is a difference of two terms; 0 on a row without one."""
    geo = _Geometry(grid)
    perm = np.asarray(perm, dtype=float).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=float)
    dK = np.asarray(dK, dtype=float).reshape(-1, 9)
    ddm = fold_direction(perm, dK) if ddm is None else np.asarray(ddm, dtype=float)
    neu = np.asarray(neumann_flag).astype(np.int64) != 0
    nnz = len(geo.esup)
    out = {"weights": np.zeros(nnz), "neumann_ws": np.zeros(geo.P), "computed": np.zeros(geo.P, dtype=bool),
           "tangent": np.zeros(nnz), "tangent_neumann_ws": np.zeros(geo.P), "scale": np.zeros(geo.P)}
    for p in range(geo.P):
        sys_ = assemble(geo, p, perm, dmag, bool(neu[p]))
        if sys_ is None:
            continue
        A, c, rows, cells = sys_
        ne = len(cells)
        eb = geo.esup_ptr[p]
        y = np.linalg.lstsq(A, c, rcond=None)[0]
        r = c - A @ y
        rho = r @ r
        with np.errstate(all="ignore"):
            w = r[:ne] / rho
        if not (rho > 0) or not np.all(np.isfinite(w)):
            continue
        nws = w[ne - 1] if neu[p] else 0.0
        out["weights"][eb:eb + ne] = w + (nws if add_neumann else 0.0)
        out["neumann_ws"][p] = nws
        out["computed"][p] = True
        dA = np.zeros_like(A)
        for kind, f, t, Ia, Ib, N, U, un, tau, eta, pick in rows:
            a = cells[Ia]
            dA[t, 3 * Ia:3 * Ia + 3] = -(dK[a].reshape(3, 3) @ N)
            if kind == "neumann":
                continue
            b = cells[Ib]
            dA[t, 3 * Ib:3 * Ib + 3] = dK[b].reshape(3, 3) @ N
            if pick >= 0:
                dtau = -np.log(un) * tau * ddm[cells[pick]]
                dA[t + 2, 3 * Ia:3 * Ia + 3] = -dtau * U
                dA[t + 2, 3 * Ib:3 * Ib + 3] = dtau * U
        z1 = dA @ y
        z2 = dA.T @ r
        dr = -(z1 - A @ np.linalg.lstsq(A, z1, rcond=None)[0]) - np.linalg.lstsq(A.T, z2, rcond=None)[0]   # (A^+)^T z2: the least-norm solution of A^T x = z2
        drho = 2 * (r @ dr)
        dw = dr[:ne] / rho - r[:ne] * drho / rho ** 2
        dnws = dw[ne - 1] if neu[p] else 0.0
        out["tangent"][eb:eb + ne] = dw + (dnws if add_neumann else 0.0)
        out["tangent_neumann_ws"][p] = dnws
        out["scale"][p] = (np.abs(dr[:ne]) / rho + np.abs(r[:ne]) * abs(drho) / rho ** 2).max() + abs(dnws)
    return out
