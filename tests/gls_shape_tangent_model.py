"""A numpy model of the directional derivative of the GLS weights in the node coordinates: the shape tangent.

Per computed node the system, the factorisation, y, r and rho are those of tests/gls_derivative_exact.py (GM.assemble, one Householder
QR in a number format of the caller's choice: numpy.longdouble is the 80-bit model the device is held to, numpy.float64 the restatement
whose distance from it measures what a float64 solver may lose).  dX [P][3] is a direction; the right-hand column c does not depend on
the coordinates, so only dA is new and the tail is the K tangent's (tests/gls_tangent_model.py):

  dr = -Q [ R^-T (dA^T r) ; (Q^T (dA y))(n-1:m) ]
  drho = 2 r.dr,   dw_i = dr_i / rho - r_i drho / rho^2,   dnws = dw_{ne-1} on a Neumann node,   dd_i = dw_i + (add_neumann ? dnws : 0)

The geometry tangents are the transposes of the chain of tests/gls_shape_model.py, the float32 casts of the resident normals again
counted as the identity:

  dC_e  = (sum_{v in e} dx_v) / n_e
  dFc_f = (sum_{v in f} dx_v) / npofa                      (the fourth vertex of a quadrilateral included)
  dn    = dv1 x v2 + v1 x dv2,  dv1 = dx_0 - dx_1,  dv2 = dx_2 - dx_1   (the first three points of the inpofa row)
  dN_f  = (dn - (dn.N) N) / |n|                            (v1, v2, |n| from the coordinates, N the grid's normal)

and the rows of dA for node p, with T = x_p - fc_f, U = N x T, tau = |U|^-eta (eta depends on K alone):

  cell row i (cell e)                       dA[i, 3i:3i+3] = dC_e - dx_p
  internal face, rows t..t+2, cells Ia, Ib  row t    -(K_a dN) on Ia's columns, +(K_b dN) on Ib's
                                            row t+1  -/+ dT,        dT = dx_p - dFc_f
                                            row t+2  -/+ d(tau U),  dU = dN x T + N x dT,  d(tau U) = tau dU - eta tau (U.dU) / |U|^2 U
  Neumann boundary face row t (cell a)      -(K_a dN) on Ia's columns

A node with the forward's zero row has tangent exactly 0.  `grid` is any bag with the Grid's array names, as for gls_shape_model.

Not a test module (no test_ prefix).  Plain numpy."""
import numpy as np

import gls_adjoint_model as GM
from gls_derivative_exact import qr
from gls_exact import LD
from gls_shape_model import cell_points, face_points

# one-line errors the tests must be able to see
MUTANTS = ("quad_fourth_vertex", "normal_projection", "dtau", "own_point")


def geometry_tangents(grid, inpoel, inpofa, dX, dtype=LD, mutant=None):
    """(dC [E][3], dFc [F][3], dN [F][3]) along dX [P][3], in dtype"""
    X = np.asarray(grid.point_coords, dtype=np.float64).reshape(-1, 3).astype(dtype)
    Nres = np.asarray(grid.normal_faces, dtype=np.float64).reshape(-1, 3).astype(dtype)
    dX = np.asarray(dX, dtype=dtype).reshape(-1, 3)
    cpts, fpts = cell_points(inpoel), face_points(inpofa)
    dC = np.array([dX[v].sum(axis=0) / len(v) for v in cpts], dtype=dtype).reshape(-1, 3)
    dFc, dN = np.zeros((len(fpts), 3), dtype=dtype), np.zeros((len(fpts), 3), dtype=dtype)
    for f, v in enumerate(fpts):
        share = v[:3] if (mutant == "quad_fourth_vertex" and len(v) == 4) else v
        dFc[f] = dX[share].sum(axis=0) / len(v)
        v1, v2 = X[v[0]] - X[v[1]], X[v[2]] - X[v[1]]
        dv1, dv2 = dX[v[0]] - dX[v[1]], dX[v[2]] - dX[v[1]]
        n = np.cross(v1, v2)
        nn = np.sqrt(n @ n)
        dn = np.cross(dv1, v2) + np.cross(v1, dv2)
        N = Nres[f]
        dN[f] = dn / nn if mutant == "normal_projection" else (dn - (dn @ N) * N) / nn
    return dC, dFc, dN


def shape_tangents(grid, perm, diff_mag, flag, inpoel, inpofa, directions, add_neumann=True, dtype=LD, mutant=None):
    """One pass over the nodes, one factorisation per node, any number of directions dX [P][3] -> a dict each: tangent [nnz_esup] (of
    the stored weights of a launch with `add_neumann`), tangent_plain [nnz_esup] (dw alone: the tangent with add_neumann = False),
    tangent_neumann_ws [P], computed [P], and scale [P]: per row max_i (|dr_i| / rho + |r_i| |drho| / rho^2) + |dnws|, the K tangent's
    scale; in dtype.  mutant: None, one of MUTANTS, or one per direction."""
    mutants = list(mutant) if isinstance(mutant, (list, tuple)) else [mutant] * len(directions)
    assert len(mutants) == len(directions) and all(m is None or m in MUTANTS for m in mutants)
    geo = GM._Geometry(grid)
    perm = np.asarray(perm, dtype=np.float64).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=np.float64)
    neu = np.asarray(flag).astype(np.int64) != 0
    nnz, P, E = len(geo.esup), geo.P, geo.E
    Z = lambda *shape: np.zeros(shape, dtype=dtype)                          # noqa: E731
    K = perm.astype(dtype).reshape(E, 3, 3)
    dirs = [np.asarray(d, dtype=np.float64).reshape(P, 3).astype(dtype) for d in directions]
    geom = [geometry_tangents(grid, inpoel, inpofa, d, dtype, mu) for d, mu in zip(dirs, mutants)]
    computed = np.zeros(P, dtype=bool)
    out = [{"tangent": Z(nnz), "tangent_plain": Z(nnz), "tangent_neumann_ws": Z(P), "scale": Z(P), "computed": computed} for _ in dirs]
    for p in range(P):
        sys_ = GM.assemble(geo, p, perm, dmag, bool(neu[p]))
        if sys_ is None:
            continue
        A64, c64, rows, cells = sys_
        ne, eb = len(cells), geo.esup_ptr[p]
        m, nc = A64.shape
        Fq = qr(A64, dtype)
        if Fq.singular:
            continue
        ct = Fq.qt(c64.astype(dtype))
        y = Fq.r_solve(ct[:nc])
        ct[:nc] = 0
        r = Fq.q(ct)
        rho = r @ r
        with np.errstate(all="ignore"):
            w = r[:ne] / rho
        if not (rho > 0) or not np.all(np.isfinite(w)):
            continue
        computed[p] = True
        faces = []
        for kind, f, t, Ia, Ib, N64, U64, un64, tau64, eta64, _ in rows:
            N = np.asarray(N64, dtype=np.float64).astype(dtype)
            if kind == "neumann":
                faces.append((kind, f, t, Ia, Ib, N, None, None, None, None, None))
            else:
                T = (geo.coords[p] - geo.fcent[f]).astype(dtype)
                faces.append((kind, f, t, Ia, Ib, N, T, np.asarray(U64).astype(dtype), dtype(un64), dtype(tau64), dtype(eta64)))
        for dX, (dC, dFc, dN), mu, o in zip(dirs, geom, mutants, out):
            dA = Z(m, nc)
            for i, e in enumerate(cells):
                dA[i, 3 * i:3 * i + 3] = dC[e] if mu == "own_point" else dC[e] - dX[p]
            for kind, f, t, Ia, Ib, N, T, U, un, tau, eta in faces:
                a = cells[Ia]
                dA[t, 3 * Ia:3 * Ia + 3] = -(K[a] @ dN[f])
                if kind == "neumann":
                    continue
                b = cells[Ib]
                dA[t, 3 * Ib:3 * Ib + 3] = K[b] @ dN[f]
                dT = dX[p] - dFc[f]
                dA[t + 1, 3 * Ia:3 * Ia + 3] = -dT
                dA[t + 1, 3 * Ib:3 * Ib + 3] = dT
                dU = np.cross(dN[f], T) + np.cross(N, dT)
                dtU = tau * dU
                if eta != 0 and mu != "dtau":
                    dtU = dtU - (eta * tau * (U @ dU) / (un * un)) * U
                dA[t + 2, 3 * Ia:3 * Ia + 3] = -dtU
                dA[t + 2, 3 * Ib:3 * Ib + 3] = dtU
            z = Fq.qt(dA @ y)
            z[:nc] = Fq.rt_solve(dA.T @ r)
            dr = -Fq.q(z)
            drho = 2 * (r @ dr)
            dw = dr[:ne] / rho - r[:ne] * drho / (rho * rho)
            dnws = dw[ne - 1] if neu[p] else dtype(0)
            o["tangent_plain"][eb:eb + ne] = dw
            o["tangent"][eb:eb + ne] = dw + (dnws if add_neumann else 0)
            o["tangent_neumann_ws"][p] = dnws
            o["scale"][p] = (np.abs(dr[:ne]) / rho + np.abs(r[:ne]) * abs(drho) / (rho * rho)).max() + abs(dnws)
    return out


def shape_tangent(grid, perm, diff_mag, flag, inpoel, inpofa, dX, add_neumann=True, dtype=LD, mutant=None):
    """shape_tangents for one direction"""
    return shape_tangents(grid, perm, diff_mag, flag, inpoel, inpofa, [dX], add_neumann, dtype, mutant)[0]
