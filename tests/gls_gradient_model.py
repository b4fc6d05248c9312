"""A numpy model of the corner gradients of the GLS reconstruction: the gradient half of the per-node least-squares
solve whose last unknown the weights keep.  Per computed node, with the system of tests/gls_adjoint_model.py (GM.assemble: A m x 3 ne,
c the last column) and ONE Householder QR of A in a number format of the caller's choice (gls_derivative_exact.qr -- the kernel's
algorithm: dlarfg reflectors, columns in esup order):

    y = argmin |c - A y|,  r = c - A y,  rho = r.r                      (the weights' half: w_i = r_i / rho on the cell rows)
    b = u on the cell rows, 0 on every face row (Neumann rows too)     (a homogeneous system, as the stored weights are)
    u_p = (r.b) / rho,   g = argmin |(b - c u_p) - A g|                 ((g, u_p) is the least-squares solution of [A | c] x = b)

  dtype = numpy.longdouble   the 80-bit model: what the device is held to
  dtype = numpy.float64      the float64 restatement: what a correct float64 solver loses on that system

Both start from the same float64 system (assembled in float64, then cast), as the derivative models do.  Per entry a scale: the sum
of the absolute contributions, sum_j |A+_kj| |b'_j| with b' = b - c u_p for g and sum_i |w_i| |u_i| for u_p (|A+| from LAPACK's
float64 pseudo-inverse in either format: it only sets the scale).  With `room` [E] (an
absolute uncertainty of every cell value) the model also propagates it: room_up = sum_i |w_i| room_i and
room_g[k] = sum_j |A+_kj| (room_j + c_j room_up) -- what the rounding of the inputs may move the answer by, solver aside.

Mutants (tests/test_gls_gradient_model.py shows that the test meshes tell them from the model): "face_rhs" -- b = 1 on the first
face row instead of 0; "no_cup" -- g = argmin |b - A g|, the c u_p term missing.

Not a test module (no test_ prefix).  Plain numpy."""
import numpy as np

import gls_adjoint_model as GM
import gls_derivative_exact as D
from gls_exact import LD

MUTANTS = ("face_rhs", "no_cup")


def corner_gradients(grid, perm, diff_mag, flag, u, dtype=LD, mutant=None, room=None, nodes=None):
    """u [E] or [k][E] -> a dict of dtype arrays shaped [k][...] (k = 1 for one field): grad [k][nnz_esup][3], node_values [k][P], scale
    [k][nnz_esup][3], scale_node [k][P], computed [P] (bool); with room [E] also room_grad [k][nnz_esup][3] and room_node [k][P].  Zero rows are
    zeros.  nodes: only these (default: all)."""
    assert mutant is None or mutant in MUTANTS
    geo = GM._Geometry(grid)
    perm = np.asarray(perm, dtype=np.float64).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=np.float64)
    neu = np.asarray(flag).astype(np.int64) != 0
    U = np.atleast_2d(np.asarray(u, dtype=np.float64)).astype(dtype)
    k, nnz, P = U.shape[0], len(geo.esup), geo.P
    Z = lambda *shape: np.zeros(shape, dtype=dtype)                          # noqa: E731
    out = {"grad": Z(k, nnz, 3), "node_values": Z(k, P), "scale": Z(k, nnz, 3), "scale_node": Z(k, P), "computed": np.zeros(P, dtype=bool)}
    if room is not None:
        room = np.asarray(room, dtype=np.float64).astype(dtype)
        out.update(room_grad=Z(k, nnz, 3), room_node=Z(k, P))
    for p in (range(P) if nodes is None else nodes):
        sys_ = GM.assemble(geo, p, perm, dmag, bool(neu[p]))
        if sys_ is None:
            continue
        A64, c64, rows, cells = sys_
        ne, eb = len(cells), geo.esup_ptr[p]
        m, nc = A64.shape
        F = D.qr(A64, dtype)
        if F.singular:
            continue
        c = c64.astype(dtype)
        ct = F.qt(c)
        ct[:nc] = 0
        r = F.q(ct)
        rho = r @ r
        with np.errstate(all="ignore"):
            w = r[:ne] / rho
        if not (rho > 0) or not np.all(np.isfinite(w)):
            continue
        out["computed"][p] = True
        b = Z(m, k)
        b[:ne] = U[:, cells].T
        if mutant == "face_rhs":
            b[ne] = 1
        up = (r @ b) / rho
        bp = b if mutant == "no_cup" else b - np.outer(c, up)
        g = F.r_solve(F.qt(bp)[:nc])
        pinv = np.abs(np.linalg.pinv(A64)).astype(dtype)                         # |A+| [nc][m]: a scale, taken in float64 whatever dtype
        out["grad"][:, eb:eb + ne] = g.T.reshape(k, ne, 3)
        out["node_values"][:, p] = up
        out["scale"][:, eb:eb + ne] = (pinv @ np.abs(bp)).T.reshape(k, ne, 3)
        out["scale_node"][:, p] = np.abs(w) @ np.abs(b[:ne])
        if room is not None:
            d = Z(m)
            d[:ne] = room[cells]
            dup = np.abs(w) @ d[:ne]
            out["room_grad"][:, eb:eb + ne] = (pinv @ (d + np.abs(c) * dup)).reshape(ne, 3)
            out["room_node"][:, p] = dup
    return out


def normal_equation_defect(grid, perm, diff_mag, flag, u, model, dtype=LD):
    """max over the computed nodes and the unknowns of |M^T (b - M x)| / (|M|^T (|b| + |M| |x|)) with M = [A | c] and x = (g, u_p) of
    `model` (one field), all in dtype: 0 for the exact least-squares solution, a few units of dtype's roundoff for a computed one"""
    geo = GM._Geometry(grid)
    perm = np.asarray(perm, dtype=np.float64).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=np.float64)
    neu = np.asarray(flag).astype(np.int64) != 0
    u = np.asarray(u, dtype=np.float64).astype(dtype)
    worst = 0.0
    for p in np.flatnonzero(model["computed"]):
        A64, c64, rows, cells = GM.assemble(geo, p, perm, dmag, bool(neu[p]))
        ne, eb = len(cells), geo.esup_ptr[p]
        Mx = np.concatenate([A64, c64[:, None]], axis=1).astype(dtype)
        x = np.concatenate([np.asarray(model["grad"][0, eb:eb + ne], dtype=dtype).reshape(-1), [dtype(model["node_values"][0, p])]])
        b = np.zeros(len(c64), dtype=dtype)
        b[:ne] = u[cells]
        res = b - Mx @ x
        room = np.abs(Mx).T @ (np.abs(b) + np.abs(Mx) @ np.abs(x))
        worst = max(worst, float((np.abs(Mx.T @ res) / room).max()))
    return worst


def linear_field(grid, a, beta):
    """u = a + beta . x at the centroids in float64, and room [E] = the bound on its rounding: one rounding per product and per sum,
    (1 + eps)^6 - 1 < 7 eps64 of |a| + sum_k |beta_k x_k|"""
    X = np.asarray(grid.centroids, dtype=np.float64).reshape(-1, 3)
    beta = np.asarray(beta, dtype=np.float64)
    u = a + ((beta[0] * X[:, 0] + beta[1] * X[:, 1]) + beta[2] * X[:, 2])
    room = 7 * np.finfo(np.float64).eps * (abs(a) + np.abs(beta * X).sum(axis=1))
    return u, room
