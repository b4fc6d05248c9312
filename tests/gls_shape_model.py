"""A numpy model of the GLS weights differentiated with respect to the node coordinates: the shape adjoint.

Per computed node the system, the factorisation and Abar = -q y^T - r s^T are those of tests/gls_derivative_exact.py (GM.assemble, one
Householder QR in a number format of the caller's choice: numpy.longdouble is the 80-bit model the device is held to, numpy.float64 the
restatement whose distance from it measures what a float64 solver may lose).  The coordinates enter A through four geometric inputs:

  cell row i (cell e)          A[i, 3i:3i+3] = centroid_e - x_p:   cbar(p, e) = Abar(i, 3i:3i+3),  xbar_p -= the same
  internal face f, rows t..t+2, local cells Ia, Ib; N the resident normal, T = x_p - fc_f, U = N x T, tau = |U|^-eta,
  D_k = Abar(t+k, 3Ib:3Ib+3) - Abar(t+k, 3Ia:3Ia+3):
      Nbar  = K_b^T Abar(t, 3Ib:) - K_a^T Abar(t, 3Ia:)                              (the K.N row)
      Ubar  = tau D_2 - eta tau (D_2.U) / |U|^2 U                                    (the tau.U row; eta depends on K alone)
      Tbar  = D_1 + Ubar x N,   Nbar += T x Ubar,   xbar_p += Tbar,   fcbar(p, f) = -Tbar
  Neumann boundary face row t (cell a):  Nbar(p, f) = -K_a^T Abar(t, 3Ia:)

and the geometry chain (csrc/geom_math.hpp, 3-D) takes those to the vertices:

  centroid_e = sum x_v / n_e             every vertex of e gets Cbar_e / n_e,  Cbar_e = sum_p cbar(p, e)
  fc_f = sum x_v / npofa                 every vertex of f gets Fcbar_f / npofa -- the fourth vertex of a quadrilateral too
  n = v1 x v2, v1 = x_0 - x_1, v2 = x_2 - x_1 (the first three points of the inpofa row), N = n / |n|:
      nbar = (Nbar_f - (Nbar_f.N) N) / |n|,  v1bar = v2 x nbar,  v2bar = nbar x v1,  xbar_0 += v1bar,  xbar_2 += v2bar,
      xbar_1 -= v1bar + v2bar

The derivative is that of the real-valued model: the float32 casts of the resident normals count as the identity.  Dirichlet nodes
are not computed but receive gradient as vertices of their cells and faces.  The Neumann seeding of g is the K adjoint's.

`grid` is any bag with the Grid's array names (esup, fsup, esuf, their pointers, point_coords, centroids, faces_centers, normal_faces,
boundary_points): the library's Grid, the oracle's, or smooth_bag() -- the same connectivity with the geometry recomputed from
coordinates in float64, the forward whose central differences pin this model (tests/test_gls_shape_model.py).

scale [P][3]: per coordinate the sum of the absolute values of the contributions, carried through the same chain with every sign
made a plus.

Not a test module (no test_ prefix).  Plain numpy."""
import types

import numpy as np

import gls_adjoint_model as GM
from gls_derivative_exact import qr
from gls_exact import LD

MUTANTS = ("quad_fourth_vertex", "normal_projection", "dtau")
# The adjoint kernel's bar per entry on the scale of its absolute contributions (tests/test_gpu_gls_adjoint.py, where it is derived;
# tests/test_gpu_gls_shape_adjoint.py asserts that the two are one number): the floor of the device bar and the bar of the translation
# sums, here so that the CPU tests need no GPU test module for it
ADJOINT_RTOL = 5.1e-11


def face_points(inpofa):
    """[(the points of face f in inpofa order)]: a row ends at the first -1"""
    rows = np.asarray(inpofa).astype(np.int64).reshape(-1, 4)
    return [r[:(list(r) + [-1]).index(-1)] for r in rows]


def cell_points(inpoel):
    rows = np.asarray(inpoel).astype(np.int64)
    return [r[r >= 0] for r in rows]


def smooth_geometry(coords, inpoel, inpofa):
    """(centroids [E][3], face centres [F][3], unit normals [F][3]) from coords [P][3] in float64: the mean of a cell's points, the mean
    of a face's, the normalised cross product of the first three points of the face's row"""
    X = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    cen = np.array([X[v].mean(axis=0) for v in cell_points(inpoel)])
    fp = face_points(inpofa)
    fc = np.array([X[v].mean(axis=0) for v in fp])
    n = np.array([np.cross(X[v[0]] - X[v[1]], X[v[2]] - X[v[1]]) for v in fp])
    return cen, fc, n / np.sqrt((n * n).sum(axis=1))[:, None]


def smooth_bag(grid, coords, inpoel, inpofa):
    """grid's connectivity with the geometry of `coords`, all float64"""
    cen, fc, N = smooth_geometry(coords, inpoel, inpofa)
    bag = types.SimpleNamespace(**{k: np.asarray(getattr(grid, k)) for k in ("esup", "esup_ptr", "fsup", "fsup_ptr", "esuf", "esuf_ptr",
                                                                            "boundary_points")})
    bag.point_coords, bag.centroids, bag.faces_centers, bag.normal_faces = np.array(coords, dtype=np.float64).reshape(-1, 3), cen, fc, N
    return bag


def loss(grid, perm, diff_mag, flag, grad_csr, grad_neumann_ws=None, add_neumann=True, nodes=None):
    """<grad_csr, stored weights> + <grad_neumann_ws, neumann_ws> of the float64 forward (numpy lstsq) over `nodes` (default: all)"""
    geo = GM._Geometry(grid)
    perm = np.asarray(perm, dtype=np.float64).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=np.float64)
    neu = np.asarray(flag).astype(np.int64) != 0
    total = 0.0
    for p in (range(geo.P) if nodes is None else nodes):
        sys_ = GM.assemble(geo, p, perm, dmag, bool(neu[p]))
        if sys_ is None:
            continue
        A, c, _, cells = sys_
        ne, eb = len(cells), geo.esup_ptr[p]
        y = np.linalg.lstsq(A, c, rcond=None)[0]
        r = c - A @ y
        rho = r @ r
        w = r[:ne] / rho
        nws = w[ne - 1] if neu[p] else 0.0
        total += grad_csr[eb:eb + ne] @ (w + (nws if add_neumann else 0.0))
        if grad_neumann_ws is not None:
            total += grad_neumann_ws[p] * nws
    return float(total)


def _cross_abs(a, b):
    """the cross product with every sign a plus: the scale of a x b from the scales of a and b"""
    a, b = np.abs(a), np.abs(b)
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]], dtype=a.dtype)


def shape_adjoints(grid, perm, diff_mag, flag, inpoel, inpofa, cotangents, dtype=LD, mutant=None):
    """One pass over the nodes, one factorisation per node, any number of cotangents [(grad_csr [nnz_esup], grad_neumann_ws [P] or
    None, add_neumann)] -> a dict each: grad_points [P][3] = dL/d point_coords for L = <grad_csr, stored weights> + <grad_neumann_ws,
    neumann_ws>, scale [P][3] and computed [P]; in dtype.  mutant: one of MUTANTS, a one-line error the tests must be able to see."""
    assert mutant is None or mutant in MUTANTS
    geo = GM._Geometry(grid)
    perm = np.asarray(perm, dtype=np.float64).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=np.float64)
    neu = np.asarray(flag).astype(np.int64) != 0
    cots = [(np.asarray(g, dtype=dtype), None if gn is None else np.asarray(gn, dtype=dtype), bool(an)) for g, gn, an in cotangents]
    P, E, F = geo.P, geo.E, len(geo.fc)
    Z = lambda *shape: np.zeros(shape, dtype=dtype)                          # noqa: E731
    K = perm.astype(dtype).reshape(E, 3, 3)
    X = geo.coords.astype(dtype)
    # per cotangent: the gradient and its scale, and (value, scale) of Cbar [E], Fcbar [F], Nbar [F]
    acc = [{"grad": Z(P, 3), "scale": Z(P, 3), "Cb": Z(E, 3), "Ca": Z(E, 3), "Fb": Z(F, 3), "Fa": Z(F, 3), "Nb": Z(F, 3), "Na": Z(F, 3)}
           for _ in cots]
    computed = np.zeros(P, dtype=bool)
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
        Y3 = y.reshape(ne, 3)
        faces = []
        for kind, f, t, Ia, Ib, N64, U64, un64, tau64, eta64, _ in rows:
            N = np.asarray(N64, dtype=np.float64).astype(dtype)
            if kind == "neumann":
                faces.append((kind, f, t, Ia, Ib, N, None, None, None, None, None))
            else:
                T = (geo.coords[p] - geo.fcent[f]).astype(dtype)
                faces.append((kind, f, t, Ia, Ib, N, T, np.asarray(U64).astype(dtype), dtype(un64), dtype(tau64), dtype(eta64)))
        for (ghat_all, gnws_all, add_neumann), o in zip(cots, acc):
            g = Z(m)
            g[:ne] = ghat_all[eb:eb + ne]
            if neu[p]:
                if add_neumann:
                    g[ne - 1] += ghat_all[eb:eb + ne].sum()
                if gnws_all is not None:
                    g[ne - 1] += gnws_all[p]
            rbar = g / rho - 2 * (g @ r) * r / (rho * rho)
            z = Fq.qt(rbar)
            s = Fq.r_solve(z[:nc])
            z[:nc] = 0
            q = Fq.q(z)
            S3 = s.reshape(ne, 3)
            ab = lambda t, i: -(q[t] * Y3[i]) - r[t] * S3[i]                  # noqa: E731  (Abar(t, 3i:3i+3))
            grad, scale = o["grad"], o["scale"]
            for i, e in enumerate(cells):
                cb = ab(i, i)
                o["Cb"][e] += cb
                o["Ca"][e] += np.abs(cb)
                grad[p] -= cb
                scale[p] += np.abs(cb)
            for kind, f, t, Ia, Ib, N, T, U, un, tau, eta in faces:
                a = cells[Ia]
                if kind == "neumann":
                    nbar = -(K[a].T @ ab(t, Ia))
                    o["Nb"][f] += nbar
                    o["Na"][f] += np.abs(nbar)
                    continue
                b = cells[Ib]
                nbar = K[b].T @ ab(t, Ib) - K[a].T @ ab(t, Ia)
                D1, D2 = ab(t + 1, Ib) - ab(t + 1, Ia), ab(t + 2, Ib) - ab(t + 2, Ia)
                ubar = tau * D2
                if eta != 0 and mutant != "dtau":
                    ubar = ubar - (eta * tau * (D2 @ U) / (un * un)) * U
                tbar = D1 + np.cross(ubar, N)
                nbar = nbar + np.cross(T, ubar)
                grad[p] += tbar
                scale[p] += np.abs(tbar)
                o["Fb"][f] -= tbar
                o["Fa"][f] += np.abs(tbar)
                o["Nb"][f] += nbar
                o["Na"][f] += np.abs(nbar)
    # ---- the geometry chain -------------------------------------------------------------------------------------------------
    Nres = geo.normal.astype(dtype)
    cpts, fpts = cell_points(inpoel), face_points(inpofa)
    out = []
    for o in acc:
        grad, scale = o["grad"], o["scale"]
        for e, v in enumerate(cpts):
            grad[v] += o["Cb"][e] / len(v)
            scale[v] += o["Ca"][e] / len(v)
        for f, v in enumerate(fpts):
            share = v[:3] if (mutant == "quad_fourth_vertex" and len(v) == 4) else v
            grad[share] += o["Fb"][f] / len(v)
            scale[share] += o["Fa"][f] / len(v)
            v1, v2 = X[v[0]] - X[v[1]], X[v[2]] - X[v[1]]
            n = np.cross(v1, v2)
            nn = np.sqrt(n @ n)
            N, Nb, Na = Nres[f], o["Nb"][f], o["Na"][f]
            if mutant == "normal_projection":
                nbar, nabs = Nb / nn, Na / nn
            else:
                nbar, nabs = (Nb - (Nb @ N) * N) / nn, (Na + (Na @ np.abs(N)) * np.abs(N)) / nn
            v1b, v2b = np.cross(v2, nbar), np.cross(nbar, v1)
            v1a, v2a = _cross_abs(v2, nabs), _cross_abs(nabs, v1)
            grad[v[0]] += v1b
            grad[v[2]] += v2b
            grad[v[1]] -= v1b + v2b
            scale[v[0]] += v1a
            scale[v[2]] += v2a
            scale[v[1]] += v1a + v2a
        out.append({"grad_points": grad, "scale": scale, "computed": computed})
    return out


def shape_adjoint(grid, perm, diff_mag, flag, inpoel, inpofa, grad_csr, grad_neumann_ws=None, add_neumann=True, dtype=LD, mutant=None):
    """shape_adjoints for one cotangent"""
    return shape_adjoints(grid, perm, diff_mag, flag, inpoel, inpofa, [(grad_csr, grad_neumann_ws, add_neumann)], dtype, mutant)[0]
