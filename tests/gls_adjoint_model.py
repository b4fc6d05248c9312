"""A numpy model of the GLS weights and of their adjoint with respect to the permeability, node by node from
the Grid arrays: the dense m x n system of csrc/kernels_gls.hip's header, numpy.linalg.lstsq for the two least-squares solves.

Forward, per computed node:  y = argmin |c - A y|,  r = c - A y,  rho = r.r,  w_i = r_i / rho on the cell rows; the stored entry is
d_i = w_i + nws, nws = w_{ne-1} on a Neumann node (when add_neumann), else 0.
Backward, given ghat_i = dL/dd_i (and optionally dL/dneumann_ws[p]):  g = ghat on the cell rows (+ the nws terms on row ne-1),
rbar = g / rho - 2 (g.r) r / rho^2,  s = argmin |rbar - A s|,  q = rbar - A s,  Abar = -q y^T - r s^T; K enters A through the K.N
rows (internal faces, Neumann boundary faces) and through eta = max(0, diff_mag_a, diff_mag_b) of the tau.T2 rows.

Not a test module (no test_ prefix): tests/test_gls_adjoint_model.py pins it against central differences of the oracle,
tests/test_gpu_gls_adjoint.py holds the device kernels to it."""
import numpy as np


def face_cells(grid):
    """[F][2] cells of every face, the second -1 on a boundary face (esuf / esuf_ptr)"""
    esuf, ptr = np.asarray(grid.esuf).astype(np.int64), np.asarray(grid.esuf_ptr).astype(np.int64)
    F = len(ptr) - 1
    fc = -np.ones((F, 2), dtype=np.int64)
    cnt = np.diff(ptr)
    fc[:, 0] = esuf[ptr[:-1]]
    two = cnt >= 2
    fc[two, 1] = esuf[ptr[:-1][two] + 1]
    return fc


def diff_mag_of(perm):
    """(1 - 3 / tr K)^2, the table's expression"""
    perm = np.asarray(perm, dtype=float).reshape(-1, 9)
    tr = (perm[:, 0] + perm[:, 4]) + perm[:, 8]
    return (1 - 3 / tr) ** 2


def diff_mag_derivative(perm):
    """d diff_mag / d K_dd (the same on the three diagonal entries): 2 (1 - 3 / tr) 3 / tr^2"""
    perm = np.asarray(perm, dtype=float).reshape(-1, 9)
    tr = (perm[:, 0] + perm[:, 4]) + perm[:, 8]
    return 2 * (1 - 3 / tr) * 3 / tr ** 2


def fold(grad_perm, grad_diff_mag, perm):
    """the chain rule through the table's diff_mag: the gradient with respect to K alone"""
    out = np.array(grad_perm, dtype=float).reshape(-1, 9).copy()
    t = np.asarray(grad_diff_mag) * diff_mag_derivative(perm)
    for d in (0, 4, 8):
        out[:, d] += t
    return out


class _Geometry:
    def __init__(self, grid):
        g = grid
        self.esup, self.esup_ptr = np.asarray(g.esup).astype(np.int64), np.asarray(g.esup_ptr).astype(np.int64)
        self.fsup, self.fsup_ptr = np.asarray(g.fsup).astype(np.int64), np.asarray(g.fsup_ptr).astype(np.int64)
        self.fc = face_cells(g)
        self.coords = np.asarray(g.point_coords, dtype=float).reshape(-1, 3)
        self.centroids = np.asarray(g.centroids, dtype=float).reshape(-1, 3)
        self.fcent = np.asarray(g.faces_centers, dtype=float).reshape(-1, 3)
        self.normal = np.asarray(g.normal_faces, dtype=float).reshape(-1, 3)
        self.boundary = np.asarray(g.boundary_points).astype(np.int64) != 0
        self.P, self.E = len(self.esup_ptr) - 1, len(self.centroids)


def node_shape(geo, p):
    """(ne, nf, n_bf) of node p"""
    faces = geo.fsup[geo.fsup_ptr[p]:geo.fsup_ptr[p + 1]]
    return int(geo.esup_ptr[p + 1] - geo.esup_ptr[p]), len(faces), int(np.count_nonzero(geo.fc[faces, 1] < 0))


def assemble(geo, p, perm, dmag, is_neu):
    """A (m x (n - 1)), c (m) and the face rows [(kind, face, row, Ia, Ib, N, U, |U|, tau, eta, pick)] of node p; None for a node
    that gets the zero row before any arithmetic"""
    cells = geo.esup[geo.esup_ptr[p]:geo.esup_ptr[p + 1]]
    faces = geo.fsup[geo.fsup_ptr[p]:geo.fsup_ptr[p + 1]]
    ne = len(cells)
    internal = [f for f in faces if geo.fc[f, 1] >= 0]
    bnd = [f for f in faces if geo.fc[f, 1] < 0]
    n = 3 * ne + 1
    m = ne + 3 * len(internal) + (len(bnd) if is_neu else 0)
    if (geo.boundary[p] and not is_neu) or len(internal) == 0 or m < n - 1:
        return None
    where = {int(c): i for i, c in enumerate(cells)}
    xv = geo.coords[p]
    A, c = np.zeros((m, n - 1)), np.zeros(m)
    c[:ne] = 1.0
    for i, e in enumerate(cells):
        A[i, 3 * i:3 * i + 3] = geo.centroids[e] - xv
    rows = []
    t = ne
    for f in internal:
        a, b = geo.fc[f]
        Ia, Ib = where[int(a)], where[int(b)]
        N = geo.normal[f]
        T1 = xv - geo.fcent[f]
        U = np.cross(N, T1)
        un = np.sqrt(U @ U)
        da, db = dmag[a], dmag[b]
        eta = max(0.0, da, db)
        tau = un ** (-eta)
        pick = Ib if db > da else (Ia if da > 0 else -1)
        A[t, 3 * Ia:3 * Ia + 3] = -(perm[a].reshape(3, 3) @ N)
        A[t, 3 * Ib:3 * Ib + 3] = perm[b].reshape(3, 3) @ N
        A[t + 1, 3 * Ia:3 * Ia + 3] = -T1
        A[t + 1, 3 * Ib:3 * Ib + 3] = T1
        A[t + 2, 3 * Ia:3 * Ia + 3] = -tau * U
        A[t + 2, 3 * Ib:3 * Ib + 3] = tau * U
        rows.append(("internal", f, t, Ia, Ib, N, U, un, tau, eta, pick))
        t += 3
    if is_neu:
        for f in bnd:
            a = geo.fc[f, 0]
            Ia = where[int(a)]
            N = geo.normal[f]
            A[t, 3 * Ia:3 * Ia + 3] = -(perm[a].reshape(3, 3) @ N)
            rows.append(("neumann", f, t, Ia, -1, N, None, 0.0, 0.0, 0.0, -1))
            t += 1
    return A, c, rows, cells


def gls_adjoint_model(grid, perm, diff_mag, neumann_flag, grad_csr=None, add_neumann=True, grad_neumann_ws=None):
    """The stored weights [nnz_esup] and neumann_ws [P]; with grad_csr (dL/d stored weights, [nnz_esup]; grad_neumann_ws: dL/d
    neumann_ws [P] or None) also grad_perm [E][9] (diff_mag held fixed), grad_diff_mag [E] and the error scales scale_perm [E] /
    scale_diff_mag [E]: per cell the sum of the absolute values of the contributions (the largest of the nine entries' sums for
    grad_perm) -- a cell's gradient is a sum of signed terms."""
    geo = _Geometry(grid)
    perm = np.asarray(perm, dtype=float).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=float)
    neu = np.asarray(neumann_flag).astype(np.int64) != 0
    nnz = len(geo.esup)
    out = {"weights": np.zeros(nnz), "neumann_ws": np.zeros(geo.P), "computed": np.zeros(geo.P, dtype=bool)}
    back = grad_csr is not None
    if back:
        ghat_all = np.asarray(grad_csr, dtype=float)
        gp, gd = np.zeros((geo.E, 9)), np.zeros(geo.E)
        sp, sd = np.zeros((geo.E, 9)), np.zeros(geo.E)
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
        if not back:
            continue
        g = np.zeros(len(c))
        g[:ne] = ghat_all[eb:eb + ne]
        if neu[p]:
            if add_neumann:
                g[ne - 1] += ghat_all[eb:eb + ne].sum()
            if grad_neumann_ws is not None:
                g[ne - 1] += grad_neumann_ws[p]
        rbar = g / rho - 2 * (g @ r) * r / rho ** 2
        s = np.linalg.lstsq(A, rbar, rcond=None)[0]
        q = rbar - A @ s
        abar = lambda t, col: -q[t] * y[col] - r[t] * s[col]                 # noqa: E731  (the entries of Abar that are needed)
        for kind, f, t, Ia, Ib, N, U, un, tau, eta, pick in rows:
            a = cells[Ia]
            for rr in range(3):
                term = -abar(t, 3 * Ia + rr) * N
                gp[a, 3 * rr:3 * rr + 3] += term
                sp[a, 3 * rr:3 * rr + 3] += np.abs(term)
            if kind == "neumann":
                continue
            b = cells[Ib]
            for rr in range(3):
                term = abar(t, 3 * Ib + rr) * N
                gp[b, 3 * rr:3 * rr + 3] += term
                sp[b, 3 * rr:3 * rr + 3] += np.abs(term)
            if pick >= 0:
                dot = sum((abar(t + 2, 3 * Ib + k) - abar(t + 2, 3 * Ia + k)) * U[k] for k in range(3))
                term = dot * (-np.log(un) * tau)
                gd[cells[pick]] += term
                sd[cells[pick]] += abs(term)
    if back:
        out.update(grad_perm=gp, grad_diff_mag=gd, scale_perm=sp.max(axis=1), scale_diff_mag=sd)
    return out


def adjoint_bins(grid, budgets=(16384, 40960, 159744)):
    """Nodes per bin of the adjoint kernel (csrc/kernels_gls_adjoint.hip: adj_node_bytes against the LDS budgets of 1 / 2 / 4
    wavefronts, then the global-scratch class), and every node's system bytes -- the classification the device does, restated."""
    geo = _Geometry(grid)
    counts, sizes = [0, 0, 0, 0], np.zeros(geo.P, dtype=np.int64)
    for p in range(geo.P):
        ne, nf, nbf = node_shape(geo, p)
        n = 3 * ne + 1
        m = ne + 3 * (nf - nbf) + nbf
        doubles = m * n + 3 * n + 2 * m + (ne + 3 * nf + 1) // 2
        sizes[p] = (doubles * 8 + 15) // 16 * 16
        counts[next((k for k, b in enumerate(budgets) if sizes[p] <= b), 3)] += 1
    return counts, sizes
