"""The high-precision yardstick of the GLS derivative tests: the adjoint and the tangent of the GLS weights in the permeability
 by the formulas of tests/gls_adjoint_model.py and tests/gls_tangent_model.py, with every projection taken
through ONE Householder QR of the node's system -- the kernel's algorithm (csrc/kernels_gls_adjoint.hip: dlarfg reflectors, columns
in esup order) -- in a number format of the caller's choice:

  dtype = numpy.longdouble   the 80-bit model ("exact"): what every derivative kernel is held to
  dtype = numpy.float64      the float64 restatement: the same algorithm in the kernels' own format.  Its distance from the 80-bit
                             model is what a correct float64 solver loses on that system, and the measure of what a kernel may lose.

Both start from the SAME float64 system: A, |U| and tau are assembled in float64 by gls_adjoint_model.assemble and then cast (the
question is what a float64 solver does to that system; tests/gls_exact.py makes the same choice for the forward weights); log|U| and
everything behind the assembly run in `dtype`.  The lstsq models the device tests were written against are themselves up to sixty
times further from the 80-bit model than this restatement on their own ALH unit-box cases (grad_perm on the Delaunay mesh: 3.48e-12
against 5.7e-14; tests/test_gls_derivative_exact.py prints both).

adjoint() and tangent() are the two derivations; they share the assembly and the factorisation and nothing after it, and
tests/test_gls_derivative_exact.py holds them to each other through the duality <ghat, dd> + <gnws, dnws> = <Kbar, dK> + <etabar, ddm>
in 80 bits.  jvp() / vjp() and their reduced forms are glue, as tests/gls_jacobian_model.py and tests/gls_reduced_jacobian_model.py are.

Rules: the four places where a derivative kernel can be wrong while every forward kernel is right -- the sign of log|U|, the cell a
tie of eta = max(0, diff_mag_a, diff_mag_b) is charged to, the faces where max() takes eta from nobody, the factor of the fold.  The
standard rules are the kernels'; the others are the mutants the CPU tests use to show that the cases below can see such a bug.

Not a test module (no test_ prefix).  Plain numpy."""
import numpy as np

import gls_adjoint_model as GM
import gls_exact as X
from gls_exact import LD

# (gls_exact's top-level assert on longdouble's eps is in force: with a longdouble that is only a float64 nothing here means anything)
assert np.finfo(LD).eps < 2e-19

# A case is in the set only if the float64 restatement is within CASE_CAP of the 80-bit model on every output: 1e-8 is the level at
# which the lstsq models are pinned to central differences of the oracle (FD_RTOL, tests/test_gls_adjoint_model.py) -- beyond it no
# float64 solver says anything about the derivative.
CASE_CAP = 1e-8


class Rules:
    """how K reaches tau: the kernels' rules by default, one mutation at a time otherwise"""

    def __init__(self, log_sign=-1.0, tie_to_b=False, zero_to_a=False, fold_tr_shift=0.0):
        self.log_sign, self.tie_to_b, self.zero_to_a, self.fold_tr_shift = log_sign, tie_to_b, zero_to_a, fold_tr_shift

    def pick(self, da, db, Ia, Ib):
        """the local cell eta = max(0, da, db) is taken from, -1: nobody (kernels_gls_adjoint.hip: db > da ? Ib : (da > 0 ? Ia : -1))"""
        if db > da:
            return Ib
        if da > 0:
            return Ib if (self.tie_to_b and da == db) else Ia
        return Ia if self.zero_to_a else -1

    def fold_factor(self, perm, dtype):
        """d diff_mag / d K_dd = 2 (1 - 3 / tr) 3 / tr^2 [E], evaluated in dtype from the float64 perm"""
        K = np.asarray(perm, dtype=np.float64).reshape(-1, 9).astype(dtype)
        tr = ((K[:, 0] + K[:, 4]) + K[:, 8]) - dtype(self.fold_tr_shift)
        return 2 * (1 - 3 / tr) * 3 / (tr * tr)


STANDARD = Rules()
MUTANTS = {
    "log_sign": Rules(log_sign=+1.0),                # +log|U| for -log|U|
    "tie_to_b": Rules(tie_to_b=True),                # pick = Ib at a tie da == db > 0
    "zero_to_a": Rules(zero_to_a=True),              # pick = Ia where da == 0 (and db == 0): eta is nobody's there
    "fold_tr_shift": Rules(fold_tr_shift=3.0),       # the fold factor with tr - 3 for tr
}


class qr:
    """Householder QR of A (m x n, m >= n or not: a column without rows below it gets the identity), dlarfg reflectors, columns in the
    order given, all arithmetic in dtype.  R on and above the diagonal of self.a, v_k (v_k[k] = 1) below it, self.tau as LAPACK keeps
    them.  singular: a pivot column that is zero on and below its diagonal.  The solves take a vector [m] or a block [m][k]."""

    def __init__(self, A, dtype):
        a = np.array(A, dtype=dtype)
        m, n = a.shape
        tau = np.zeros(n, dtype=dtype)
        self.singular = False
        for k in range(n):
            alpha = a[k, k]
            x = a[k + 1:, k]
            ss = x @ x
            if ss != 0:
                beta = -np.copysign(np.sqrt(alpha * alpha + ss), alpha)
                tau[k] = (beta - alpha) / beta
                x *= 1 / (alpha - beta)
                a[k, k] = 1
                if k + 1 < n:
                    v = a[k:, k]
                    a[k:, k + 1:] -= np.outer(v, tau[k] * (v @ a[k:, k + 1:]))
                a[k, k] = beta
            elif alpha == 0:
                self.singular = True
        self.a, self.tau, self.m, self.n, self.dtype = a, tau, m, n, dtype

    def _sweep(self, z, order):
        z = np.array(z, dtype=self.dtype)
        a, tau = self.a, self.tau
        for k in order:
            if tau[k] == 0:
                continue
            v = a[k:, k].copy()
            v[0] = 1
            if z.ndim == 1:
                z[k:] -= (tau[k] * (v @ z[k:])) * v
            else:
                z[k:] -= np.outer(v, tau[k] * (v @ z[k:]))
        return z

    def qt(self, z):
        """Q^T z"""
        return self._sweep(z, range(min(self.n, self.m)))

    def q(self, z):
        """Q z"""
        return self._sweep(z, range(min(self.n, self.m) - 1, -1, -1))

    def r_solve(self, b):
        """R^-1 b, b [n] or [n][k]"""
        x = np.array(b, dtype=self.dtype)
        a = self.a
        for k in range(self.n - 1, -1, -1):
            x[k] = (x[k] - a[k, k + 1:self.n] @ x[k + 1:]) / a[k, k]
        return x

    def rt_solve(self, b):
        """R^-T b, b [n] or [n][k]"""
        x = np.array(b, dtype=self.dtype)
        a = self.a
        for k in range(self.n):
            x[k] = (x[k] - a[:k, k] @ x[:k]) / a[k, k]
        return x

    def solve(self, b):
        """argmin |b - A x|"""
        return self.r_solve(self.qt(b)[:self.n])

    def residual(self, b):
        """b - A argmin |b - A x| = Q [0; (Q^T b)(n:m)]"""
        z = self.qt(b)
        z[:self.n] = 0
        return self.q(z)

    def pinv_t(self, z):
        """(A^+)^T z = Q [R^-T z; 0]"""
        x = self.rt_solve(z)
        return self.q(np.concatenate([x, np.zeros((self.m - self.n,) + x.shape[1:], dtype=self.dtype)], axis=0))


def _face_tables(rows, cells, dmag, dtype, rules):
    """the node's face rows as arrays: internal (T, IA, IB, N, U, coef = d tau / d eta by the rules, PICK) and Neumann (T, IA, N)"""
    it = [r for r in rows if r[0] == "internal"]
    nb = [r for r in rows if r[0] == "neumann"]
    I = {"T": np.array([r[2] for r in it], dtype=np.int64), "IA": np.array([r[3] for r in it], dtype=np.int64),
         "IB": np.array([r[4] for r in it], dtype=np.int64),
         "N": np.array([r[5] for r in it], dtype=np.float64).reshape(-1, 3).astype(dtype),
         "U": np.array([r[6] for r in it], dtype=np.float64).reshape(-1, 3).astype(dtype)}
    un = np.array([r[7] for r in it], dtype=np.float64).astype(dtype)
    tau = np.array([r[8] for r in it], dtype=np.float64).astype(dtype)
    I["coef"] = dtype(rules.log_sign) * np.log(un) * tau                  # the kernels': -ln|U| tau
    I["PICK"] = np.array([rules.pick(dmag[cells[r[3]]], dmag[cells[r[4]]], r[3], r[4]) for r in it], dtype=np.int64)
    B = {"T": np.array([r[2] for r in nb], dtype=np.int64), "IA": np.array([r[3] for r in nb], dtype=np.int64),
         "N": np.array([r[5] for r in nb], dtype=np.float64).reshape(-1, 3).astype(dtype)}
    return I, B


def derivatives(grid, perm, diff_mag, flag, adjoints=(), tangents=(), add_neumann=True, dtype=LD, rules=STANDARD):
    """One pass over the nodes, one factorisation per node, any number of right-hand sides:
      adjoints  [(grad_csr [nnz_esup], grad_neumann_ws [P] or None)] -> a dict each: grad_perm [E][9] (diff_mag held fixed),
                grad_diff_mag [E], scale_perm [E], scale_diff_mag [E] as gls_adjoint_model gives them, and folded [E][9] /
                scale_folded [E] (the chain rule through diff_mag = (1 - 3 / tr K)^2, scale_perm + scale_diff_mag |fold factor|)
      tangents  [(dK [E][9], ddm [E] or None: folded)] -> a dict each: tangent [nnz_esup], tangent_neumann_ws [P], scale [P] as
                gls_tangent_model gives them
    Returns (forward, [adjoint dicts], [tangent dicts]); forward: weights [nnz_esup], neumann_ws [P], computed [P].  Arrays are of
    dtype."""
    geo = GM._Geometry(grid)
    perm = np.asarray(perm, dtype=np.float64).reshape(-1, 9)
    dmag = np.asarray(diff_mag, dtype=np.float64)
    neu = np.asarray(flag).astype(np.int64) != 0
    nnz, P, E = len(geo.esup), geo.P, geo.E
    fold = rules.fold_factor(perm, dtype)
    Z = lambda *shape: np.zeros(shape, dtype=dtype)                          # noqa: E731
    fwd = {"weights": Z(nnz), "neumann_ws": Z(P), "computed": np.zeros(P, dtype=bool)}
    adj_in = [(np.asarray(g, dtype=dtype), None if gn is None else np.asarray(gn, dtype=dtype)) for g, gn in adjoints]
    tan_in = []
    for dK, ddm in tangents:
        dK = np.asarray(dK, dtype=dtype).reshape(E, 9)
        ddm = fold * ((dK[:, 0] + dK[:, 4]) + dK[:, 8]) if ddm is None else np.asarray(ddm, dtype=dtype)
        tan_in.append((dK.reshape(E, 3, 3), ddm))
    adj = [{"grad_perm": Z(E, 9), "grad_diff_mag": Z(E), "sp": Z(E, 9), "scale_diff_mag": Z(E)} for _ in adj_in]
    tan = [{"tangent": Z(nnz), "tangent_neumann_ws": Z(P), "scale": Z(P)} for _ in tan_in]
    ka = len(adj_in)
    for p in range(P):
        sys_ = GM.assemble(geo, p, perm, dmag, bool(neu[p]))
        if sys_ is None:
            continue
        A64, c64, rows, cells = sys_
        ne, eb = len(cells), geo.esup_ptr[p]
        m, nc = A64.shape
        F = qr(A64, dtype)
        if F.singular:
            continue
        c = c64.astype(dtype)
        ct = F.qt(c)
        y = F.r_solve(ct[:nc])
        ct[:nc] = 0
        r = F.q(ct)
        rho = r @ r
        with np.errstate(all="ignore"):
            w = r[:ne] / rho
        if not (rho > 0) or not np.all(np.isfinite(w)):
            continue
        nws = w[ne - 1] if neu[p] else dtype(0)
        fwd["weights"][eb:eb + ne] = w + (nws if add_neumann else 0)
        fwd["neumann_ws"][p] = nws
        fwd["computed"][p] = True
        if not adj_in and not tan_in:
            continue
        I, B = _face_tables(rows, cells, dmag, dtype, rules)
        Y3 = y.reshape(ne, 3)
        picked = I["PICK"] >= 0
        # ---- the right-hand sides of the second pass: rbar per adjoint, z1 = dA y per tangent (z2 = dA^T r kept beside it)
        rhs = Z(m, ka + len(tan_in))
        for j, (ghat, gnws) in enumerate(adj_in):
            g = Z(m)
            g[:ne] = ghat[eb:eb + ne]
            if neu[p]:
                if add_neumann:
                    g[ne - 1] += ghat[eb:eb + ne].sum()
                if gnws is not None:
                    g[ne - 1] += gnws[p]
            rhs[:, j] = g / rho - 2 * (g @ r) * r / (rho * rho)
        z2s = Z(nc, len(tan_in))
        for t, (dK, ddm) in enumerate(tan_in):
            kna = np.einsum("rij,rj->ri", dK[cells[I["IA"]]], I["N"])             # dK_a N, dK_b N per internal face
            knb = np.einsum("rij,rj->ri", dK[cells[I["IB"]]], I["N"])
            knn = np.einsum("rij,rj->ri", dK[cells[B["IA"]]], B["N"])             # ... and per Neumann boundary face
            dtau = Z(len(picked))
            dtau[picked] = I["coef"][picked] * ddm[cells[I["PICK"][picked]]]
            z1 = Z(m)
            z1[I["T"]] = (knb * Y3[I["IB"]]).sum(axis=1) - (kna * Y3[I["IA"]]).sum(axis=1)
            z1[I["T"] + 2] = dtau * (I["U"] * (Y3[I["IB"]] - Y3[I["IA"]])).sum(axis=1)
            z1[B["T"]] = -(knn * Y3[B["IA"]]).sum(axis=1)
            z2 = Z(ne, 3)
            rT, rT2 = r[I["T"]][:, None], (dtau * r[I["T"] + 2])[:, None]
            np.add.at(z2, I["IA"], -(kna * rT) - rT2 * I["U"])
            np.add.at(z2, I["IB"], knb * rT + rT2 * I["U"])
            np.add.at(z2, B["IA"], -(knn * r[B["T"]][:, None]))
            rhs[:, ka + t] = z1
            z2s[:, t] = z2.reshape(-1)
        # ---- Q^T of all of them at once; s = R^-1 top (adjoint), x = R^-T z2 (tangent); Q [0; tail] and Q [x; tail]
        qt = F.qt(rhs)
        S = F.r_solve(qt[:nc, :ka]) if ka else Z(nc, 0)
        qt[:nc, :ka] = 0
        if tan_in:
            qt[:nc, ka:] = F.rt_solve(z2s)
        back = F.q(qt)
        for j in range(ka):
            q, S3, o = back[:, j], S[:, j].reshape(ne, 3), adj[j]
            ab = lambda T, Ic: -(q[T][:, None] * Y3[Ic]) - r[T][:, None] * S3[Ic]   # noqa: E731  (Abar(t, 3 Ic + 0..2))
            for T, Ic, N, sign in ((I["T"], I["IA"], I["N"], -1), (I["T"], I["IB"], I["N"], +1), (B["T"], B["IA"], B["N"], -1)):
                term = (sign * ab(T, Ic)[:, :, None] * N[:, None, :]).reshape(-1, 9)
                np.add.at(o["grad_perm"], cells[Ic], term)
                np.add.at(o["sp"], cells[Ic], np.abs(term))
            T2 = I["T"] + 2
            term = ((ab(T2, I["IB"]) - ab(T2, I["IA"])) * I["U"]).sum(axis=1) * I["coef"]
            np.add.at(o["grad_diff_mag"], cells[I["PICK"][picked]], term[picked])
            np.add.at(o["scale_diff_mag"], cells[I["PICK"][picked]], np.abs(term[picked]))
        for t in range(len(tan_in)):
            dr = -back[:, ka + t]
            drho = 2 * (r @ dr)
            dw = dr[:ne] / rho - r[:ne] * drho / (rho * rho)
            dnws = dw[ne - 1] if neu[p] else dtype(0)
            tan[t]["tangent"][eb:eb + ne] = dw + (dnws if add_neumann else 0)
            tan[t]["tangent_neumann_ws"][p] = dnws
            tan[t]["scale"][p] = (np.abs(dr[:ne]) / rho + np.abs(r[:ne]) * abs(drho) / (rho * rho)).max() + abs(dnws)
    afold = np.abs(fold)
    for o in adj:
        o["scale_perm"] = o.pop("sp").max(axis=1)
        o["folded"] = o["grad_perm"].copy()
        with np.errstate(invalid="ignore"):                                   # (a mutant's factor may be infinite where tr = 3)
            t = o["grad_diff_mag"] * fold
            for d in (0, 4, 8):
                o["folded"][:, d] += t
            o["scale_folded"] = o["scale_perm"] + o["scale_diff_mag"] * afold
        o.update(fwd)
    for o in tan:
        o.update(fwd)
    return fwd, adj, tan


def adjoint(grid, perm, diff_mag, flag, grad_csr, grad_neumann_ws=None, add_neumann=True, dtype=LD, rules=STANDARD):
    """gls_adjoint_model's answer (the same keys, the same scales, and folded / scale_folded) through the QR, in dtype"""
    return derivatives(grid, perm, diff_mag, flag, adjoints=[(grad_csr, grad_neumann_ws)], add_neumann=add_neumann, dtype=dtype,
                       rules=rules)[1][0]


def tangent(grid, perm, diff_mag, flag, dK, ddm=None, add_neumann=True, dtype=LD, rules=STANDARD):
    """gls_tangent_model's answer (the same keys, the same scale) through the QR, in dtype"""
    return derivatives(grid, perm, diff_mag, flag, tangents=[(dK, ddm)], add_neumann=add_neumann, dtype=dtype, rules=rules)[2][0]


def _rows(grid):
    ptr = np.asarray(grid.esup_ptr).astype(np.int64)
    return ptr, np.asarray(grid.esup).astype(np.int64), np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def cotangent(grid, u, v, b, dtype):
    """(grad_csr, grad_neumann_ws) of J^T v: v_p u[esup[pos]] and v b (gls_jacobian_model.vjp_model), the products taken in dtype"""
    _, esup, rows = _rows(grid)
    u, v = np.asarray(u, dtype=dtype), np.asarray(v, dtype=dtype)
    return v[rows] * u[esup], None if b is None else v * np.asarray(b, dtype=dtype)


def jvp_of(grid, tan, u, b, dtype):
    """J . dK from a tangent dict (add_neumann = True): `value` [P] and `scale` [P] as gls_jacobian_model.jvp_model forms them"""
    ptr, esup, rows = _rows(grid)
    P = len(ptr) - 1
    u = np.asarray(u, dtype=dtype)
    value, room = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
    np.add.at(value, rows, np.asarray(tan["tangent"], dtype=dtype) * u[esup])
    np.add.at(room, rows, np.abs(u[esup]))
    if b is not None:
        b = np.asarray(b, dtype=dtype)
        value = value + np.asarray(tan["tangent_neumann_ws"], dtype=dtype) * b
        room = room + np.abs(b)
    return {"value": value, "scale": np.asarray(tan["scale"], dtype=dtype) * room}


def jvp(grid, perm, diff_mag, flag, u, dK, b=None, ddm=None, dtype=LD, rules=STANDARD):
    return jvp_of(grid, tangent(grid, perm, diff_mag, flag, dK, ddm, True, dtype, rules), u, b, dtype)


def vjp(grid, perm, diff_mag, flag, u, v, b=None, dtype=LD, rules=STANDARD):
    g, gn = cotangent(grid, u, v, b, dtype)
    return adjoint(grid, perm, diff_mag, flag, g, gn, True, dtype, rules)


def direction(B, dtheta, dtype):
    """dK [E][9] = sum_m dtheta[e][m] B[e][m], in dtype"""
    B = np.asarray(B, dtype=dtype)
    return np.einsum("emk,em->ek", B, np.asarray(dtheta, dtype=dtype).reshape(B.shape[:2]))


def reduced_vjp_of(adj, B, dtype):
    """J_theta^T v from an adjoint dict: `grad_theta` [E][M] = <B_(e,m), folded_e> and `scale` [E][M] = sum_k |B_(e,m)[k]| scale_folded_e
    (gls_reduced_jacobian_model.vjp_model)"""
    B = np.asarray(B, dtype=dtype)
    return {"grad_theta": np.einsum("emk,ek->em", B, np.asarray(adj["folded"], dtype=dtype)),
            "scale": np.abs(B).sum(axis=2) * np.asarray(adj["scale_folded"], dtype=dtype)[:, None]}


def reduced_jvp(grid, perm, diff_mag, flag, u, B, dtheta, b=None, dtype=LD, rules=STANDARD):
    return jvp(grid, perm, diff_mag, flag, u, direction(B, dtheta, dtype), b, None, dtype, rules)


def reduced_vjp(grid, perm, diff_mag, flag, u, B, v, b=None, dtype=LD, rules=STANDARD):
    return reduced_vjp_of(vjp(grid, perm, diff_mag, flag, u, v, b, dtype, rules), B, dtype)


# ---- distances: always on the scale of the 80-bit model ---------------------------------------------------------------------------

def dist(got, exact, scale):
    """max over the leading axis of max|got - exact| / scale (got, exact [n] or [n][k]; scale [n] or the shape of got).  Where the
    scale is 0 the exact value is 0 and got must be exactly 0: otherwise inf.  A value that is not finite: inf."""
    got, exact, scale = np.asarray(got, dtype=LD), np.asarray(exact, dtype=LD), np.asarray(scale, dtype=LD)
    if not np.all(np.isfinite(got)):
        return float("inf")
    d = np.abs(got - exact)
    if scale.ndim < d.ndim:
        d = d.reshape(len(scale), -1).max(axis=1)
    none = scale == 0
    if d[none].any():
        return float("inf")
    return float((d[~none] / scale[~none]).max()) if (~none).any() else 0.0


def adjoint_dist(got, exact):
    """{output: distance} of an adjoint dict (or any mapping with these keys) from the 80-bit one"""
    out = {}
    for key, sk in (("grad_perm", "scale_perm"), ("grad_diff_mag", "scale_diff_mag"), ("folded", "scale_folded")):
        if key in got and got[key] is not None:
            out[key] = dist(got[key], exact[key], exact[sk])
    return out


def tangent_dist(grid, got, got_nws, exact):
    """a tangent (csr [nnz_esup], neumann_ws [P] or None) from the 80-bit one, per row on the row's scale"""
    _, _, rows = _rows(grid)
    got = np.asarray(got, dtype=LD)
    if not np.all(np.isfinite(got)) or (got_nws is not None and not np.all(np.isfinite(got_nws))):
        return float("inf")
    d = np.zeros(len(exact["scale"]), dtype=LD)
    np.maximum.at(d, rows, np.abs(got - exact["tangent"]))
    if got_nws is not None:
        d = np.maximum(d, np.abs(np.asarray(got_nws, dtype=LD) - exact["tangent_neumann_ws"]))
    return dist(d, np.zeros_like(d), exact["scale"])


# ---- the cases (tests/test_gls_derivative_exact.py on the CPU, tests/test_gpu_gls_derivative_exact.py on the device) ----------------

NEUMANN_PLANE = (2, 0.0)
SEED = 3
TENSORS = ("ALH", "FAN", "LIN")      # LIN: tr K = 3, diff_mag == 0 on every cell -- eta is taken from nobody; FAN: one constant
#                                      tensor, every face a tie at diff_mag = 0.998, cond(K) = 3e3
TRANSFORMS = tuple(t for t in X.TRANSFORMS if t != "scale_1e-3")
# Out of the set by the decision that set this table up: a prototype restatement of the adjoint measured 2.0e-8 to 2.7e-8 from exact on
# scale_1e-3 and 5.6e-8 on delaunay / FAN, beyond CASE_CAP.  This module's restatement is closer there (`python
# tests/gls_derivative_exact.py` prints every case, these included):
#   scale_1e-3      adjoint 5.8e-11 to 1.2e-10, tangent up to 1.5e-9 (tet), and the 80-bit duality gap itself reaches 5e-17 of the
#                   sum of the absolute terms, forty times the worst case of the set: |U| ~ 1e-4 and ln|U| ~ -9 in every tau row
#   delaunay / FAN  adjoint 1.0e-10 (grad_perm) to 3.2e-9 (grad_diff_mag): rows of up to 65 cells at cond(K) = 3e3
# They stay out all the same; putting them in is a decision of its own, with its own device measurement.
LEFT_OUT = (("hex", None, "scale_1e-3"), ("tet", None, "scale_1e-3"), ("mixed", None, "scale_1e-3"), ("delaunay", "FAN", None))
TRANSFORM_MESHES = ("hex", "tet", "mixed")
UNIT_ALH = ("hex/ALH", "tet/ALH", "mixed/ALH", "delaunay/ALH")


def _table():
    t = {}
    for mesh in TRANSFORM_MESHES:
        for tensor in TENSORS:
            t[f"{mesh}/{tensor}"] = (mesh, tensor, None)
    for mesh in TRANSFORM_MESHES:
        for tr in TRANSFORMS:
            t[f"{mesh}/{tr}"] = (mesh, None, tr)
    t["delaunay/ALH"] = ("delaunay", "ALH", None)        # populates every bin of the kernel
    return t


CASES = _table()
# the reduced Jacobian: M = 3 on every case, M = 1 and 6 on these
REDUCED_ALL_M = tuple(k for k in CASES if k.startswith("hex/") and CASES[k][2] is None) + ("delaunay/ALH",)
REDUCED_BASES = {1: "scale", 3: "percell3", 6: "symmetric"}     # of tests/test_gpu_gls_reduced_jacobian.py's Reduced.bases


def case_mesh(mesh, tensor, transform):
    from ninpol_amd import mesh as M
    from test_gpu_gls_tangent import MESHES
    if transform is not None:
        return X.transformed_mesh(mesh, transform, factory=(MESHES[mesh], NEUMANN_PLANE), seed=SEED)
    return M.attach_fields(MESHES[mesh](), "u", perm=tensor, neumann_plane=NEUMANN_PLANE, seed=SEED)


class Problem:
    """One case: the mesh in an Interpolator (on a device or not), its tables on the host, seeded inputs for every surface, and the
    80-bit model and the float64 restatement of all of them -- one pass over the nodes per format, computed once."""

    def __init__(self, name, spec=None):
        import ninpol_amd
        from test_gpu_gls_reduced_jacobian import Reduced
        self.name = name
        self.spec = spec or CASES[name]
        self.I = I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=case_mesh(*self.spec))
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        perm, dmag = I._perm_rows()
        self.perm, self.dmag = np.array(perm).reshape(self.E, 9), np.array(dmag)
        self.flag = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        self.ptr, self.esup, self.rows = _rows(g)
        rng = np.random.default_rng(17)
        self.ghat, self.gnws = rng.uniform(-1.0, 1.0, self.nnz), rng.uniform(-1.0, 1.0, self.P)
        self.dK = np.random.default_rng(1).uniform(-1, 1, (self.E, 9))
        self.ddm = np.random.default_rng(2).uniform(-1, 1, self.E)
        rng = np.random.default_rng(23)
        self.u, self.b, self.v = rng.uniform(-1.0, 1.0, self.E), rng.uniform(-1.0, 1.0, self.P), rng.uniform(-1, 1, self.P)
        self.reduced = Reduced(self)                                    # its bases and directions in theta (it reads E and perm)
        self.Ms = (1, 3, 6) if (name in REDUCED_ALL_M or self.spec[0] == "delaunay") else (3,)
        self._runs = {}

    def B(self, M):
        return np.ascontiguousarray(self.reduced.B(REDUCED_BASES[M]))

    def dtheta(self, M):
        return self.reduced.dtheta[REDUCED_BASES[M]][0]

    def run(self, dtype=LD, rules=STANDARD, reduced=True):
        """{surface: dict} in dtype: "backward" (adjoint of ghat, gnws), "vjp" (adjoint of v u, v b), "tangent" / "tangent_explicit",
        "jvp" / "jvp_explicit", and per M "rjvp<M>" / "rvjp<M>" """
        key = (dtype, rules, reduced)
        if key in self._runs:
            return self._runs[key]
        Ms = self.Ms if reduced else ()
        tangents = [(self.dK, None), (self.dK, self.ddm)] + [(direction(self.B(M), self.dtheta(M), dtype), None) for M in Ms]
        adjoints = [(self.ghat, self.gnws), cotangent(self.grid, self.u, self.v, self.b, dtype)]
        _, adj, tan = derivatives(self.grid, self.perm, self.dmag, self.flag, adjoints, tangents, True, dtype, rules)
        out = {"backward": adj[0], "vjp": adj[1], "tangent": tan[0], "tangent_explicit": tan[1],
               "jvp": jvp_of(self.grid, tan[0], self.u, self.b, dtype), "jvp_explicit": jvp_of(self.grid, tan[1], self.u, self.b, dtype)}
        for i, M in enumerate(Ms):
            out[f"rjvp{M}"] = jvp_of(self.grid, tan[2 + i], self.u, self.b, dtype)
            out[f"rvjp{M}"] = reduced_vjp_of(adj[1], self.B(M), dtype)
        self._runs[key] = out
        return out

    def distances(self, got, exact=None):
        """{(surface, output): distance from the 80-bit model} of a run()-shaped dict (the float64 restatement, a mutant)"""
        exact = exact or self.run(LD)
        out = {}
        for s, o in got.items():
            e = exact[s]
            if s in ("backward", "vjp"):
                for k, d in adjoint_dist(o, e).items():
                    out[(s, k)] = d
            elif s.startswith("tangent"):
                out[(s, "tangent")] = tangent_dist(self.grid, o["tangent"], o["tangent_neumann_ws"], e)
            elif s.startswith("rvjp"):
                out[(s, "grad_theta")] = dist(o["grad_theta"], e["grad_theta"], e["scale"])
            else:
                out[(s, "value")] = dist(o["value"], e["value"], e["scale"])
        return out


if __name__ == "__main__":          # the table: every case, and the ones left out, every output of the float64 restatement
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    specs = dict(CASES)
    specs.update({"left out: " + "/".join(str(x) for x in s if x): s for s in LEFT_OUT})
    for name, spec in specs.items():
        pb = Problem(name, spec)
        for (s, o), v in pb.distances(pb.run(np.float64)).items():
            print(f"{name} {s} {o}: restatement {v:.2e}")
