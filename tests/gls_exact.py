"""The high-precision yardstick of the GLS tests: a node's least-squares problem -- the float64 matrix M_v exactly as the
reference assembles it (gls.pyx:252-416) -- solved in 80-bit extended precision (numpy longdouble Householder QR, eps = 1.1e-19)
and rounded to float64.  system() and last_row_of_pinv() are the code that made tests/golden/pins/fan_exact.npz
(tests/golden/make_fan_exact.py imports them from here; tests/test_gls_exact.py recomputes pinned rows bit for bit).

A float64 QR -- the reference's dgels, the C restatement, every HIP kernel -- is ~cond(M_v) * eps away from this solution, and
how far the reference itself is away is the measure of what a correct kernel may be: tests/test_gls_exact.py (the yardstick
itself, CPU) and tests/test_gpu_gls_exact.py (every kernel of the launch plan held to it).

Plain numpy: needs nothing but a grid (the oracle's attribute bag or ninpol_amd's Grid: same names) and the field rows."""
import numpy as np

LD = np.longdouble
# x87 extended precision (64-bit significand); both the development and the GPU machines are x86.  With a longdouble that is
# only a float64 the "exact" rows would be one more float64 QR and every bar built on them meaningless: an error, not a skip.
assert np.finfo(LD).eps < 2e-19, "numpy longdouble is not 80-bit extended precision here"


def system(p, G, perm, dmag, flag):
    """M_v as the reference assembles it (gls.pyx:252-416), float64 arithmetic in the reference's operation order;
    returns (M, n_elem) -- the weights are row n-1 of pinv(M) restricted to the cell rows."""
    cells = G.esup[G.esup_ptr[p]:G.esup_ptr[p + 1]]
    faces = G.fsup[G.fsup_ptr[p]:G.fsup_ptr[p + 1]]
    loc = {int(c): i for i, c in enumerate(cells)}
    ne, nf = len(cells), len(faces)
    bfaces = [f for f in faces if G.boundary_faces[f] == 1]
    m = ne + 3 * nf + len(bfaces)
    Mi = np.zeros((m, 3 * ne + 1))
    xv = G.point_coords[p]
    for e, c in enumerate(cells):
        Mi[e, 3 * e:3 * e + 3] = G.centroids[c] - xv
        Mi[e, -1] = 1.0
    row = ne
    for f in faces:
        a, b = G.esuf_ptr[f], G.esuf_ptr[f + 1]
        if b - a < 2:
            continue
        ca, cb = int(G.esuf[a]), int(G.esuf[a + 1])
        N = G.normal_faces[f]
        T = xv - G.faces_centers[f]
        U = np.array([N[1] * T[2] - N[2] * T[1], N[2] * T[0] - N[0] * T[2], N[0] * T[1] - N[1] * T[0]])
        eta = max(0.0, dmag[ca], dmag[cb])
        tau = np.sqrt(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]) ** (-eta)
        Ka, Kb = perm[ca].reshape(3, 3), perm[cb].reshape(3, 3)
        kna = np.array([Ka[r, 0] * N[0] + Ka[r, 1] * N[1] + Ka[r, 2] * N[2] for r in range(3)])
        knb = np.array([Kb[r, 0] * N[0] + Kb[r, 1] * N[1] + Kb[r, 2] * N[2] for r in range(3)])
        for k, (va, vb) in enumerate(((kna, knb), (T, T), (tau * U, tau * U))):
            Mi[row + k, 3 * loc[ca]:3 * loc[ca] + 3] = -va
            Mi[row + k, 3 * loc[cb]:3 * loc[cb] + 3] = vb
        row += 3
    if flag[p]:
        start = ne + 3 * nf
        for i, f in enumerate(bfaces):
            c0 = int(G.esuf[G.esuf_ptr[f]])
            K0 = perm[c0].reshape(3, 3)
            N = G.normal_faces[f]
            Mi[start + i, 3 * loc[c0]:3 * loc[c0] + 3] = [-(K0[r, 0] * N[0] + K0[r, 1] * N[1] + K0[r, 2] * N[2]) for r in range(3)]
    return Mi, ne


def last_row_of_pinv(Mi, ne):
    """Row n-1 of the least-squares solution of M X = [I_ne; 0] in extended precision (Householder QR, full column rank)."""
    A = Mi.astype(LD)
    m, n = A.shape
    B = np.zeros((m, ne), dtype=LD)
    B[:ne, :ne] = np.eye(ne, dtype=LD)
    for k in range(n):
        x = A[k:, k].copy()
        nx = np.sqrt((x * x).sum())
        if nx == 0:
            raise ZeroDivisionError("rank deficient")
        beta = -np.copysign(nx, x[0])
        v = x.copy()
        v[0] -= beta
        g = LD(1) / (v * v).sum() * 2
        A[k:, k:] -= np.outer(v, g * (v @ A[k:, k:]))
        B[k:, :] -= np.outer(v, g * (v @ B[k:, :]))
    return np.asarray(B[n - 1, :] / A[n - 1, n - 1], dtype=np.float64)   # back-substitution's first step IS row n-1


def fields(oracle_interp, mesh, variable):
    """(perm[E, 9], diff_mag[E], flag[P] as bool): the field rows system() reads, taken from a loaded OracleInterpolator and the
    mesh's Neumann flags the way make_fan_exact.py takes them."""
    G = oracle_interp.grid
    v2i = oracle_interp.variable_to_index
    perm = oracle_interp.cells_data[v2i["cells"]["permeability"]][:G.n_elems * 9].reshape(-1, 9)
    dmag = oracle_interp.cells_data[v2i["cells"]["diff_mag"]][:G.n_elems]
    flag = np.asarray(mesh.point_data["neumann_flag_" + variable]).astype(bool)
    return perm, dmag, flag


def exact_rows(oracle_interp, mesh, variable, nodes, tau_scale=None):
    """The exact weight rows of `nodes`: (exact[len(nodes), MX_ELEMENTS_PER_POINT], ok[len(nodes)]).  ok is False -- and the row
    zero -- where the extended-precision QR meets a zero column or gives a non-finite result (the degenerate set of the parity
    contract: those systems have no unique solution to be held to).
    tau_scale (tests of the yardstick's own resolution only): the tau.U rows of every system multiplied by it."""
    G = oracle_interp.grid
    perm, dmag, flag = fields(oracle_interp, mesh, variable)
    nodes = np.asarray(nodes, dtype=np.int64)
    exact = np.zeros((len(nodes), int(G.MX_ELEMENTS_PER_POINT)))
    ok = np.zeros(len(nodes), dtype=bool)
    for i, p in enumerate(nodes):
        Mi, ne = system(int(p), G, perm, dmag, flag)
        if tau_scale is not None:
            _scale_tau_rows(Mi, int(p), G, ne, tau_scale)
        try:
            with np.errstate(all="ignore"):
                row = last_row_of_pinv(Mi, ne)
        except ZeroDivisionError:
            continue
        if np.isfinite(row).all():
            exact[i, :ne] = row
            ok[i] = True
    return exact, ok


def _scale_tau_rows(Mi, p, G, ne, s):
    """tau -> tau * s in an assembled system: the third row of every internal face's triple (system() packs the triples from
    row ne on, in fsup order, internal faces only)."""
    row = ne
    for f in G.fsup[G.fsup_ptr[p]:G.fsup_ptr[p + 1]]:
        if G.esuf_ptr[f + 1] - G.esuf_ptr[f] < 2:
            continue
        Mi[row + 2] *= s
        row += 3


def exact_neumann_ws(exact, ok, G, flag, nodes):
    """neumann_ws of the same nodes.  The reference stores the LAST CELL'S WEIGHT there (gls.pyx:470-472: row n-1 of the
    solution's column w_total - 1; oracle/ninpol_oracle.c does the same), so no second solve: exact[i, ne - 1] on flagged nodes,
    0 elsewhere."""
    nodes = np.asarray(nodes, dtype=np.int64)
    ne = np.asarray(G.esup_ptr)[nodes + 1] - np.asarray(G.esup_ptr)[nodes]
    nws = np.zeros(len(nodes))
    on = np.asarray(flag)[nodes].astype(bool) & np.asarray(ok)
    nws[on] = exact[np.flatnonzero(on), ne[on] - 1]
    return nws


def dist(w, exact):
    """The worst row of |w - exact| / max|exact_row|: the scale util.rowscaled_err uses (a row of zeros counts absolutely).
    For 1-D input (neumann_ws) pass the rows' scales yourself: dist_scaled."""
    w, exact = np.asarray(w, dtype=float), np.asarray(exact, dtype=float)
    assert w.shape == exact.shape and w.ndim == 2
    if w.size == 0:
        return 0.0
    assert np.isfinite(w).all(), "non-finite weights"
    return dist_scaled(np.abs(w - exact).max(axis=1), exact)


def dist_scaled(absdiff, exact):
    """max over rows of absdiff[row] / max|exact_row|: neumann_ws is one entry of its row and is measured on the row's scale."""
    scale = np.abs(np.asarray(exact, dtype=float)).max(axis=1)
    scale = np.where(scale == 0, 1.0, scale)
    absdiff = np.asarray(absdiff, dtype=float)
    assert np.isfinite(absdiff).all(), "non-finite values"
    return float((absdiff / scale).max()) if len(absdiff) else 0.0


# ---- the cases both test files run (tests/test_gls_exact.py: the oracle's own distance; tests/test_gpu_gls_exact.py: the kernels) ----

TENSORS = ("ALH", "FAN")


def unit_cases():
    """name -> (mesh factory, Neumann plane): small single-family meshes on the unit box, each run with the ALH and the FAN
    tensor.  Between them every kernel of the launch plan that the default routing can produce owns sampled nodes
    (tests/test_gpu_gls_exact.py asserts it from the plans)."""
    from ninpol_amd import mesh as M
    return {
        "hex8": (lambda: M.hex_mesh(8, jitter=0.15, seed=0), (2, 0.0)),
        "tet5": (lambda: M.tet_mesh(5, jitter=0.1, seed=1), (2, 0.0)),
        "wedge5": (lambda: M.wedge_mesh(5, jitter=0.05, seed=2), (2, 0.0)),
        "mixed844": (lambda: M.mixed_mesh(8, 4, 4, jitter=0.1, seed=3), (2, 0.0)),
        "delaunay_tet8_random": (lambda: M.delaunay_tet_mesh(8, seed=9, lattice="random"), (2, 0.0)),      # up to 48 cells a node
        "delaunay_wedge12x6_random": (lambda: M.delaunay_wedge_mesh(12, 6, seed=6, lattice="random"), (2, 0.0)),
        "wedge_fan50x2": (lambda: M.wedge_fan(50, 2, jitter=0.02, seed=50), (2, 0.0)),                     # 100 cells: global scratch
        "hex987_side": (lambda: M.hex_mesh(9, 8, 7, jitter=0.15), (0, 0.0)),                               # quad4, small*
        "delaunay_tet8_bcc": (lambda: M.delaunay_tet_mesh(8, seed=2), (2, 0.0)),                           # mfx_7x12, mfx_boundary
        "delaunay_tet10_random": (lambda: M.delaunay_tet_mesh(10, seed=4, lattice="random"), (2, 0.0)),    # mfg_tiles
        "wedge_fan30x3": (lambda: M.wedge_fan(30, 3), (2, 0.0)),                                           # the block kernel's wide slots
        # (the smallest cloud found whose Neumann plane holds a node the wide kernel's boundary list refuses: 15 cells -> block2)
        "delaunay_tet7_random": (lambda: M.delaunay_tet_mesh(7, seed=7, lattice="random"), (2, 0.0)),
    }


def unit_mesh(name, perm):
    from ninpol_amd import mesh as M
    make, plane = unit_cases()[name]
    return M.attach_fields(make(), "u", perm=perm, neumann_plane=plane, seed=7)


# Off the unit box and beyond eta = 1.  Fields are attached on the unit mesh (K and the flags are then fixed), then
# points <- points * A + b; or the LIN tensor scaled down: diff_mag = (1 - 3 / tr K)^2, so a small K drives eta past 1.
# (LIN x 0.2 gives eta = 16 and a numerically singular system -- the oracle itself is 100 % away from exact there: outside the
# parity set and not a case.)
TRANSFORMS = {
    "scale_1e-3": dict(A=(1e-3, 1e-3, 1e-3)),
    "scale_1e3": dict(A=(1e3, 1e3, 1e3)),
    "stretch_1_10_100": dict(A=(1.0, 10.0, 100.0)),
    "squash_z_0.01": dict(A=(1.0, 1.0, 0.01)),
    "offset_100": dict(b=(100.0, -100.0, 100.0)),
    "offset_1e4": dict(b=(1e4, 1e4, 1e4)),
    "lin_x0.45_eta1.49": dict(lin=0.45),
    "lin_x0.36_eta3.16": dict(lin=0.36),
}
TRANSFORM_MESHES = ("hex8", "tet5", "mixed844")


def transformed_mesh(name, transform, factory=None, seed=7):
    """unit_cases()[name] under TRANSFORMS[transform]; factory: a (mesh factory, Neumann plane) pair of the caller's own instead of
    the unit case's (tests/gls_derivative_exact.py: the meshes of the derivative tests), seed: attach_fields' """
    from ninpol_amd import mesh as M
    t = TRANSFORMS[transform]
    make, plane = unit_cases()[name] if factory is None else factory
    m = M.attach_fields(make(), "u", perm="LIN" if "lin" in t else "ALH", neumann_plane=plane, seed=seed)
    if "lin" in t:
        m.cell_data["permeability"] = [np.ascontiguousarray(k * t["lin"]) for k in m.cell_data["permeability"]]
    m.points = np.ascontiguousarray(m.points * np.asarray(t.get("A", (1.0, 1.0, 1.0))) + np.asarray(t.get("b", (0.0, 0.0, 0.0))))
    return m


def computed_nodes(G, flag):
    """the nodes GLS computes a row for: interior nodes and flagged (Neumann) boundary nodes"""
    return np.flatnonzero(~(np.asarray(G.boundary_points).astype(bool) & ~np.asarray(flag).astype(bool)))


def sample_nodes(candidates, G, label, total=32, top=8):
    """A seeded sample of `candidates` (node ids): all of them up to `total`; beyond that the `top` with the most cells (ties: the
    lowest ids) and a random draw of the rest, seeded by `label` alone -- the same nodes on every machine and in every run.
    Interior and Neumann nodes are drawn alike."""
    import zlib
    cand = np.sort(np.asarray(candidates, dtype=np.int64))
    if len(cand) <= total:
        return cand
    deg = np.diff(np.asarray(G.esup_ptr))[cand]
    order = np.argsort(-deg, kind="stable")
    head, rest = cand[order[:top]], cand[order[top:]]
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    return np.sort(np.concatenate([head, rng.choice(rest, total - top, replace=False)]))
