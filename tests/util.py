"""Shared helpers for the test-suite (golden loading, tolerances)."""
import glob
import os

import numpy as np

from ninpol_amd import mesh as M

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the reference's outputs on the meshes of test_port_matches_reference / test_edges_match_reference (not golden cases)
REFERENCE_OUTPUTS_DIR = os.path.join(GOLDEN_DIR, "reference_outputs")
GOLDEN_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))

GRID_ARRAYS = ("esup", "esup_ptr", "psup", "psup_ptr", "fsup", "fsup_ptr", "esuf", "esuf_ptr", "esuel",
               "infael", "inpofa", "inpoel", "boundary_faces", "boundary_points", "point_coords",
               "centroids", "faces_centers", "normal_faces", "faces_areas")
GRID_SCALARS = ("dim", "n_elems", "n_points", "n_faces", "MX_ELEMENTS_PER_POINT", "MX_POINTS_PER_POINT",
                "MX_ELEMENTS_PER_FACE", "MX_FACES_PER_POINT")

# north_star: "within 1e-10 relative for the float64 weights".  Weights of one node are O(1/n_elem)
# and sum to ~1, so the error is measured relative to the largest weight of the row.
WEIGHT_RTOL = 1e-10

# The reference's own FAN tensor (tests/utils/analytical.py:285-293; cond(K) = 3.0e3) makes the GLS matrix M_v
# ill-conditioned: cond(M_v) = 7e4 on hex 8^3, 3e5 on 32^3, ~6e5 on 64^3 (tools/gls_condition.py; it grows like 1/h:
# the K.N rows do not scale with the mesh, the d / T / U rows do).  Every correct float64 QR is then ~cond * eps away
# from the exact least-squares solution -- THE REFERENCE INCLUDED: measured in the dev container on
# hex_mesh(n, jitter=0.15, seed=0), Neumann plane z = 0, row-scaled like WEIGHT_RTOL (tests/golden/make_fan_exact.py;
# `exact` = the same float64 matrix solved in 80-bit arithmetic):
#     n    reference vs exact    C restatement vs exact    restatement vs reference (all nodes)
#     32   4.1e-11               3.6e-11                   8.0e-11
#     64   9.0e-11               1.07e-10                  1.85e-10
# Two such codes can differ by the SUM of their distances.  So on this case only:
#   * test_gpu_gls_fan_exact_sample holds the HIP path to "no further from exact than FAN_EXACT_SLACK x the reference's
#     own distance" on the committed sample (tests/golden/pins/fan_exact.npz), never looser than that and never tighter
#     than the global bar;
#   * the all-node comparison with the C restatement uses FAN_RTOL[n] (64^3: 3e-10 = the two distances, rounded up).
# Every other case keeps WEIGHT_RTOL.
FAN_RTOL = {32: 1e-10, 64: 3e-10}
FAN_EXACT_SLACK = 1.5


def fan_rtol(n):
    return max(WEIGHT_RTOL, FAN_RTOL[n])


def load_fan_exact():
    return np.load(os.path.join(GOLDEN_DIR, "pins", "fan_exact.npz"), allow_pickle=False)


def flat_mesh(kind, n=5, jitter=0.12, seed=3):
    """Degenerate class (iii) of the GLS parity set: a jittered 3-D mesh squashed into the plane
    z = 0.  Cells keep their 3-D types and every face stays a non-degenerate polygon IN the plane, so all normals are
    exactly (0, 0, +-1); with K = diag(1, 1, 0) the z-column of every cell is then zero altogether (d_z = 0, T_z = 0,
    (N x T)_z = 0, (K N)_z = 0): a pivot column that is zero at its step in every GLS kernel.  (K = 0 alone does not do
    it: the T and tau.U rows do not depend on K.)"""
    gen = {"hex": M.hex_mesh, "tet": M.tet_mesh, "wedge": M.wedge_mesh}.get(kind)
    m = gen(n, jitter=jitter, seed=seed) if gen else M.mixed_mesh(n + 3, n, n, jitter=jitter, seed=seed)
    M.attach_fields(m, "u", perm="LIN", neumann_plane=(0, 0.0), seed=seed)    # Neumann nodes: the plane x = 0 of the box
    # project along (-0.3, -0.2, 1): no box plane contains that direction, so boundary faces stay proper polygons too
    z = m.points[:, 2].copy()
    m.points = np.ascontiguousarray(m.points + np.outer(z, [0.3, 0.2, -1.0]))
    m.points[:, 2] = 0.0
    K = np.zeros((m.n_cells, 9))
    K[:, 0] = K[:, 4] = 1.0
    sizes = np.cumsum([0] + [len(c) for c in m.cells])
    m.cell_data["permeability"] = [K[sizes[b]:sizes[b + 1]] for b in range(len(m.cells))]
    return m


def load_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    nb = int(z["n_blocks"])
    cells = [M.CellBlock(str(z[f"block{b}_type"]), z[f"block{b}_data"]) for b in range(nb)]
    mesh = M.Mesh(z["points"], cells,
                  point_data={"neumann_flag_u": z["neumann_flag_u"], "neumann_u": z["neumann_u"]},
                  cell_data={"permeability": [z[f"permeability_block{b}"] for b in range(nb)],
                             "u": [z[f"u_block{b}"] for b in range(nb)]})
    return mesh, z


def assert_grid_equal(grid, z, prefix="grid_"):
    """bit-exact: integers AND geometry (centroids, face centres, float32 normals, areas)."""
    for k in GRID_SCALARS:
        assert int(getattr(grid, k)) == int(z[prefix + k]), k
    for k in GRID_ARRAYS:
        a = np.asarray(getattr(grid, k))
        b = z[prefix + k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=k)


def rowscaled_err(a, b):
    """max over rows of |a-b| / max|b_row| for dense (n, w) tables; NaNs must coincide."""
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN pattern differs"
    if a.size == 0:
        return 0.0
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin), "inf pattern differs"
    d = np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0)), 0.0)
    if a.ndim == 1:
        scale = max(np.abs(np.where(fin, b, 0.0)).max(), 1e-300)
        return float(d.max() / scale)
    scale = np.abs(np.where(fin, b, 0.0)).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    return float((d / scale).max())


# north_star says "within 1e-10 RELATIVE for the float64 weights".  Element-wise that can only be asked of entries that are not
# themselves rounding residue: a GLS row has signed weights, some of them orders of magnitude below the row's largest, and their
# absolute error is the row's (~cond * eps * max|w|).  So the bar of record stays row-scaled (WEIGHT_RTOL) and the ELEMENT-WISE
# relative error is measured beside it on every entry with |w| >= ELEMENTWISE_FLOOR * (largest weight of its row), and asserted:
# GLS <= ELEMENTWISE_RTOL_GLS (an entry at the floor may carry 1e3 x the row-scaled error), IDW / LS <= 1e-14.
ELEMENTWISE_FLOOR = 1e-3
ELEMENTWISE_RTOL_GLS = 1e-9
# (the reference's FAN tensor: the row-scaled distance itself is up to 1e-10 there -- see above -- and an entry at the floor
#  carries 1 / ELEMENTWISE_FLOOR of it: the element-wise figure is reported and held to what the row-scaled bar implies)
ELEMENTWISE_RTOL_GLS_FAN = 1e-7


def elementwise_rtol(meth, perm="ALH"):
    return 1e-14 if meth != "gls" else (ELEMENTWISE_RTOL_GLS_FAN if perm == "FAN" else ELEMENTWISE_RTOL_GLS)


def elementwise_err(a, b, floor=ELEMENTWISE_FLOOR):
    """max |a - b| / |b| over the entries with |b| >= floor * max|b_row| (dense (n, w) tables; finite entries only)."""
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    assert a.shape == b.shape
    if a.size == 0:
        return 0.0
    fin = np.isfinite(b) & np.isfinite(a)
    bb = np.where(fin, np.abs(b), 0.0)
    scale = bb.max(axis=1, keepdims=True) if a.ndim == 2 else bb.max()
    sel = fin & (bb >= floor * scale) & (bb > 0)
    if not sel.any():
        return 0.0
    return float((np.abs(a[sel] - b[sel]) / bb[sel]).max())


def csr_elementwise_err(W, indptr, indices, data, floor=ELEMENTWISE_FLOOR):
    """the same for a scipy CSR against (indptr, indices, data) of the same pattern."""
    a, b = np.asarray(W.data), np.asarray(data)
    if len(b) == 0:
        return 0.0
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    fin = np.isfinite(a) & np.isfinite(b)
    bb = np.where(fin, np.abs(b), 0.0)
    scale = np.zeros(len(indptr) - 1)
    np.maximum.at(scale, rows, bb)
    sel = fin & (bb >= floor * scale[rows]) & (bb > 0)
    if not sel.any():
        return 0.0
    return float((np.abs(a[sel] - b[sel]) / bb[sel]).max())


def csr_rowscaled_err(W, indptr, indices, data):
    """compare a scipy CSR with a golden (indptr, indices, data): pattern exact, values row-scaled."""
    np.testing.assert_array_equal(W.indptr, indptr)
    np.testing.assert_array_equal(W.indices, indices)
    assert W.indices.dtype == indices.dtype
    a, b = W.data, data
    assert np.array_equal(np.isnan(a), np.isnan(b))
    if len(b) == 0:
        return 0.0
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    bf = np.where(np.isfinite(b), np.abs(b), 0.0)
    scale = np.zeros(len(indptr) - 1)
    np.maximum.at(scale, rows, bf)
    scale[scale == 0] = 1.0
    d = np.where(np.isfinite(b), np.abs(np.nan_to_num(a) - np.nan_to_num(b)), 0.0)
    return float((d / scale[rows]).max())


# ---- composite meshes (mesh.composite_mesh): a part's rows of the union, in the part's own layout ---------------------------

def esup_csr(grid, w):
    """a dense (n_points, MX_ELEMENTS_PER_POINT) weight table in esup layout (entry j of row p belongs to cell
    esup[esup_ptr[p] + j]) as a scipy CSR (n_points, n_elems); explicit zeros are kept."""
    import scipy.sparse as sp
    ptr, esup = np.asarray(grid.esup_ptr), np.asarray(grid.esup)
    cnt = np.diff(ptr)
    rows = np.repeat(np.arange(len(cnt)), cnt)
    local = np.arange(len(esup)) - np.repeat(ptr[:-1], cnt)
    return sp.csr_matrix((np.asarray(w)[rows, local], esup, ptr), shape=(len(cnt), int(grid.n_elems)))


def part_table(W, part_grid, nodes, cells):
    """the rows of a composite mesh's weights W (scipy CSR over the composite's nodes and cells) that belong to one part, as a
    dense table in the PART's esup layout: row p, entry j = W[nodes[p], cells[c]] with c = esup[esup_ptr[p] + j] of the part's
    own grid.  (That the composite's cells around nodes[p] are exactly cells[...] of the part's is a grid property:
    test_composite.py checks it.)"""
    ptr, esup = np.asarray(part_grid.esup_ptr), np.asarray(part_grid.esup)
    cnt = np.diff(ptr)
    rows = np.repeat(np.arange(len(cnt)), cnt)
    local = np.arange(len(esup)) - np.repeat(ptr[:-1], cnt)
    W = W.tocsr()
    W.sort_indices()
    r, c = np.asarray(nodes)[rows], np.asarray(cells)[esup]
    # position of column c in row r of W (columns sorted inside each row)
    lo, hi = W.indptr[r], W.indptr[r + 1]
    key = r.astype(np.int64) * (int(W.shape[1]) + 1) + c
    flat = np.repeat(np.arange(W.shape[0], dtype=np.int64), np.diff(W.indptr)) * (int(W.shape[1]) + 1) + W.indices
    pos = np.searchsorted(flat, key)
    found = (pos < hi) & (pos >= lo)
    found[found] = W.indices[pos[found]] == c[found]
    out = np.zeros((len(cnt), int(part_grid.MX_ELEMENTS_PER_POINT)))
    out[rows[found], local[found]] = W.data[pos[found]]
    return out
