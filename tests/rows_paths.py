"""Meshes and models for the paths of the IDW / LS row kernels (csrc/kernels_idw_ls.hip) and of the row kernels behind interpolate()
and apply() (csrc/kernels_csr.hip) that no mesh of the GLS parity set reaches.  A helper module, not a test
module: tests/test_rows_paths.py pins on the CPU, with the oracle alone, that every mesh here does reach its path;
tests/test_gpu_rows_paths.py holds the kernels to the oracle on them.  Plain numpy and ninpol_amd.mesh.

Which mesh pins which path:
  fan_axis_first     a tile whose run of esup is longer than the LDS a wavefront owns: rows straight from / to HBM (`staged == false`)
  delaunay_small     tiles of 32 nodes, in the full launch and in the pieces of interpolate()'s pipeline
  flat_on_axis       LS's D == 0.0 fallback on rows of more than 8 cells (axis 0 and 1; axis 2 takes the planar branch: the control)
  tiny_tet           IDW's node-on-a-centroid branch, firing in the second and third chunk of 8 on some rows and not at all on others
"""
import numpy as np

from ninpol_amd import mesh as M

# the launch rule of launch_rows (kernels_idw_ls.hip) and apply_cap (kernels_csr.hip), restated by rows_tiling() below
CAP_SHORT, CAP_LONG = 1024, 1536


def all_flags_one(mesh, variable="u"):
    """every node carries the Neumann flag: no row is skipped as a Dirichlet boundary node (idw.pyx:62-63, ls.pyx:58-59)"""
    mesh.point_data["neumann_flag_" + variable] = np.ones(mesh.points.shape[0])
    return mesh


def fan_axis_first(sectors, layers, at, jitter=0.02, seed=1):
    """M.wedge_fan with its nodes renumbered: the non-axis nodes in their old order, and the layers + 1 axis nodes -- 2 * sectors cells
    each inside, sectors at the two ends -- as ONE consecutive block at position `at`.  (In wedge_fan's own order the axis nodes sit
    sectors + 1 ids apart: no tile holds more than two of them.)

    fan_axis_first(60, 16, at=70): 1037 nodes, longest row 120, mean row 5.55 -> cap 1536, tiles of 64; 17 tiles; tile 1 holds all 17
    axis nodes, 2108 entries: not staged; the 16 others are.  at=0: the long tile is tile 0, 2014 entries."""
    m = M.wedge_fan(sectors, layers, jitter=jitter, seed=seed)
    per = sectors + 1
    P = m.points.shape[0]
    old = np.arange(P)
    axis, rest = old[old % per == 0], old[old % per != 0]
    assert len(axis) == layers + 1 and 0 <= at <= len(rest)
    order = np.concatenate([rest[:at], axis, rest[at:]])      # order[new id] = old id
    new_id = np.empty(P, dtype=np.int64)
    new_id[order] = np.arange(P)
    return M.Mesh(np.ascontiguousarray(m.points[order]), [M.CellBlock(b.type, new_id[b.data]) for b in m.cells])


def fan_axis_nodes(layers, at):
    """the ids of fan_axis_first's axis nodes"""
    return np.arange(at, at + layers + 1)


def flat_on_axis(kind, n, axis):
    """util.flat_mesh's projection, onto the plane x[axis] = 0 instead of z = 0: a jittered 3-D mesh squashed along (0.3, 0.2, 0.25)
    with -1 at `axis` (no box plane contains that direction: every cell keeps a proper image).  Every node and every centroid has
    coordinate `axis` exactly 0, so LS's D is exactly 0 on every node for axis 0 and 1 (a zero row and column of the moment matrix:
    each product of its expansion has an exactly zero factor) -- the IDW fallback of ls.pyx:88-102 -- and for axis 2 the planar branch
    sets Izz = 1 first: the control.  Every node carries the Neumann flag, so no row is skipped.

    Counted with the oracle: ("tet", 5, 0) has 216 nodes, all 216 LS rows equal the normalised 1 / dist formula to 1e-12 and 160 of
    them have more than 8 cells; ("wedge", 5, 0) has 64 such long rows."""
    gen = {"hex": M.hex_mesh, "tet": M.tet_mesh, "wedge": M.wedge_mesh}[kind]
    m = gen(n, jitter=0.12, seed=3)
    M.attach_fields(m, "u", perm="LIN", neumann_plane=(0, 0.0), seed=3)
    d = np.array([0.3, 0.2, 0.25])
    d[axis] = -1.0
    t = m.points[:, axis].copy()
    m.points = np.ascontiguousarray(m.points + np.outer(t, d))
    m.points[:, axis] = 0.0
    return all_flags_one(m)


TINY_LENGTH = 3.5e-7


def tiny_tet(length=TINY_LENGTH, flags_one=True, n=5):
    """Kuhn tetrahedra on a box of 3.5e-7: IDW compares the SQUARED distance node - centroid with (float)1e-15 = 1.00000000362e-15
    (idw.pyx:53,67-69), i.e. a distance of 3.16e-8, and the distances here are 2.5e-8 .. 6e-8 (cells of 7e-8): the branch fires for
    some neighbours and not for others.  The row of a hit is e_j, j the FIRST neighbour within the threshold.

    Counted with the oracle (216 nodes, 64 of them interior):
      default flags (the interior rows only):   17 unit rows, 13 with j >= 8, 6 with j >= 16, none at j = 0; 47 ordinary rows
      all flags 1 (every row, the default here): 24 unit rows, 15 with j >= 8, 6 with j >= 16, 3 at j = 0; 192 ordinary rows
    length = 1.0: no unit row; length = 5e-9: every computed row is e_0 (the two controls of tests/test_rows_paths.py).
    n = 6 (the same cells, one more a side: 343 nodes -- interpolate() is cut into pieces from 256 nodes on, which n = 5 does not
    have): 47 unit rows, 31 with j >= 8, 10 with j >= 16, in every piece of the pipeline."""
    m = M.tet_mesh(n, lengths=(length * n / 5,) * 3, jitter=0.2, seed=2)
    M.attach_fields(m, "u", perm="LIN", seed=2)
    return all_flags_one(m) if flags_one else m


def fan_fields(mesh, variable="u"):
    """fields for a fan: the Neumann flag on two nodes of three (ids not divisible by 3), so that most rows of every tile are computed
    -- the rim nodes are boundary nodes: without a flag their rows are skipped -- and every tile, the long one included, still holds
    skipped rows (written as zeros) between computed ones"""
    M.attach_fields(mesh, variable, perm="LIN", neumann_plane=(2, 0.0), seed=3)
    mesh.point_data["neumann_flag_" + variable] = (np.arange(mesh.points.shape[0]) % 3 != 0).astype(float)
    return mesh


def delaunay_small():
    """559 nodes, mean row 20.6 -> cap 1536 and tiles of 32 nodes; 18 tiles, none longer than the cap"""
    return M.delaunay_tet_mesh(6, seed=4, lattice="random")


def rows_tiling(esup_ptr):
    """(cap, tn, run length of every tile): launch_rows (kernels_idw_ls.hip) and apply_cap (kernels_csr.hip) restated.  cap = the
    entries of LDS a wavefront owns: 64 x the longest row, or 1536 when that exceeds 1024; then tn, the nodes of a tile, halves from 64
    down to 16 while tn x the mean row x 1.25 exceeds 1536.  A tile whose run exceeds cap is not staged."""
    ptr = np.asarray(esup_ptr, dtype=np.int64)
    P = len(ptr) - 1
    mx = int(np.diff(ptr).max())
    cap, tn = 64 * mx, 64
    if cap > CAP_SHORT:
        cap = CAP_LONG
        mean = float(ptr[-1]) / P
        while tn > 16 and tn * mean * 1.25 > cap:
            tn >>= 1
    starts = np.arange(0, P, tn)
    ends = np.minimum(starts + tn, P)
    return cap, tn, ptr[ends] - ptr[starts]


def tiles_of(nodes, tn):
    return np.unique(np.asarray(nodes) // tn)


def nodes_of_tiles(tiles, tn, P):
    return np.concatenate([np.arange(t * tn, min((t + 1) * tn, P)) for t in tiles if 0 <= t * tn < P])


def apply_model(indptr, indices, w, u):
    """(ref, bound) of one field: ref[p] = sum_j w_j u[c_j] over row p in np.longdouble, and the bound a sequential float64 sum of the
    row's n_p products may be off by: (n_p + 1) * 2**-53 * sum_j |w_j u_j| -- the forward error of a recursive sum of n_p products
    (n_p roundings at most on any term: its product's and the additions after it), one term larger to cover the reference's own
    rounding to float64 and its 80-bit sums.  An FMA in place of a product and its addition only removes a rounding."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = np.diff(indptr)
    rows = np.repeat(np.arange(len(n)), n)
    t = np.asarray(w, dtype=np.longdouble) * np.asarray(u, dtype=np.longdouble)[np.asarray(indices)]
    ref = np.zeros(len(n), dtype=np.longdouble)
    mag = np.zeros(len(n), dtype=np.longdouble)
    np.add.at(ref, rows, t)
    np.add.at(mag, rows, np.abs(t))
    return ref, (n + 1) * np.longdouble(2.0) ** -53 * mag


def esup_data(grid, w, nws=None):
    """a dense (n_points, MX_ELEMENTS_PER_POINT) table as the array in CSR position (esup layout), `+ nws[row]` where given"""
    ptr = np.asarray(grid.esup_ptr, dtype=np.int64)
    n = np.diff(ptr)
    rows = np.repeat(np.arange(len(n)), n)
    local = np.arange(int(ptr[-1])) - np.repeat(ptr[:-1], n)
    d = np.asarray(w)[rows, local]
    return d if nws is None else d + np.asarray(nws)[rows]


def inverse_distance_rows(grid):
    """the normalised 1 / dist rows, three coordinates: what LS's D == 0.0 fallback (ls.pyx:88-102) writes, as a dense table"""
    ptr, esup = np.asarray(grid.esup_ptr, dtype=np.int64), np.asarray(grid.esup, dtype=np.int64)
    X, C = np.asarray(grid.point_coords), np.asarray(grid.centroids)
    n = np.diff(ptr)
    rows = np.repeat(np.arange(len(n)), n)
    local = np.arange(int(ptr[-1])) - np.repeat(ptr[:-1], n)
    inv = 1.0 / np.sqrt(((C[esup] - X[rows]) ** 2).sum(axis=1))
    tot = np.zeros(len(n))
    np.add.at(tot, rows, inv)
    out = np.zeros((len(n), int(grid.MX_ELEMENTS_PER_POINT)))
    out[rows, local] = inv / tot[rows]
    return out


def fallback_rows(grid, w, tol=1e-12):
    """which rows of the dense table w equal the 1 / dist formula to `tol` (absolute: a row sums to 1)"""
    f = inverse_distance_rows(grid)
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(np.asarray(w) - f) <= tol, axis=1)


def unit_rows(grid, w):
    """(nodes, j) of the rows of the dense table w that are e_j: one entry exactly 1.0, every other exactly 0, among the first n_p"""
    n = np.diff(np.asarray(grid.esup_ptr, dtype=np.int64))
    w = np.asarray(w)
    inside = np.arange(w.shape[1])[None, :] < n[:, None]
    ones = (w == 1.0) & inside
    zeros = (w == 0.0) & inside
    unit = (ones.sum(axis=1) == 1) & (zeros.sum(axis=1) == n - 1) & (n > 1)
    nodes = np.flatnonzero(unit)
    return nodes, np.argmax(ones[nodes], axis=1)
