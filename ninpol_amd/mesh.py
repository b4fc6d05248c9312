"""Mesh containers and synthetic mesh generators.

`Interpolator.load_mesh(mesh_obj=...)` is duck-typed exactly as in the reference
(`interpolator.pyx:258,291-294,333-361,217-227,433-447,454`): anything with `.points`,
`.cells` (blocks with `.type` / `.data`), `.cell_data`, `.cell_data_dict`, `.point_data` works --
a real `meshio.Mesh` included.  `Mesh` / `CellBlock` below are the minimal containers of that
shape used by our own generators (meshio is not a dependency of this package).

The reference ships no mesh files (`tests/mesh/.gitkeep`), so the generators here are ours:
structured hexahedra, the Kuhn 6-tetrahedra split, wedges, and a conforming hex | pyramid+tet |
tet mix.  Node numbering is x-fastest, z-slowest so a contiguous node block is a z-slab.
"""
import numpy as np


class CellBlock:
    def __init__(self, type, data):
        self.type = type
        self.data = np.ascontiguousarray(data)

    def __len__(self):
        return len(self.data)

    def __repr__(self):
        return f"<CellBlock {self.type} x{len(self.data)}>"


class Mesh:
    """points (P, 3); cells: list of CellBlock; point_data {name: (P,) array};
    cell_data {name: [array per block]} -- the meshio.Mesh layout."""

    def __init__(self, points, cells, point_data=None, cell_data=None):
        self.points = np.asarray(points)
        self.cells = [c if hasattr(c, "type") else CellBlock(*c) for c in cells]
        self.point_data = dict(point_data or {})
        self.cell_data = dict(cell_data or {})

    @property
    def cell_data_dict(self):
        return {k: {cb.type: a for cb, a in zip(self.cells, v)} for k, v in self.cell_data.items()}

    @property
    def n_cells(self):
        return sum(len(c) for c in self.cells)


# ------------------------------------------------------------------------------------------------
# structured generators
# ------------------------------------------------------------------------------------------------

def _lattice_points(nx, ny, nz, lengths, origin, jitter, seed, k0=0, k1=None):
    """Lattice nodes of planes k0..k1 (inclusive) of the global (nx, ny, nz) box, x fastest.

    Jitter is drawn per z-plane from default_rng([seed, k]) so that any z-slab of the mesh can be
    generated on its own (one slab per GPU rank) and agrees with the whole mesh on shared planes."""
    k1 = nz if k1 is None else k1
    x = np.linspace(0.0, lengths[0], nx + 1) + origin[0]
    y = np.linspace(0.0, lengths[1], ny + 1) + origin[1]
    z = np.linspace(0.0, lengths[2], nz + 1)[k0:k1 + 1] + origin[2]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    if jitter:
        h = np.array([lengths[0] / nx, lengths[1] / ny, lengths[2] / nz])
        npl = (nx + 1) * (ny + 1)
        I = np.arange(npl)
        i, j = I % (nx + 1), I // (nx + 1)
        for k in range(k0, k1 + 1):
            d = np.random.default_rng([seed, k]).uniform(-jitter, jitter, size=(npl, 3)) * h
            # keep the box: boundary nodes only move inside their boundary plane
            d[(i == 0) | (i == nx), 0] = 0.0
            d[(j == 0) | (j == ny), 1] = 0.0
            if k == 0 or k == nz:
                d[:, 2] = 0.0
            pts[(k - k0) * npl:(k - k0 + 1) * npl] += d
    return np.ascontiguousarray(pts)


def _hex_corner_ids(nx, ny, nz, i0=0, i1=None):
    """(E, 8) node ids of the lattice cells i0 <= i < i1 in meshio hexahedron order:
    0=(i,j,k) 1=(i+1,j,k) 2=(i+1,j+1,k) 3=(i,j+1,k), 4..7 the same at k+1.  Cell order x-fastest."""
    if i1 is None:
        i1 = nx
    sx, sy = nx + 1, (nx + 1) * (ny + 1)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(i0, i1), indexing="ij")
    n0 = (i + j * sx + k * sy).ravel().astype(np.int64)
    off = np.array([0, 1, 1 + sx, sx, sy, sy + 1, sy + 1 + sx, sy + sx], dtype=np.int64)
    return n0[:, None] + off[None, :]


def hex_mesh(nx, ny=None, nz=None, lengths=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
             jitter=0.0, seed=0):
    """nx*ny*nz hexahedra on a box."""
    ny = nx if ny is None else ny
    nz = nx if nz is None else nz
    pts = _lattice_points(nx, ny, nz, lengths, origin, jitter, seed)
    return Mesh(pts, [CellBlock("hexahedron", _hex_corner_ids(nx, ny, nz))])


def hex_slab(nx, ny, nz, plane_lo, plane_hi, lengths=(1.0, 1.0, 1.0), jitter=0.0, seed=0):
    """The part of hex_mesh(nx, ny, nz) a rank owning node planes [plane_lo, plane_hi) needs: those
    planes plus one halo plane on each interior side, and every cell between them.  Returns
    (mesh, node_offset, cell_offset, owned_lo, owned_hi): local ids + offset = global ids, and the
    owned nodes are the local range [owned_lo, owned_hi).  Nodes partition by contiguous index
    blocks with the neighbouring cells replicated (north_star)."""
    k0 = max(plane_lo - 1, 0)
    k1 = min(plane_hi, nz)            # last node plane kept (inclusive)
    pts = _lattice_points(nx, ny, nz, lengths, (0.0, 0.0, 0.0), jitter, seed, k0, k1)
    cells = _hex_corner_ids(nx, ny, k1 - k0)
    npl = (nx + 1) * (ny + 1)
    mesh = Mesh(pts, [CellBlock("hexahedron", cells)])
    return mesh, k0 * npl, k0 * nx * ny, (plane_lo - k0) * npl, (plane_hi - k0) * npl


# the six Kuhn simplices of the unit cube as paths 0 -> 6 through hexahedron-local corners,
# each re-ordered to positive orientation
_KUHN = np.array([
    [0, 1, 2, 6], [0, 2, 3, 6], [0, 3, 7, 6], [0, 7, 4, 6], [0, 4, 5, 6], [0, 5, 1, 6],
], dtype=np.int64)


def _kuhn_from_hex(hexes):
    return hexes[:, _KUHN].reshape(-1, 4)


def tet_mesh(nx, ny=None, nz=None, lengths=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
             jitter=0.0, seed=0):
    """Kuhn split: 6 tetrahedra per lattice cell around the 0-6 diagonal (conforming)."""
    ny = nx if ny is None else ny
    nz = nx if nz is None else nz
    pts = _lattice_points(nx, ny, nz, lengths, origin, jitter, seed)
    return Mesh(pts, [CellBlock("tetra", _kuhn_from_hex(_hex_corner_ids(nx, ny, nz)))])


def wedge_mesh(nx, ny=None, nz=None, lengths=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
               jitter=0.0, seed=0):
    """2 wedges per lattice cell, split along the 0-2 diagonal of the bottom quad."""
    ny = nx if ny is None else ny
    nz = nx if nz is None else nz
    pts = _lattice_points(nx, ny, nz, lengths, origin, jitter, seed)
    h = _hex_corner_ids(nx, ny, nz)
    w = np.stack([h[:, [0, 1, 2, 4, 5, 6]], h[:, [0, 2, 3, 4, 6, 7]]], axis=1).reshape(-1, 6)
    return Mesh(pts, [CellBlock("wedge", w)])


def wedge_fan(n_sectors, n_layers=2, jitter=0.0, seed=0):
    """A disc of `n_sectors` triangles around its centre, extruded into `n_layers` layers of wedges: the interior
    nodes on the axis have 2 * n_sectors cells and 5 * n_sectors faces around them -- the high-degree nodes that no
    lattice generator produces (wide GLS systems: column slots 3-4, the global-scratch class)."""
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * np.arange(n_sectors) / n_sectors
    pts = []
    for k in range(n_layers + 1):
        z = k / n_layers
        pts.append([0.0, 0.0, z])
        pts.extend([[np.cos(t), np.sin(t), z] for t in th])
    pts = np.asarray(pts, dtype=float)
    if jitter:
        pts[:, :2] += rng.uniform(-jitter, jitter, size=(len(pts), 2)) * (np.abs(pts[:, :1]) + np.abs(pts[:, 1:2]) > 0)
    per = n_sectors + 1
    w = []
    for k in range(n_layers):
        lo, hi = k * per, (k + 1) * per
        for i in range(n_sectors):
            a, b = 1 + i, 1 + (i + 1) % n_sectors
            w.append([lo, lo + a, lo + b, hi, hi + a, hi + b])   # bottom triangle counter-clockwise from above
    return Mesh(pts, [CellBlock("wedge", np.asarray(w, dtype=np.int64))])


def mixed_mesh(nx, ny=None, nz=None, n_hex=None, lengths=(1.0, 1.0, 1.0), jitter=0.0, seed=0):
    """Conforming hex | transition | tet mesh along x.

    Lattice columns i < n_hex stay hexahedra; column i == n_hex is the transition layer: each cell
    gets a centre node and six pyramids (quad faces meet the hexahedra and each other), and the
    pyramid on the +x face is cut into two tetrahedra along the diagonal the Kuhn split uses there;
    columns i > n_hex are Kuhn tetrahedra.  Blocks are [hexahedron, pyramid, tetra] (meshio order of
    appearance), so the global cell numbering is the concatenation in that order.
    """
    ny = nx if ny is None else ny
    nz = nx if nz is None else nz
    n_hex = nx // 2 if n_hex is None else n_hex
    assert 0 < n_hex < nx - 1
    pts = _lattice_points(nx, ny, nz, lengths, (0.0, 0.0, 0.0), jitter, seed)
    hexes = _hex_corner_ids(nx, ny, nz, 0, n_hex)
    trans = _hex_corner_ids(nx, ny, nz, n_hex, n_hex + 1)
    tets_src = _hex_corner_ids(nx, ny, nz, n_hex + 1, nx)
    centres = pts[trans].mean(axis=1)
    c_id = pts.shape[0] + np.arange(trans.shape[0], dtype=np.int64)
    pts = np.vstack([pts, centres])
    # pyramid base = the hexahedron face reversed (so its own base face [0,3,2,1] points outward)
    hex_faces = np.array([[0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [1, 2, 6, 5],
                          [2, 3, 7, 6], [3, 0, 4, 7]])
    pyr, tet_extra = [], []
    for f in hex_faces:
        base = trans[:, f[::-1]]
        if set(f.tolist()) == {1, 2, 6, 5}:          # the +x face: two tetrahedra, diagonal 1-6
            # base (reversed face) = [5, 6, 2, 1]; Kuhn cuts the quad {1,2,6,5} along 1-6
            q = trans
            tet_extra.append(np.stack([q[:, 1], q[:, 6], q[:, 2], c_id], axis=1))
            tet_extra.append(np.stack([q[:, 1], q[:, 5], q[:, 6], c_id], axis=1))
        else:
            pyr.append(np.concatenate([base, c_id[:, None]], axis=1))
    pyr = np.stack(pyr, axis=1).reshape(-1, 5)
    tet_extra = np.stack(tet_extra, axis=1).reshape(-1, 4)
    tets = np.vstack([tet_extra, _kuhn_from_hex(tets_src)])
    tets = _fix_tet_orientation(pts, tets)
    return Mesh(pts, [CellBlock("hexahedron", hexes), CellBlock("pyramid", pyr),
                      CellBlock("tetra", tets)])


def delaunay_tet_mesh(n, jitter=0.25, seed=0, lattice="bcc", renumber=True):
    """UNSTRUCTURED tetrahedra: the Delaunay tetrahedrisation (scipy.spatial.Delaunay = Qhull) of a jittered point cloud
    in the unit box -- the mesh class the reference's tetra / prism / misc numbers are taken on (gmsh-type meshes,
    tests/results/yaml/performance.yaml:184-246: ~23 cells per node); the reference ships no mesh files, so this generator
    stands in for them.  Node degree is irregular: 2 V - 4 cells around an interior node with V neighbours -- 14 .. 40, mean 25
    for the default cloud (Kuhn meshes: always 24; no two-colouring of the cells either).

    lattice = "bcc": the corners and the centres of an n^3 lattice (2 n^3 + ... points, ~12.5 n^3 cells), each moved by
              U(-jitter, jitter) * h -- slivers stay rare (smallest cell volume ~1e-3 h^3 at jitter 0.25);
              "random": the lattice corners on the boundary + (n - 1)^3 + n^3 uniform random interior points (a wider degree
              distribution: up to ~50 cells per node, and worse cells).
    Boundary points stay in their boundary plane (corners fixed), so the hull is the box.  renumber: nodes in (z, y, x) order of
    their lattice cell and cells in the order of their lowest node, so that contiguous node blocks are z-slabs as in the
    structured generators (Qhull's own order is kept otherwise)."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    h = 1.0 / n
    g = np.arange(n + 1) * h
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    corners = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    c = (np.arange(n) + 0.5) * h
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    centres = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    if lattice == "bcc":
        pts = np.vstack([corners, centres])
        d = rng.uniform(-jitter, jitter, size=pts.shape) * h
    elif lattice == "random":
        on_b = np.any((corners < 1e-12) | (corners > 1 - 1e-12), axis=1)
        n_int = (n - 1) ** 3 + n ** 3
        pts = np.vstack([corners[on_b], rng.uniform(0.2 * h, 1.0 - 0.2 * h, size=(n_int, 3))])
        d = np.zeros_like(pts)
        d[:int(on_b.sum())] = rng.uniform(-jitter, jitter, size=(int(on_b.sum()), 3)) * h
    else:
        raise ValueError("lattice must be 'bcc' or 'random'")
    for a in range(3):                                   # boundary points only move inside their boundary plane
        on = (np.abs(pts[:, a]) < 1e-12) | (np.abs(pts[:, a] - 1.0) < 1e-12)
        d[on, a] = 0.0
    pts = pts + d
    tets = Delaunay(pts).simplices.astype(np.int64)
    if renumber:
        ijk = np.clip(np.floor(pts / h - 1e-9).astype(np.int64), 0, n - 1)
        order = np.lexsort((pts[:, 0], ijk[:, 0], ijk[:, 1], ijk[:, 2]))
        new_id = np.empty(len(pts), dtype=np.int64)
        new_id[order] = np.arange(len(pts))
        pts = pts[order]
        tets = new_id[tets]
        tets = tets[np.lexsort((tets.max(axis=1), tets.min(axis=1)))]
    tets = _fix_tet_orientation(pts, tets)
    return Mesh(np.ascontiguousarray(pts), [CellBlock("tetra", tets)])


def delaunay_wedge_mesh(n, layers=None, jitter=0.3, seed=0, lattice="grid"):
    """UNSTRUCTURED prisms: the Delaunay triangulation (scipy / Qhull) of a jittered point cloud in the unit square, extruded into
    `layers` layers of wedges (default n) -- the "prism" mesh class of the reference's numbers (performance.yaml; it ships no mesh
    files).  A node inside has 2 V wedges around it, V = its valence in the triangulation: 4 .. 9 (the structured wedge_mesh: always
    6), and the ring of wedges is two-coloured only where V is even.

    lattice = "grid": the (n + 1)^2 lattice points, each moved by U(-jitter, jitter) * h; "random": the lattice points on the
    boundary + (n - 1)^2 uniform random points inside.  Boundary points stay on their boundary line.  Nodes are numbered layer by
    layer ((z, y, x) order of their lattice cell), cells layer by layer, bottom triangle counter-clockwise seen from above."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    layers = n if layers is None else layers
    h = 1.0 / n
    g = np.arange(n + 1) * h
    Y, X = np.meshgrid(g, g, indexing="ij")
    p2 = np.stack([X.ravel(), Y.ravel()], axis=1)
    on_b = np.any((p2 < 1e-12) | (p2 > 1 - 1e-12), axis=1)
    if lattice == "grid":
        d = rng.uniform(-jitter, jitter, size=p2.shape) * h
    elif lattice == "random":
        p2 = np.vstack([p2[on_b], rng.uniform(0.2 * h, 1.0 - 0.2 * h, size=((n - 1) ** 2, 2))])
        on_b = np.arange(len(p2)) < int(on_b.sum())
        d = np.zeros_like(p2)
        d[on_b] = rng.uniform(-jitter, jitter, size=(int(on_b.sum()), 2)) * h
    else:
        raise ValueError("lattice must be 'grid' or 'random'")
    for a in range(2):
        on = (np.abs(p2[:, a]) < 1e-12) | (np.abs(p2[:, a] - 1.0) < 1e-12)
        d[on, a] = 0.0
    p2 = p2 + d
    ij = np.clip(np.floor(p2 / h - 1e-9).astype(np.int64), 0, n - 1)
    order = np.lexsort((p2[:, 0], ij[:, 0], ij[:, 1]))
    p2 = p2[order]
    tri = Delaunay(p2).simplices.astype(np.int64)
    a, b, c = p2[tri[:, 0]], p2[tri[:, 1]], p2[tri[:, 2]]
    cw = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]) < 0
    tri[cw] = tri[cw][:, [0, 2, 1]]
    tri = tri[np.lexsort((tri.max(axis=1), tri.min(axis=1)))]
    per = len(p2)
    z = np.arange(layers + 1) / layers
    pts = np.concatenate([np.column_stack([p2, np.full(per, zk)]) for zk in z])
    w = np.concatenate([np.hstack([tri + k * per, tri + (k + 1) * per]) for k in range(layers)])
    return Mesh(np.ascontiguousarray(pts), [CellBlock("wedge", w.astype(np.int64))])


def quad_tri_mesh_2d(nx, ny=None, jitter=0.0, seed=0):
    """2-D mesh on the unit square: left half quads, right half triangles (each lattice cell cut along its
    0-2 diagonal).  Points are (P, 3) with z = 0, as meshio delivers 2-D meshes."""
    ny = nx if ny is None else ny
    pts = _lattice_points(nx, ny, 1, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), jitter, seed, 0, 0)
    pts[:, 2] = 0.0
    sx = nx + 1
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    n0 = (i + j * sx).ravel().astype(np.int64)
    q = np.stack([n0, n0 + 1, n0 + 1 + sx, n0 + sx], axis=1)
    left = (i.ravel() < nx // 2)
    quads = q[left]
    qt = q[~left]
    tris = np.stack([qt[:, [0, 1, 2]], qt[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return Mesh(pts, [CellBlock("quad", quads), CellBlock("triangle", tris)])


def composite_mesh(parts, interleave=True):
    """The disjoint union of several meshes: one mesh whose connected components are the `parts`, so that every kernel a
    part needs runs in the same launch.  Points are concatenated as they are (the parts may overlap in space: the grid is
    built from connectivity alone); blocks of one cell type are merged into one block (cell_data_dict is keyed by type),
    each holding the parts' cells in part order.  The blocks are ordered so that every part's cells keep their relative order
    where the parts' own block orders allow it: a node's cells are then listed in the same order as in its part, and the
    methods form the same sums (GLS on a mixed mesh is sensitive to the column order of its systems at ~1e-8).

    interleave: global node ids follow each node's fractional position inside its own part (a stable merge on
    (local id + 0.5) / n_part): every part keeps its own node order, and every quarter of the node range holds about a quarter of
    every part -- interpolate() cuts each kernel's list by node range, and the parts' kernels then share every piece.  Without
    it the parts' nodes follow one another.

    The returned mesh carries `part_nodes` / `part_cells`: per part, the global id of each local node / cell.  Point and cell
    data arrays that every part has are carried over, mapped the same way."""
    n_pts = [int(p.points.shape[0]) for p in parts]
    total = sum(n_pts)
    if interleave:
        key = np.concatenate([(np.arange(n) + 0.5) / n for n in n_pts])
        order = np.argsort(key, kind="stable")          # ties: the lower part first
        gid = np.empty(total, dtype=np.int64)
        gid[order] = np.arange(total)
    else:
        gid = np.arange(total, dtype=np.int64)
    part_nodes = np.split(gid, np.cumsum(n_pts)[:-1])
    points = np.empty((total, 3))
    points[gid] = np.concatenate([np.asarray(p.points, dtype=float) for p in parts])
    # block order: every part's own block order wherever the parts agree on it (then each part's cells keep their relative
    # order, and so does every node's list of cells); ties and conflicts go to the type that appears first
    seen = []
    for p in parts:
        seen += [b.type for b in p.cells if b.type not in seen]
    before = {t: set() for t in seen}
    for p in parts:
        order_p = [b.type for b in p.cells]
        for k, t in enumerate(order_p):
            before[t].update(u for u in order_p[:k] if u != t)
    types = []
    while len(types) < len(seen):
        free = [t for t in seen if t not in types and before[t] <= set(types)]
        types.append(free[0] if free else next(t for t in seen if t not in types))
    part_cells = [np.empty(p.n_cells, dtype=np.int64) for p in parts]
    blocks, pieces = [], []           # pieces: (part, first local cell, count) in global cell order
    at = 0
    for t in types:
        data = []
        for i, p in enumerate(parts):
            first = 0
            for b in p.cells:
                if b.type == t:
                    data.append(part_nodes[i][np.asarray(b.data)])
                    part_cells[i][first:first + len(b)] = at + np.arange(len(b))
                    pieces.append((i, first, len(b)))
                    at += len(b)
                first += len(b)
        blocks.append(CellBlock(t, np.vstack(data)))
    sizes = np.cumsum([0] + [len(b) for b in blocks])
    cell_data = {}
    for name in set.intersection(*(set(p.cell_data) for p in parts)):
        flat = [np.concatenate(p.cell_data[name]) for p in parts]
        merged = np.concatenate([flat[i][f:f + n] for i, f, n in pieces])
        cell_data[name] = [merged[sizes[b]:sizes[b + 1]] for b in range(len(blocks))]
    point_data = {}
    for name in set.intersection(*(set(p.point_data) for p in parts)):
        a = np.concatenate([np.asarray(p.point_data[name]) for p in parts])
        point_data[name] = np.empty_like(a)
        point_data[name][gid] = a
    m = Mesh(points, blocks, point_data=point_data, cell_data=cell_data)
    m.part_nodes, m.part_cells = part_nodes, part_cells
    return m


# ------------------------------------------------------------------------------------------------
# relabelling: the same mesh as an arbitrary mesher would number it
# ------------------------------------------------------------------------------------------------

def _cyclic(face):
    """a face as the set of its cyclic rotations' canonical form: rotated so that its smallest vertex comes first"""
    if len(face) == 2:          # an edge of a 2-D cell: the ordered pair is its orientation
        return tuple(face)
    k = face.index(min(face))
    return tuple(face[k:] + face[:k])


def _oriented_automorphisms(n, faces):
    """Every permutation s of range(n) that maps each oriented face (v0, v1, ...) of `faces` onto an oriented face of `faces`
    (same cyclic order, not reversed): the orientation-preserving symmetries of the cell's surface."""
    from itertools import permutations
    have = {_cyclic(list(f)) for f in faces}
    return [s for s in permutations(range(n)) if all(_cyclic([s[v] for v in f]) in have for f in faces)]


def _hexahedron_rotations():
    """The 24 proper rotations of the cube (signed permutation matrices of determinant +1) acting on the corner coordinates
    of the meshio hexahedron: s[v] = the corner that corner v is carried to."""
    from itertools import permutations, product
    corners = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]) * 2 - 1
    index = {tuple(c): v for v, c in enumerate(corners)}
    out = []
    for axes in permutations(range(3)):
        for signs in product((1, -1), repeat=3):
            R = np.zeros((3, 3), dtype=np.int64)
            for r in range(3):
                R[r, axes[r]] = signs[r]
            if round(np.linalg.det(R)) == 1:
                out.append(tuple(index[tuple(R @ c)] for c in corners))
    return out


_ROTATIONS = {}


def cell_rotations(cell_type):
    """(G, n) int64: the orientation-preserving symmetry group of a cell type in meshio vertex order, one permutation a row
    (24 hexahedron, 12 tetra, 6 wedge, 4 pyramid, 4 quad, 3 triangle); data[:, row] is the same cell with its vertices listed
    from another corner.  Derived, not typed in: the hexahedron's from the rotations of the cube, the others from the type's
    face table (2-D types: their edges) in topology.py.  None for a type without faces (vertex, line)."""
    if cell_type not in _ROTATIONS:
        from .topology import ELEMENTS
        e = ELEMENTS[cell_type]
        faces = e["faces"] or (e["edges"] if cell_type in ("triangle", "quad") else [])
        if cell_type == "hexahedron":
            rows = _hexahedron_rotations()
        elif faces:
            rows = _oriented_automorphisms(e["number_of_points"], faces)
        else:
            rows = None
        _ROTATIONS[cell_type] = None if rows is None else np.array(sorted(rows), dtype=np.int64)
    return _ROTATIONS[cell_type]


def relabel_mesh(mesh, seed, nodes=True, cells=True, rotate=True):
    """The same mesh (geometry, topology, fields) under another labelling, as a mesher's file would bring it:

    nodes:  a random permutation of the node ids (points, every point_data array, all connectivity);
    cells:  a random permutation of the cells inside each block (connectivity and every cell_data array); blocks keep their
            type and order;
    rotate: per cell, a random element of cell_rotations(type): its vertices listed from another corner, orientation kept
            (no reflections: the reference assumes positively oriented cells).

    Attach fields BEFORE relabelling: they are carried over, so a Neumann plane and its seeded values mean the same nodes.
    The returned mesh carries `new_node_of_old` (new id of each old node) and `old_cell_of_new` (old global cell id, block
    order, of each new global cell), as composite_mesh carries part_nodes / part_cells."""
    rng = np.random.default_rng(seed)
    P = int(np.asarray(mesh.points).shape[0])
    new_node_of_old = rng.permutation(P).astype(np.int64) if nodes else np.arange(P, dtype=np.int64)
    points = np.empty_like(np.asarray(mesh.points))
    points[new_node_of_old] = mesh.points
    point_data = {}
    for name, a in mesh.point_data.items():
        a = np.asarray(a)
        point_data[name] = np.empty_like(a)
        point_data[name][new_node_of_old] = a
    blocks, orders = [], []
    for b in mesh.cells:
        data = np.asarray(b.data)
        n = len(data)
        order = rng.permutation(n) if cells else np.arange(n)
        data = data[order]
        table = cell_rotations(b.type) if rotate else None
        if table is not None and n:
            data = np.take_along_axis(data, table[rng.integers(len(table), size=n)], axis=1)
        blocks.append(CellBlock(b.type, new_node_of_old[data]))
        orders.append(order)
    cell_data = {name: [np.asarray(a)[o] for a, o in zip(per_block, orders)] for name, per_block in mesh.cell_data.items()}
    first = np.cumsum([0] + [len(o) for o in orders])
    m = Mesh(np.ascontiguousarray(points), blocks, point_data=point_data, cell_data=cell_data)
    m.new_node_of_old = new_node_of_old
    m.old_cell_of_new = np.concatenate([first[b] + o for b, o in enumerate(orders)]).astype(np.int64) if orders else np.zeros(0, dtype=np.int64)
    return m


def _fix_tet_orientation(pts, tets):
    a, b, c, d = (pts[tets[:, i]] for i in range(4))
    vol = np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a)
    neg = vol < 0
    tets = tets.copy()
    tets[neg, 1], tets[neg, 2] = tets[neg, 2].copy(), tets[neg, 1].copy()
    return tets


# ------------------------------------------------------------------------------------------------
# synthetic fields (the shapes the reference's analytical cases use, tests/utils/analytical.py)
# ------------------------------------------------------------------------------------------------

def cell_centroids(mesh):
    """vertex mean per cell, block order (what analytical.py:142 evaluates K at)."""
    return np.vstack([mesh.points[c.data].mean(axis=1) for c in mesh.cells])


def permeability_alh(centroids):
    """Heterogeneous SPD tensor of the ALH case (tests/utils/analytical.py:303-323)."""
    x, y, z = centroids[:, 0], centroids[:, 1], centroids[:, 2]
    K = np.zeros((len(x), 3, 3))
    K[:, 0, 0] = y ** 2 + z ** 2 + 1
    K[:, 0, 1] = -x * y
    K[:, 0, 2] = -x * z
    K[:, 1, 0] = -y * x
    K[:, 1, 1] = x ** 2 + z ** 2 + 1
    K[:, 1, 2] = -y * z
    K[:, 2, 0] = -z * x
    K[:, 2, 1] = -z * y
    K[:, 2, 2] = x ** 2 + y ** 2 + 1
    return K


def permeability_const(n, kind="LIN"):
    """Constant tensors of the LIN/QUAD and FAN cases (analytical.py:253-296)."""
    if kind == "FAN":
        Ku = np.array([[2464.36, 0.0, 1148.68], [0.0, 536.64, 0.0], [1148.68, 0.0, 536.64]])
    else:
        Ku = np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.5], [0.0, 0.5, 1.0]])
    K = np.zeros((n, 3, 3))
    K[:] = Ku
    return K


def attach_fields(mesh, variable="u", perm="ALH", neumann_plane=None, seed=1, values=None):
    """Attach `permeability`, a scalar cell variable and the Neumann point arrays to `mesh`.

    neumann_plane: None (all-Dirichlet boundary, flags 0) or (axis, coordinate): nodes with
    |x[axis] - coordinate| < 1e-12 get flag 1 and a U(0,1) Neumann value (default_rng(seed)).
    """
    cen = cell_centroids(mesh)
    E = cen.shape[0]
    K = permeability_alh(cen) if perm == "ALH" else permeability_const(E, perm)
    K = K.reshape(E, 9)
    if values is None:
        values = cen[:, 0] + cen[:, 1] + cen[:, 2]
    P = mesh.points.shape[0]
    flag = np.zeros(P)
    val = np.zeros(P)
    if neumann_plane is not None:
        axis, coord = neumann_plane
        on = np.abs(mesh.points[:, axis] - coord) < 1e-12
        flag[on] = 1.0
        val[on] = np.random.default_rng(seed).uniform(0.0, 1.0, int(on.sum()))
    sizes = np.cumsum([0] + [len(c) for c in mesh.cells])
    split = lambda a: [a[sizes[b]:sizes[b + 1]] for b in range(len(mesh.cells))]
    mesh.cell_data = {"permeability": split(K), variable: split(np.asarray(values, dtype=float))}
    mesh.point_data = {"neumann_flag_" + variable: flag, "neumann_" + variable: val}
    return mesh
