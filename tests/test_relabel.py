"""Labelling invariance on the host (no GPU): mesh.relabel_mesh itself, and everything between load_mesh() and a kernel's
arithmetic that is a function of the node order, the cell order and the local vertex order of a mesh -- the descriptor models
of the multifrontal kernels (tools/proto_hex8_mf.py, tools/proto_mfw.py), the host grid builder, the oracle.

The generators of mesh.py emit ONE labelling (nodes and cells x-fastest, every cell with the same local vertex order); on it
every interior node of a structured mesh gets the same descriptor words.  A mesher's file does not.  The yardstick for a
relabelled mesh is the oracle ON THE SAME relabelled mesh: the reference is not equivariant under cell reordering or vertex
rotation (the float32 normal of a non-planar face depends on which cell and which vertices come first: up to 7e-2 of a row's
largest weight on jittered hexahedra, 2e-8 .. 7e-8 on tetrahedra, O(1) on some Neumann boundary rows).  Under a NODE-ONLY
renumbering it is bit-identical (test_node_only_relabelling_leaves_the_oracle_bit_identical), which the GPU suite relies on."""
import os
import sys
from itertools import permutations

import numpy as np
import pytest

import util
from ninpol_amd import mesh as M
from ninpol_amd.topology import ELEMENTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_ORDER = {"hexahedron": 24, "tetra": 12, "wedge": 6, "pyramid": 4, "quad": 4, "triangle": 3}


def _tools():
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import proto_hex8_mf
    import proto_mfw
    return proto_hex8_mf, proto_mfw


@pytest.fixture(scope="module")
def lib():
    from ninpol_amd import build as nbuild
    nbuild.build()
    from ninpol_amd import _lib
    return _lib


def families():
    """name -> a mesh of every family of the generators, small enough for the host"""
    return {
        "hex": lambda: M.hex_mesh(5, 4, 3, jitter=0.15, seed=1),
        "tet": lambda: M.tet_mesh(3, jitter=0.1, seed=2),
        "wedge": lambda: M.wedge_mesh(4, 3, 3, jitter=0.05, seed=3),
        "mixed": lambda: M.mixed_mesh(6, 4, 4, jitter=0.1, seed=4),
        "delaunay": lambda: M.delaunay_tet_mesh(4, seed=5),
        "delaunay_random": lambda: M.delaunay_tet_mesh(4, seed=6, lattice="random"),
        "prisms": lambda: M.delaunay_wedge_mesh(5, 3, seed=7, lattice="random"),
        "fan": lambda: M.wedge_fan(12, 2, jitter=0.02, seed=8),
        "quad_tri_2d": lambda: M.quad_tri_mesh_2d(7, 5, jitter=0.1, seed=9),
    }


# ---- the symmetry tables ----------------------------------------------------------------------------------------------------

def _faces_of(cell_type):
    e = ELEMENTS[cell_type]
    return e["faces"] or e["edges"]


def _canon(face):
    if len(face) == 2:          # an edge of a 2-D cell: the ordered pair is its orientation
        return tuple(face)
    k = face.index(min(face))
    return tuple(face[k:] + face[:k])


@pytest.mark.parametrize("cell_type", sorted(GROUP_ORDER))
def test_rotation_tables_are_groups_that_map_faces_onto_faces(cell_type):
    """cell_rotations(type): the stated number of distinct permutations, the identity among them, closed under composition
    and inverse, and each maps every oriented face (2-D: edge) of the type's topology table onto an oriented face -- same
    cyclic order, so no reflection is among them."""
    T = M.cell_rotations(cell_type)
    n = ELEMENTS[cell_type]["number_of_points"]
    assert T.shape == (GROUP_ORDER[cell_type], n)
    rows = {tuple(r) for r in T.tolist()}
    assert len(rows) == len(T) and all(sorted(r) == list(range(n)) for r in rows)
    assert tuple(range(n)) in rows
    for a in rows:
        inv = [0] * n
        for i, v in enumerate(a):
            inv[v] = i
        assert tuple(inv) in rows
        for b in rows:
            assert tuple(a[b[i]] for i in range(n)) in rows
    faces = {_canon(list(f)) for f in _faces_of(cell_type)}
    for s in rows:
        assert {_canon([s[v] for v in f]) for f in _faces_of(cell_type)} == faces, s
    # and it is the WHOLE group: no other permutation keeps the oriented faces (8! for the hexahedron is still quick)
    others = [s for s in permutations(range(n)) if s not in rows
              and all(_canon([s[v] for v in f]) in faces for f in _faces_of(cell_type))]
    assert not others
    assert M.cell_rotations("line") is None and M.cell_rotations("vertex") is None


# ---- relabel_mesh itself ----------------------------------------------------------------------------------------------------

def _signed_volumes(mesh):
    """per cell (block order): the sum over its oriented faces of the divergence-theorem term, each face fanned into triangles
    around its vertex mean (so that a non-planar face gives the same value from whichever vertex it is listed) -- positive for
    a positively oriented cell; 2-D: the polygon's signed area"""
    out = []
    for b in mesh.cells:
        X = mesh.points[b.data]                      # (n, nv, 3)
        if b.type in ("quad", "triangle"):
            a = np.zeros(len(X))
            for i in range(1, X.shape[1] - 1):
                p, q = X[:, i, :2] - X[:, 0, :2], X[:, i + 1, :2] - X[:, 0, :2]
                a += p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]
            out.append(0.5 * a)
            continue
        v = np.zeros(len(X))
        for f in ELEMENTS[b.type]["faces"]:
            c = X[:, f].mean(axis=1)
            for i in range(len(f)):
                v += np.einsum("ij,ij->i", c, np.cross(X[:, f[i]], X[:, f[(i + 1) % len(f)]])) / 6.0
        out.append(v)
    return np.concatenate(out)


@pytest.mark.parametrize("switches", [(True, True, True), (True, False, False), (False, True, False), (False, False, True)])
@pytest.mark.parametrize("family", sorted(families()))
def test_relabel_mesh_invariants(family, switches):
    nodes, cells, rotate = switches
    m = families()[family]()
    M.attach_fields(m, "u", perm="ALH", neumann_plane=(1, 0.0), seed=5)
    r = M.relabel_mesh(m, seed=11, nodes=nodes, cells=cells, rotate=rotate)
    P, E = m.points.shape[0], m.n_cells
    # the maps are permutations, the identity where a switch is off
    assert np.array_equal(np.sort(r.new_node_of_old), np.arange(P)) and np.array_equal(np.sort(r.old_cell_of_new), np.arange(E))
    assert np.array_equal(r.new_node_of_old, np.arange(P)) == (not nodes)
    assert np.array_equal(r.old_cell_of_new, np.arange(E)) == (not cells)
    # blocks keep type, order and size; cells stay inside their block
    assert [(b.type, len(b)) for b in r.cells] == [(b.type, len(b)) for b in m.cells]
    first = np.cumsum([0] + [len(b) for b in m.cells])
    for k in range(len(m.cells)):
        sl = r.old_cell_of_new[first[k]:first[k + 1]]
        assert sl.min() >= first[k] and sl.max() < first[k + 1]
    # points and point data travel with their nodes, cell data with their cells
    np.testing.assert_array_equal(r.points[r.new_node_of_old], m.points)
    for name in m.point_data:
        np.testing.assert_array_equal(r.point_data[name][r.new_node_of_old], m.point_data[name])
    for name in m.cell_data:
        np.testing.assert_array_equal(np.concatenate(r.cell_data[name]), np.concatenate(m.cell_data[name])[r.old_cell_of_new])
    assert r.point_data["neumann_flag_u"].sum() == m.point_data["neumann_flag_u"].sum() > 0
    # every cell keeps its vertex SET (and, without rotation, its vertex order)
    old_rows = [row for b in m.cells for row in b.data]
    new_rows = [row for b in r.cells for row in b.data]
    moved = 0
    for c, row in enumerate(new_rows):
        was = r.new_node_of_old[old_rows[r.old_cell_of_new[c]]]
        assert sorted(row.tolist()) == sorted(was.tolist())
        moved += not np.array_equal(row, was)
    assert (moved > 0.5 * E) if rotate else (moved == 0)
    # orientation and centroids
    v0, v1 = _signed_volumes(m), _signed_volumes(r)
    assert np.all(v0 > 0) and np.all(v1 > 0)
    np.testing.assert_allclose(v1, v0[r.old_cell_of_new], rtol=1e-9)
    c0, c1 = M.cell_centroids(m), M.cell_centroids(r)
    assert np.abs(c1 - c0[r.old_cell_of_new]).max() <= 4 * np.finfo(float).eps * max(1.0, np.abs(c0).max())
    # the input is untouched, and the same seed gives the same mesh
    again = M.relabel_mesh(m, seed=11, nodes=nodes, cells=cells, rotate=rotate)
    for a, b in zip(r.cells, again.cells):
        np.testing.assert_array_equal(a.data, b.data)
    fresh = families()[family]()
    np.testing.assert_array_equal(fresh.points, m.points)
    for a, b in zip(fresh.cells, m.cells):
        np.testing.assert_array_equal(a.data, b.data)


# ---- the descriptor models --------------------------------------------------------------------------------------------------

def _oracle(oracle_lib, mesh, threads=2):
    o = oracle_lib.OracleInterpolator("port", threads=threads)
    o.load_mesh(mesh)
    return o


def _node_inputs(G, p):
    cells = G.esup[G.esup_ptr[p]:G.esup_ptr[p + 1]]
    faces = G.fsup[G.fsup_ptr[p]:G.fsup_ptr[p + 1]]
    fc = {}
    for f in faces:
        a, b = G.esuf_ptr[f], G.esuf_ptr[f + 1]
        fc[f] = (int(G.esuf[a]), int(G.esuf[a + 1]) if b - a == 2 else -1)
    return cells, faces, fc


def _freeze(x):
    return tuple(_freeze(y) for y in x) if isinstance(x, (list, tuple)) else x


def _descriptors(model, G):
    """interior node -> the model's descriptor as a hashable value (None: the model refuses the node)"""
    out = {}
    for p in range(G.n_points):
        if G.boundary_points[p]:
            continue
        d = model.descriptor(*_node_inputs(G, p))
        out[p] = None if d is None else _freeze(d)
    return out


VARIETY = [("hex", "cube", lambda: M.hex_mesh(8, 7, 6), 210), ("tet", "mfw", lambda: M.tet_mesh(5), 64),
           ("wedge", "mfw", lambda: M.wedge_mesh(6, 5, 4), 60), ("mixed", "mfw", lambda: M.mixed_mesh(10, 5, 5), 169)]


@pytest.mark.parametrize("name,model,make,n_interior", VARIETY, ids=[v[0] for v in VARIETY])
def test_relabelling_gives_the_descriptors_variety(oracle_lib, name, model, make, n_interior):
    """A condition on the INPUT of the relabelled tests, so that they cannot quietly stop covering anything: in generator order
    the interior nodes of a structured mesh share one descriptor (the mixed mesh: a handful), relabelled they have at least
    10 x as many; and every node the model accepts in generator order it still accepts (the cube graph and the two-colouring
    are topology, not labelling)."""
    hex8, mfw = _tools()
    P = hex8 if model == "cube" else mfw
    m = make()
    M.attach_fields(m, "u", perm="ALH")
    r = M.relabel_mesh(m, seed=3)
    d0 = _descriptors(P, _oracle(oracle_lib, m).grid)
    d1 = _descriptors(P, _oracle(oracle_lib, r).grid)
    assert len(d0) == len(d1) == n_interior
    took0 = {p for p, d in d0.items() if d is not None}
    took1 = {p for p, d in d1.items() if d is not None}
    assert took0 and {int(r.new_node_of_old[p]) for p in took0} <= took1
    kinds0, kinds1 = len({d0[p] for p in took0}), len({d1[p] for p in took1})
    print(f"{name}: {len(took0)} of {n_interior} interior nodes taken; distinct descriptors {kinds0} in generator order, {kinds1} relabelled")
    assert kinds0 <= 5
    assert kinds1 >= 10 * kinds0


def _cell_fields(o):
    G, v2i = o.grid, o.variable_to_index
    perm = o.cells_data[v2i["cells"]["permeability"]][:G.n_elems * 9].reshape(-1, 9)
    dmag = o.cells_data[v2i["cells"]["diff_mag"]][:G.n_elems]
    return perm, dmag


@pytest.mark.parametrize("seed", [0, 1])
def test_cube_node_model_matches_oracle_on_relabelled_mesh(oracle_lib, seed):
    """tools/proto_hex8_mf.py (the arithmetic of kernels_gls_hex8mf.hip lane by lane) on a relabelled hexahedron mesh, at the
    bar of tests/test_multifrontal_model.py: which cell is E_l, the sort of its three faces by odd slot, and the side bit differ
    from node to node here."""
    hex8, _ = _tools()
    m = M.hex_mesh(4, 3, 4, jitter=0.15, seed=2)
    M.attach_fields(m, "u", perm="ALH")
    r = M.relabel_mesh(m, seed=seed)
    o = _oracle(oracle_lib, r)
    W, _ = o.prepare("gls", "u")
    perm, dmag = _cell_fields(o)
    G = o.grid
    interior = [p for p in range(G.n_points) if not G.boundary_points[p]]
    assert len(interior) == 3 * 2 * 3
    for p in interior:
        w = hex8.node_weights(p, G, perm, dmag)
        ref = W[p, :8]
        assert np.abs(w - ref).max() <= 1e-12 * np.abs(ref).max(), p


MFW_MESHES = {"tet": lambda: M.tet_mesh(3, jitter=0.1, seed=1), "wedge": lambda: M.wedge_mesh(3, jitter=0.05, seed=1),
              "hex": lambda: M.hex_mesh(3, jitter=0.1, seed=1), "mixed": lambda: M.mixed_mesh(6, 4, 4, jitter=0.1, seed=1)}


@pytest.mark.parametrize("kind", sorted(MFW_MESHES))
def test_one_wavefront_model_matches_oracle_on_relabelled_mesh(oracle_lib, kind):
    """tools/proto_mfw.py (the arithmetic of kernels_gls_mfw.hip) on the relabelled meshes of
    test_one_wavefront_model_matches_oracle, same bar, and it takes as many nodes as in generator order."""
    _, mfw = _tools()
    taken = {}
    for relabelled in (False, True):
        m = MFW_MESHES[kind]()
        M.attach_fields(m, "u", perm="ALH")
        if relabelled:
            m = M.relabel_mesh(m, seed=4)
        o = _oracle(oracle_lib, m)
        W, _ = o.prepare("gls", "u")
        perm, dmag = _cell_fields(o)
        G = o.grid
        n = 0
        for p in range(G.n_points):
            if G.boundary_points[p]:
                continue
            w = mfw.node_weights(p, G, perm, dmag)
            if w is None:
                continue
            ref = W[p, :len(w)]
            assert np.abs(w - ref).max() <= 1e-12 * np.abs(ref).max(), (relabelled, p)
            n += 1
        taken[relabelled] = n
    assert taken[True] == taken[False] > 0


# ---- the host grid builder --------------------------------------------------------------------------------------------------

def _assert_grid_is_oracles(I, o):
    for k in util.GRID_SCALARS:
        assert getattr(I.grid, k) == getattr(o.grid, k), k
    for k in util.GRID_ARRAYS:
        np.testing.assert_array_equal(getattr(I.grid, k), getattr(o.grid, k), err_msg=k)


@pytest.mark.parametrize("family", sorted(families()) + ["composite"])
def test_host_grid_matches_oracle_on_relabelled_mesh(lib, oracle_lib, family):
    """The native host grid builder against the oracle's grid on relabelled meshes of every family (and the union of relabelled
    parts, relabelled once more): scalars equal, every array bit-equal; one thread and several."""
    import ninpol_amd
    if family == "composite":
        parts = []
        for i, (name, make) in enumerate(sorted(families().items())):
            if name == "quad_tri_2d":
                continue
            p = make()
            M.attach_fields(p, "u", perm="ALH", neumann_plane=(2, 0.0), seed=i)
            parts.append(M.relabel_mesh(p, seed=20 + i))
        mesh = M.relabel_mesh(M.composite_mesh(parts), seed=40)
    else:
        mesh = families()[family]()
        M.attach_fields(mesh, "u", perm="ALH", neumann_plane=(0, 0.0), seed=2)
        mesh = M.relabel_mesh(mesh, seed=13)
    o = _oracle(oracle_lib, mesh)
    for nt in (1, 5):
        I = ninpol_amd.Interpolator(num_threads=nt)
        I.load_mesh(mesh_obj=mesh)
        _assert_grid_is_oracles(I, o)
        np.testing.assert_array_equal(I.cells_data, o.cells_data)
        np.testing.assert_array_equal(I.points_data, o.points_data)


# ---- the oracle under a node-only renumbering -------------------------------------------------------------------------------

NODE_ONLY = [("hex", lambda: M.hex_mesh(6, 5, 4, jitter=0.15, seed=1)), ("tet", lambda: M.tet_mesh(3, jitter=0.1, seed=2)),
             ("mixed", lambda: M.mixed_mesh(6, 4, 4, jitter=0.1, seed=3)),
             ("delaunay_random", lambda: M.delaunay_tet_mesh(4, seed=6, lattice="random")),
             ("prisms", lambda: M.delaunay_wedge_mesh(5, 3, seed=7, lattice="random"))]


@pytest.mark.parametrize("plane", [None, (2, 0.0)], ids=["dirichlet", "neumann"])
@pytest.mark.parametrize("name,make", NODE_ONLY, ids=[v[0] for v in NODE_ONLY])
def test_node_only_relabelling_leaves_the_oracle_bit_identical(oracle_lib, name, make, plane):
    """Renumbering the nodes alone leaves cell order, local vertex order and therefore face order untouched: every node's
    system is the same rows in the same order.  The oracle's LS and GLS tables and neumann_ws, rows mapped by new_node_of_old,
    are bit-identical, interior and boundary rows, with and without a Neumann plane; IDW to its bar (1e-14).  The GPU suite
    asks the same of the kernels without a tolerance."""
    m = make()
    M.attach_fields(m, "u", perm="ALH", neumann_plane=plane, seed=3)
    r = M.relabel_mesh(m, seed=9, cells=False, rotate=False)
    a, b = _oracle(oracle_lib, m), _oracle(oracle_lib, r)
    new = r.new_node_of_old
    for k in ("esup_ptr", "fsup_ptr"):
        np.testing.assert_array_equal(np.diff(getattr(b.grid, k))[new], np.diff(getattr(a.grid, k)))
    for meth in ("idw", "ls", "gls"):
        wa, na = a.prepare(meth, "u")
        wb, nb = b.prepare(meth, "u")
        if meth == "idw":
            assert util.rowscaled_err(wb[new], wa) <= 1e-14
        else:
            assert np.array_equal(wb[new], wa, equal_nan=True), meth
        assert np.array_equal(nb[new], na, equal_nan=True), meth
        assert np.any(np.nan_to_num(wa) != 0)
    if plane is not None:
        assert np.count_nonzero(a.prepare("gls", "u")[1]) > 0
