"""mesh.composite_mesh -- the disjoint union of several meshes, the input on which every GLS kernel runs in one launch
(tests/test_gpu_composite.py) -- checked on the host: its invariants, and that the oracle on the union is the oracle of each
part, row for row through the part maps.  That makes the union a valid test input before any GPU sees it."""
import numpy as np
import pytest

import util
from ninpol_amd import mesh as M


def _parts():
    return [M.hex_mesh(4, jitter=0.1, seed=1), M.delaunay_tet_mesh(4, seed=2, lattice="random"),
            M.mixed_mesh(5, 3, 3, n_hex=2, jitter=0.1, seed=4), M.wedge_fan(12, 2), M.delaunay_wedge_mesh(5, 3, seed=5),
            M.tet_mesh(3, jitter=0.1, seed=6)]


def _with_fields(parts):
    for i, p in enumerate(parts):
        M.attach_fields(p, "u", perm="ALH", neumann_plane=(2, 0.0), seed=10 + i)
    return parts


@pytest.mark.parametrize("interleave", [True, False])
def test_composite_mesh_invariants(interleave):
    parts = _with_fields(_parts())
    m = M.composite_mesh(parts, interleave=interleave)
    P, E = m.points.shape[0], m.n_cells
    assert P == sum(p.points.shape[0] for p in parts) and E == sum(p.n_cells for p in parts)
    types = [b.type for b in m.cells]
    assert len(types) == len(set(types)) == len({b.type for p in parts for b in p.cells})
    # the maps are bijections onto the node / cell ranges
    assert np.array_equal(np.sort(np.concatenate(m.part_nodes)), np.arange(P))
    assert np.array_equal(np.sort(np.concatenate(m.part_cells)), np.arange(E))
    # no cell references nodes of two parts, and every cell is its part's cell with the nodes mapped
    owner = np.empty(P, dtype=np.int64)
    for i, nodes in enumerate(m.part_nodes):
        owner[nodes] = i
    conn = [np.asarray(row) for b in m.cells for row in b.data]
    for b in m.cells:
        o = owner[b.data]
        assert np.all(o == o[:, :1]), b.type
    for i, p in enumerate(parts):
        np.testing.assert_array_equal(m.points[m.part_nodes[i]], p.points)
        local = [(b.type, row) for b in p.cells for row in b.data]
        kinds = {b.type: b.data.shape[1] for b in m.cells}
        for c, (t, row) in zip(m.part_cells[i], local):
            assert kinds[t] == len(row) and np.array_equal(conn[c], m.part_nodes[i][row])
        assert np.all(np.diff(m.part_cells[i]) > 0)   # ... in the part's own order
        if interleave:   # each part's own order is kept, and every quarter of the node range holds ~ a quarter of it
            assert np.all(np.diff(m.part_nodes[i]) > 0)
            n = len(m.part_nodes[i])
            q = np.bincount(4 * m.part_nodes[i] // P, minlength=4)
            assert q.min() >= 1 and np.abs(q - n / 4).max() <= 1 + len(parts), (i, q)
    # fields travel with their nodes and cells, and attach_fields on the union gives each part what it gives the part alone
    for name in ("permeability", "u"):
        whole = np.concatenate(m.cell_data[name])
        for i, p in enumerate(parts):
            np.testing.assert_array_equal(whole[m.part_cells[i]], np.concatenate(p.cell_data[name]))
    for name in ("neumann_flag_u", "neumann_u"):
        for i, p in enumerate(parts):
            np.testing.assert_array_equal(m.point_data[name][m.part_nodes[i]], p.point_data[name])
    fresh = M.composite_mesh(_parts(), interleave=interleave)
    M.attach_fields(fresh, "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    np.testing.assert_array_equal(np.concatenate(fresh.cell_data["permeability"]), np.concatenate(m.cell_data["permeability"]))
    np.testing.assert_array_equal(fresh.point_data["neumann_flag_u"], m.point_data["neumann_flag_u"])
    assert m.point_data["neumann_flag_u"].sum() > 0


def test_composite_oracle_equals_each_part(oracle_lib):
    """The oracle on the union against the oracle on every part alone, rows and columns mapped: weights and neumann_ws bit
    for bit, every method (each part's cells keep their relative order in the union, so every node's system is the same; the
    order matters to GLS -- on the mixed part's transition nodes a reordering of the cells moves weights by ~1e-8).  The grid
    of the union holds the parts as separate components: the cells around nodes[p] are exactly cells[...] of the part's cells
    around p."""
    parts = _with_fields(_parts())
    m = M.composite_mesh(parts)
    o = oracle_lib.OracleInterpolator("port", threads=4)
    o.load_mesh(m)
    g = o.grid
    got = {meth: o.prepare(meth, "u") for meth in ("idw", "ls", "gls")}
    ep = np.asarray(g.esup_ptr)
    pairs_whole = np.repeat(np.arange(g.n_points), np.diff(ep)) * g.n_elems + np.asarray(g.esup)
    pairs_parts = []
    for i, p in enumerate(parts):
        op = oracle_lib.OracleInterpolator("port", threads=4)
        op.load_mesh(p)
        pp = np.asarray(op.grid.esup_ptr)
        pairs_parts.append(m.part_nodes[i][np.repeat(np.arange(op.grid.n_points), np.diff(pp))] * g.n_elems
                           + m.part_cells[i][np.asarray(op.grid.esup)])
        for meth in ("idw", "ls", "gls"):
            wp, nwp = op.prepare(meth, "u")
            w, nw = got[meth]
            mine = util.part_table(util.esup_csr(g, w), op.grid, m.part_nodes[i], m.part_cells[i])
            assert np.any(np.nan_to_num(wp) != 0), (i, meth)
            np.testing.assert_array_equal(mine, wp, err_msg=f"part {i} {meth}")
            np.testing.assert_array_equal(nw[m.part_nodes[i]], nwp, err_msg=f"part {i} {meth}")
    np.testing.assert_array_equal(np.sort(pairs_whole), np.sort(np.concatenate(pairs_parts)))
