"""The yardstick of tests/test_gpu_gls_exact.py validated on its own (CPU): tests/gls_exact.py solves a node's float64 GLS system
in 80-bit arithmetic, and the GPU tests hold every kernel to "no further from that solution than util.FAN_EXACT_SLACK x the
oracle's own distance".  Before a kernel is held to it:
  * the code moved out of tests/golden/make_fan_exact.py is still the code that made the committed pin (bit for bit);
  * an independent solver (numpy's SVD-based lstsq) agrees with it;
  * the oracle's distance from exact is what the bar assumes on every case the GPU tests run -- at most WEIGHT_RTOL / 2, nothing
    degenerate in the samples;
  * the yardstick resolves a relative error of 1e-12 in tau;
  * the numpy models of the multifrontal kernels -- a correct elimination in the kernels' operation order -- fit under the bar."""
import os
import sys

import numpy as np
import pytest

import gls_exact as X
import util
from ninpol_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the figures of record (this file prints them; `pytest -s tests/test_gls_exact.py`): the oracle's worst distance over all cases
# is 3.2e-11 (delaunay_wedge12x6_random, FAN); at most 2 of a case's 40 nodes are excluded (edge / corner nodes of the Neumann plane)
MAX_EXCLUDED = 0.05


def _oracle(oracle_lib, mesh):
    o = oracle_lib.OracleInterpolator("port", threads=4)
    o.load_mesh(mesh)
    return o


def test_moved_solver_reproduces_the_pinned_rows_bit_for_bit(oracle_lib):
    """system() / last_row_of_pinv() in tests/gls_exact.py are the code that made tests/golden/pins/fan_exact.npz: 16 of the
    pinned rows of exact_32 (every 28th node of the sample: interior and Neumann-plane nodes), recomputed, are identical."""
    z = util.load_fan_exact()
    nodes, pinned = z["nodes_32"], z["exact_32"]
    pick = np.arange(0, len(nodes), len(nodes) // 16)[:16]
    mesh = M.hex_mesh(32, jitter=0.15, seed=0)
    M.attach_fields(mesh, "u", perm="FAN", neumann_plane=(2, 0.0), seed=7)
    o = _oracle(oracle_lib, mesh)
    exact, ok = X.exact_rows(o, mesh, "u", nodes[pick])
    assert ok.all() and exact.shape == (16, 8)
    flag = mesh.point_data["neumann_flag_u"].astype(bool)
    assert flag[nodes[pick]].any() and not flag[nodes[pick]].all()
    np.testing.assert_array_equal(exact, pinned[pick])


def test_extended_qr_agrees_with_an_independent_solver():
    """Random full-rank 40 x 25 systems with the identity block the GLS right-hand side has: row n-1 of the least-squares solution
    from the extended-precision Householder QR against numpy's lstsq (LAPACK gelsd: an SVD, nothing shared) to 1e-12."""
    rng = np.random.default_rng(0)
    for _ in range(8):
        A = rng.standard_normal((40, 25))
        ne = 8
        B = np.zeros((40, ne))
        B[:ne] = np.eye(ne)
        ref = np.linalg.lstsq(A, B, rcond=None)[0][-1]
        got = X.last_row_of_pinv(A, ne)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    with pytest.raises(ZeroDivisionError):
        A[:, 3] = 0.0
        X.last_row_of_pinv(A, ne)


def _yardstick(oracle_lib, mesh, label):
    """(oracle's distance from exact for the weights and for neumann_ws, nodes sampled, nodes excluded) on the seeded sample of
    about 40 computed nodes of a case"""
    o = _oracle(oracle_lib, mesh)
    wo, no = o.prepare("gls", "u")
    G = o.grid
    flag = mesh.point_data["neumann_flag_u"].astype(bool)
    nodes = X.sample_nodes(X.computed_nodes(G, flag), G, label, total=40)
    exact, ok = X.exact_rows(o, mesh, "u", nodes)
    keep = ok & np.abs(wo[nodes]).any(axis=1)
    assert flag[nodes[keep]].any() and not flag[nodes[keep]].all(), "interior and Neumann nodes both"
    nws = X.exact_neumann_ws(exact, ok, G, flag, nodes)
    d = X.dist(wo[nodes][keep], exact[keep])
    dn = X.dist_scaled(np.abs(no[nodes] - nws)[keep], exact[keep])
    print(f"{label}: {len(nodes)} nodes, {int((~keep).sum())} excluded; oracle vs exact {d:.2e}, neumann_ws {dn:.2e}")
    return d, dn, len(nodes), int((~keep).sum())


@pytest.mark.parametrize("perm", X.TENSORS)
@pytest.mark.parametrize("case", list(X.unit_cases()))
def test_oracle_distance_on_the_unit_box(oracle_lib, case, perm):
    """The yardstick table, unit box: the oracle is at most WEIGHT_RTOL / 2 from exact on every case the GPU tests run, and at
    most 5 % of the sampled nodes are excluded (exact solve degenerate, or an all-zero oracle row)."""
    d, dn, n, excluded = _yardstick(oracle_lib, X.unit_mesh(case, perm), f"{case}/{perm}")
    assert n >= 32 and excluded <= MAX_EXCLUDED * n
    assert d <= util.WEIGHT_RTOL / 2 and dn <= util.WEIGHT_RTOL / 2


@pytest.mark.parametrize("transform", list(X.TRANSFORMS))
@pytest.mark.parametrize("case", X.TRANSFORM_MESHES)
def test_oracle_distance_off_the_unit_box(oracle_lib, case, transform):
    """The yardstick table, transformed meshes and eta > 1: the same two assertions.  A kernel that is wrong there is a bug, not
    conditioning."""
    d, dn, n, excluded = _yardstick(oracle_lib, X.transformed_mesh(case, transform), f"{case}/{transform}")
    assert n >= 32 and excluded <= MAX_EXCLUDED * n
    assert d <= util.WEIGHT_RTOL / 2 and dn <= util.WEIGHT_RTOL / 2


@pytest.mark.parametrize("case", ["hex8", "tet5"])
def test_yardstick_resolves_1e_minus_12_in_tau(oracle_lib, case):
    """tau scaled by (1 + 1e-12) in every system: the exact weights must move by more than 4 x the oracle's distance (ALH) -- or
    the bar cannot see the errors it is there for (a lost digit in fast_rcp / fast_rsqrt / face_tau)."""
    mesh = X.unit_mesh(case, "ALH")
    o = _oracle(oracle_lib, mesh)
    wo, _ = o.prepare("gls", "u")
    G = o.grid
    flag = mesh.point_data["neumann_flag_u"].astype(bool)
    nodes = X.sample_nodes(X.computed_nodes(G, flag), G, f"{case}/ALH", total=40)
    exact, ok = X.exact_rows(o, mesh, "u", nodes)
    moved, ok2 = X.exact_rows(o, mesh, "u", nodes, tau_scale=1.0 + 1e-12)
    assert ok.all() and ok2.all()
    d_oracle = X.dist(wo[nodes], exact)
    d_moved = X.dist(moved, exact)
    print(f"{case}/ALH: tau x (1 + 1e-12) moves the exact weights by {d_moved:.2e}; oracle vs exact {d_oracle:.2e}")
    assert d_moved > 4 * d_oracle


def _model_pools(oracle_lib, node_weights, meshes, perm):
    """[(label, model's distances per node, oracle's distances per node)] over the interior nodes the model takes"""
    out = []
    for label, mesh in meshes:
        M.attach_fields(mesh, "u", perm=perm)
        o = _oracle(oracle_lib, mesh)
        wo, _ = o.prepare("gls", "u")
        G = o.grid
        fperm, dmag, flag = X.fields(o, mesh, "u")
        nodes = np.array([p for p in range(G.n_points) if not G.boundary_points[p]])
        exact, ok = X.exact_rows(o, mesh, "u", nodes)
        assert ok.all()
        dm, do = [], []
        for i, p in enumerate(nodes):
            w = node_weights(int(p), G, fperm, dmag)
            if w is None:
                continue
            sc = np.abs(exact[i]).max()
            dm.append(np.abs(w - exact[i, :len(w)]).max() / sc)
            do.append(np.abs(wo[p] - exact[i]).max() / sc)
        out.append((label, np.array(dm), np.array(do)))
    return out


@pytest.mark.parametrize("perm", X.TENSORS)
@pytest.mark.parametrize("model", ["proto_hex8_mf", "proto_mfw"])
def test_kernel_models_fit_under_the_bar(oracle_lib, model, perm):
    """tools/proto_hex8_mf.py and tools/proto_mfw.py -- the kernels' elimination order in numpy -- on the meshes of
    test_multifrontal_model.py: the model's worst distance from exact is at most FAN_EXACT_SLACK x the oracle's.  Pools as in the
    GPU tests: a mesh with fewer than 16 nodes is pooled with the model's other small meshes (a single node's ratio reaches 3.6)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    P = __import__(model)
    if model == "proto_hex8_mf":
        meshes = [("hex434", M.hex_mesh(4, 3, 4, jitter=0.15, seed=2))]
    else:
        meshes = [("tet3", M.tet_mesh(3, jitter=0.1, seed=1)), ("wedge3", M.wedge_mesh(3, jitter=0.05, seed=1)),
                  ("hex3", M.hex_mesh(3, jitter=0.1, seed=1)), ("mixed644", M.mixed_mesh(6, 4, 4, jitter=0.1, seed=1))]
    pools = _model_pools(oracle_lib, P.node_weights, meshes, perm)
    small = [p for p in pools if len(p[1]) < 16]
    pools = [p for p in pools if len(p[1]) >= 16]
    if small:
        pools.append(("+".join(p[0] for p in small), np.concatenate([p[1] for p in small]), np.concatenate([p[2] for p in small])))
    for label, dm, do in pools:
        assert len(dm) > 0
        print(f"{model} {label}/{perm}: {len(dm)} nodes, model vs exact {dm.max():.2e}, oracle vs exact {do.max():.2e}, "
              f"ratio {dm.max() / do.max():.2f}")
        assert dm.max() <= util.FAN_EXACT_SLACK * do.max(), label
