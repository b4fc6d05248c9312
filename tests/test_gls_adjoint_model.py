"""The numpy model of the GLS adjoint (tests/gls_adjoint_model.py) pinned on the CPU: its forward is the oracle's stored weights,
and its gradient with respect to the permeability is the central difference of the oracle -- diff_mag recomputed from the perturbed K,
so the chain through eta is in it.  eta = max(0, diff_mag_a, diff_mag_b) over the two cells of a face: the ALH field gives every cell its
own diff_mag (smallest gap across a face: 9e-3, 5e-5, 9e-6 and 1e-6 on the four meshes; the step moves a cell's by at most 1e-6), and
every sampled step is checked not to cross a tie; the constant LIN tensor would sit on one."""
import numpy as np
import pytest

import gls_adjoint_model as GM
import util
from ninpol_amd import mesh as M

H = 1e-5            # the central-difference step
FD_RTOL = 1e-8      # of max |grad|: measured 3.7e-10 at worst at this step (4.2e-10 on another machine); the FD noise reaches 5e-9 at h = 1e-6

MESHES = {
    "hex": (lambda: M.hex_mesh(4, jitter=0.1, seed=1), 150),
    "tet": (lambda: M.tet_mesh(3, jitter=0.1, seed=3), 150),
    "mixed": (lambda: M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2), 150),
    "delaunay": (lambda: M.delaunay_tet_mesh(6, seed=4, lattice="random"), 40),
}


def oracle_case(oracle_lib, make):
    mesh = M.attach_fields(make(), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    o = oracle_lib.OracleInterpolator("port", threads=2)
    o.load_mesh(mesh)
    v2i = o.variable_to_index
    E, P = o.grid.n_elems, o.grid.n_points
    perm_row, dmag_row = v2i["cells"]["permeability"], v2i["cells"]["diff_mag"]
    perm = np.array(o.cells_data[perm_row][:E * 9]).reshape(E, 9)
    dmag = np.array(o.cells_data[dmag_row][:E])
    flag = np.array(o.points_data[v2i["points"]["neumann_flag_u"]][:P]).astype(np.int64)
    return o, perm, dmag, flag, (perm_row, dmag_row)


def stored(o, targets=None):
    """the oracle's stored entries (weights + neumann_ws of the row) in esup position, and neumann_ws"""
    g = o.grid
    w, nws = o.prepare("gls", "u", targets)
    ptr = np.asarray(g.esup_ptr)
    cnt = np.diff(ptr)
    rows = np.repeat(np.arange(g.n_points), cnt)
    local = np.arange(len(g.esup)) - np.repeat(ptr[:-1], cnt)
    return w[rows, local] + nws[rows], nws


@pytest.fixture(scope="module", params=sorted(MESHES))
def case(request, oracle_lib):
    make, n_samples = MESHES[request.param]
    o, perm, dmag, flag, rows = oracle_case(oracle_lib, make)
    rng = np.random.default_rng(17)
    ghat = rng.uniform(-1.0, 1.0, len(o.grid.esup))
    gnws = rng.uniform(-1.0, 1.0, o.grid.n_points)
    model = GM.gls_adjoint_model(o.grid, perm, dmag, flag, ghat, add_neumann=True, grad_neumann_ws=gnws)
    return {"name": request.param, "o": o, "perm": perm, "dmag": dmag, "flag": flag, "rows": rows, "ghat": ghat, "gnws": gnws,
            "model": model, "n_samples": n_samples}


def test_diff_mag_is_the_tables_and_distinct(case):
    assert np.array_equal(GM.diff_mag_of(case["perm"]), case["dmag"])
    # eta = max over the two cells of a face: the step moves a cell's diff_mag by at most H |d diff_mag / d K_dd|
    fc = GM.face_cells(case["o"].grid)
    fc = fc[fc[:, 1] >= 0]
    gap = np.abs(case["dmag"][fc[:, 0]] - case["dmag"][fc[:, 1]]).min()
    reach = H * np.abs(GM.diff_mag_derivative(case["perm"])).max()
    print(f"{case['name']}: smallest diff_mag gap across a face {gap:.2e}, the step's reach {reach:.2e}")
    assert gap > 0 and case["dmag"].min() > 2 * reach      # (the sampled steps are checked one by one where they are taken)


def test_forward_is_the_oracle(case):
    d, nws = stored(case["o"])
    m = case["model"]
    ptr = np.asarray(case["o"].grid.esup_ptr)
    worst = 0.0
    for p in range(len(ptr) - 1):
        a, b = m["weights"][ptr[p]:ptr[p + 1]], d[ptr[p]:ptr[p + 1]]
        if len(b):
            worst = max(worst, util.rowscaled_err(a, b))
    print(f"{case['name']}: model forward against the oracle, row-scaled {worst:.2e}")
    assert worst <= util.WEIGHT_RTOL
    assert util.rowscaled_err(m["neumann_ws"], nws) <= util.WEIGHT_RTOL
    assert np.count_nonzero(nws) > 0 and m["computed"].sum() > 0


def test_gradient_is_the_central_difference_of_the_oracle(case):
    o, perm, flag = case["o"], case["perm"], case["flag"]
    perm_row, dmag_row = case["rows"]
    E = len(perm)
    grad = GM.fold(case["model"]["grad_perm"], case["model"]["grad_diff_mag"], perm)
    assert np.count_nonzero(case["model"]["grad_diff_mag"]) > 0, "the eta chain is not exercised"
    ghat, gnws = case["ghat"], case["gnws"]
    inpoel = np.asarray(o.grid.inpoel)
    fc = GM.face_cells(o.grid)
    fc = fc[fc[:, 1] >= 0]
    other = {}                                       # the cells across a cell's internal faces
    for a, b in fc:
        other.setdefault(int(a), []).append(int(b))
        other.setdefault(int(b), []).append(int(a))

    def loss(K, targets):
        o.cells_data[perm_row][:E * 9] = K.reshape(-1)
        o.cells_data[dmag_row][:E] = GM.diff_mag_of(K)
        d, nws = stored(o, targets)          # rows outside `targets` are zero: they do not depend on the perturbed cell
        return float(ghat @ d + gnws @ nws)

    rng = np.random.default_rng(5)
    picks = rng.choice(E * 9, size=case["n_samples"], replace=False)
    scale = np.abs(grad).max()
    worst = 0.0
    try:
        for idx in picks:
            e, k = divmod(int(idx), 9)
            targets = np.array(sorted(int(v) for v in inpoel[e] if v >= 0), dtype=np.int64)
            Kp, Km = perm.copy(), perm.copy()
            Kp[e, k] += H
            Km[e, k] -= H
            nb = case["dmag"][other.get(e, [])]
            side = np.sign(case["dmag"][e] - nb)
            for Kq in (Kp, Km):                      # no max() tie is crossed by this step
                assert np.array_equal(np.sign(GM.diff_mag_of(Kq[e:e + 1])[0] - nb), side), (e, k)
            fd = (loss(Kp, targets) - loss(Km, targets)) / (2 * H)
            worst = max(worst, abs(fd - grad[e, k]) / scale)
    finally:
        o.cells_data[perm_row][:E * 9] = perm.reshape(-1)
        o.cells_data[dmag_row][:E] = case["dmag"]
    print(f"{case['name']}: worst |FD - model| / max|grad| = {worst:.2e} over {len(picks)} entries (max|grad| = {scale:.3e})")
    assert worst <= FD_RTOL
