"""Neumann flags from the device: Interpolator.update_neumann_flags rewrites the resident flag bytes from device tensors -- the whole
array or a subset of nodes -- and marks exactly the nodes whose bit changed; DevicePlan.launch_dirty recomputes those rows in place
(csrc/flags_update.hip).  The yardstick throughout is a FRESH Interpolator loaded with a mesh that carries the new flags; comparisons
are bit for bit (np.array_equal); GLS is also held to the oracle on that mesh within the suite's bars."""
import copy

import numpy as np
import pytest

import util
import test_gpu_update_fields as UF
import test_gpu_update_local as UL
import test_gpu_update_points as UP
import test_update_points_local_host as LH
import test_update_flags_host as FH
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

METHODS, PLANE = UF.METHODS, UF.PLANE
same, on_device, with_K, _loaded = UF.same, UF.on_device, UF.with_K, UF._loaded
ids_on_device, stream, _buffers, _host, _torch, verts_of = UL.ids_on_device, UL.stream, UL._buffers, UL._host, UL._torch, UL.verts_of
with_flags, VALUES, IS_SET = FH.with_flags, FH.VALUES, FH.IS_SET
FULL, KEPT = UL.FULL, UL.KEPT
C = UL.C          # the composite mesh of test_gpu_update_local.py: every non-empty plan kernel, with the owner kernel of every node


def bits_of(flags):
    """the host packer's rule: (long long)x != 0"""
    return np.asarray(flags, dtype=np.float64).astype(np.int64) != 0


def bytes_on_device(a, dtype, odd_offset=False):
    """a bool / uint8 array as a CUDA tensor; odd_offset: a view one byte into a larger buffer, so that its address is odd"""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    if not odd_offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    start = 1 if buf.data_ptr() % 2 == 0 else 2
    view = buf[start:start + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 8 != 0 and view.is_contiguous()
    return view


def row_of(I, variable="u"):
    return FH.row(I, variable)


def fresh_launch(mesh, meth, add_neumann=True, variable="u"):
    from ninpol_amd.interpolator import DevicePlan
    plan = DevicePlan(_loaded(mesh), variable, meth)
    b = _buffers(plan, FULL)
    plan.launch(b[0].data_ptr(), b[1].data_ptr(), stream(), add_neumann=add_neumann)
    return _host(b)


# ---- 1. the kernels' corners ---------------------------------------------------------------------------------------------------------
CORNERS = {"120_nodes": lambda: M.hex_mesh(5, 4, 3), "4913_nodes": lambda: M.hex_mesh(16)}      # neither a multiple of 8, 64 or 256
CASES = ("m0", "m1", "m63", "m64", "m65", "all_shuffled", "duplicates")


@pytest.fixture(scope="module", params=sorted(CORNERS))
def corner(request):
    from ninpol_amd.interpolator import DevicePlan
    mesh = M.attach_fields(CORNERS[request.param](), "u", perm="LIN", neumann_plane=PLANE, seed=2)
    I = _loaded(mesh)
    DevicePlan(I, "u", "idw")                                        # the grid goes to the device, the host row's flags are resident
    g = I.grid
    P = int(g.n_points)
    assert P == int(request.param.split("_")[0]) and g.device >= 0 and g.dirty_nodes == -1 and g.flag_updates == 0
    bits = bits_of(row_of(I))
    assert same(g.fetch_flags(), bits.astype(np.uint8)) and bits.any() and not bits.all()
    return {"I": I, "P": P, "bits": bits, "boundary": np.array(g.boundary_points) != 0}


def _after(corner, n0, changed, what):
    g = corner["I"].grid
    assert same(g.fetch_flags(), corner["bits"].astype(np.uint8)), (what, "bits")
    assert g.flag_updates == n0, (what, "flag_updates")
    assert g.dirty_nodes == changed, (what, "dirty_nodes", g.dirty_nodes, changed)


@pytest.mark.parametrize("case", CASES)
def test_scatter_corners(corner, case):
    I, P, bits = corner["I"], corner["P"], corner["bits"]
    g = I.grid
    host_row = row_of(I)
    rng = np.random.default_rng(len(case) + P)
    if case == "all_shuffled":
        ids = rng.permutation(P)
    elif case == "duplicates":
        ids = np.tile(rng.choice(P, size=20, replace=False), 2)
    else:
        ids = rng.permutation(P)[:int(case[1:])]
    m = len(ids)
    for dt in (np.int32, np.int64):
        for kind in ("float64", "bool"):
            per_node = rng.integers(0, len(VALUES), P)               # a value per NODE: duplicate ids carry equal values
            vals = VALUES[per_node][ids] if kind == "float64" else IS_SET[per_node][ids]
            new = bits.copy()
            new[ids] = bits_of(vals)
            changed = int(np.count_nonzero(new != bits))
            bits[:] = new
            g.clear_dirty()
            n0 = g.flag_updates
            I.update_neumann_flags("u", on_device(vals) if kind == "float64" else bytes_on_device(vals, np.bool_), nodes=ids_on_device(ids, dt))
            what = (case, dt.__name__, kind)
            assert I.neumann_flags_on_device or m == 0, what
            _after(corner, n0 + (1 if m else 0), changed, what)
            # the same values again: nothing changes, nothing is marked
            g.clear_dirty()
            I.update_neumann_flags("u", on_device(vals) if kind == "float64" else bytes_on_device(vals, np.bool_), nodes=ids_on_device(ids, dt))
            _after(corner, n0 + (2 if m else 0), 0, what + ("again",))
    assert same(row_of(I), host_row)                                 # the device path leaves the host row alone
    assert same(g.boundary_points != 0, corner["boundary"])


@pytest.mark.parametrize("odd_offset", (False, True), ids=("aligned", "odd_offset"))
@pytest.mark.parametrize("kind", ("float64", "bool", "uint8"))
def test_whole_array_corners(corner, kind, odd_offset):
    I, P, bits = corner["I"], corner["P"], corner["bits"]
    g = I.grid
    host_row = row_of(I)
    rng = np.random.default_rng(P + len(kind) + odd_offset)
    for rnd in range(2):
        pick = rng.integers(0, len(VALUES), P)
        pick[rng.permutation(P)[:len(VALUES)]] = np.arange(len(VALUES))          # every value at least once
        if kind == "float64":
            vals, dev = VALUES[pick], on_device(VALUES[pick], odd_offset)
        else:
            vals = IS_SET[pick] if kind == "bool" else np.where(IS_SET[pick], pick + 1, 0)     # uint8: any non-zero byte is set
            dev = bytes_on_device(vals, np.bool_ if kind == "bool" else np.uint8, odd_offset)
        new = bits_of(vals)
        changed = int(np.count_nonzero(new != bits))
        assert changed > 0
        bits[:] = new
        g.clear_dirty()
        n0 = g.flag_updates
        I.update_neumann_flags("u", dev)
        assert I.neumann_flags_on_device
        _after(corner, n0 + 1, changed, (kind, odd_offset, rnd))
        g.clear_dirty()
        I.update_neumann_flags("u", dev)                             # equal values: nothing is marked
        _after(corner, n0 + 2, 0, (kind, odd_offset, rnd, "again"))
    assert same(row_of(I), host_row)
    assert same(g.boundary_points != 0, corner["boundary"])
    # while every node is dirty no marks are made, and the bits follow all the same
    g.mark_all_dirty()
    flip = ~bits
    I.update_neumann_flags("u", bytes_on_device(flip, np.bool_))
    bits[:] = flip
    assert g.dirty_nodes == -1 and same(g.fetch_flags(), bits.astype(np.uint8))
    g.clear_dirty()
    assert g.dirty_nodes == 0


# ---- 2, 3. every kernel of the plan, in place; nothing else is written ---------------------------------------------------------------
def flag_change(c):
    """new flags for the composite: per plan kernel that owns boundary nodes a few Dirichlet nodes turned Neumann and a few Neumann nodes
    turned Dirichlet, and a few interior nodes flagged.  Returns (f1, changed nodes, nodes turned Dirichlet)."""
    f0 = np.array(c.mesh.point_data["neumann_flag_u"], dtype=np.float64)
    b0 = bits_of(f0)
    I = _loaded(c.mesh)
    boundary = np.array(I.grid.boundary_points) != 0
    rng = np.random.default_rng(41)
    f1 = f0.copy()
    to_neu, to_dir = [], []
    owners = sorted(set(c.owner[boundary].tolist()))
    for k in owners:
        mine = boundary & (c.owner == k)
        d, n = np.flatnonzero(mine & ~b0), np.flatnonzero(mine & b0)
        to_neu += rng.choice(d, size=min(3, len(d)), replace=False).tolist()
        to_dir += rng.choice(n, size=min(3, len(n)), replace=False).tolist()
        assert len(d) + len(n) > 0
    inner = rng.choice(np.flatnonzero(~boundary), size=5, replace=False).tolist()
    f1[to_neu] = 1.0
    f1[to_dir] = 0.0
    f1[inner] = 1.0
    names = [I.grid.PLAN_KERNELS[k] for k in owners]
    assert any(n.startswith("small") for n in names) and "quad4" in names and "mfx_boundary" in names and any(n.startswith("block") for n in names), names
    # both directions in the small-node, quad and boundary multifrontal kernels, where most boundary nodes live
    for fam in ("small", "quad4", "mfx_boundary"):
        ks = [k for k in owners if I.grid.PLAN_KERNELS[k].startswith(fam)]
        assert any(c.owner[p] in ks for p in to_neu) and any(c.owner[p] in ks for p in to_dir), fam
    changed = np.flatnonzero(bits_of(f1) != b0)
    assert len(changed) == len(to_neu) + len(to_dir) + len(inner)
    return f1, changed, np.array(sorted(to_dir)), boundary


@pytest.fixture(scope="module")
def change(C):
    f1, changed, to_dir, boundary = flag_change(C)
    return {"f1": f1, "changed": changed, "to_dir": to_dir, "boundary": boundary, "mesh1": with_flags(C.mesh, f1), "fresh": {}}


def _fresh1(change, meth, add_neumann):
    key = (meth, add_neumann)
    if key not in change["fresh"]:
        change["fresh"][key] = fresh_launch(change["mesh1"], meth, add_neumann)
    return change["fresh"][key]


@pytest.mark.parametrize("add_neumann", (True, False), ids=("add_neumann", "plain"))
@pytest.mark.parametrize("meth", METHODS)
def test_every_kernel_in_place(C, change, oracle_lib, meth, add_neumann):
    I, plan, marked, clean = UL._start(C, meth, add_neumann)
    changed, f1 = change["changed"], change["f1"]
    order = np.random.default_rng(3).permutation(changed)
    I.update_neumann_flags("u", on_device(f1[order]), nodes=ids_on_device(order))
    assert I.grid.dirty_nodes == len(changed) and I.neumann_flags_on_device
    n = plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream(), add_neumann=add_neumann)
    assert n == len(changed) and I.grid.dirty_nodes == 0
    fw, fn = _fresh1(change, meth, add_neumann)
    w, nws = _host(clean)
    assert same(w, fw) and same(nws, fn)
    w0, n0 = C.fresh(C.K0, meth, add_neumann, "K0")
    on = np.zeros(C.P, dtype=bool)
    on[changed] = True
    moved = np.zeros(C.P, dtype=bool)
    differs = lambda a, b: ~((a == b) | (np.isnan(a) & np.isnan(b)))          # (LS leaves NaN in degenerate rows: same bits, not "moved")
    np.logical_or.at(moved, C.rows, differs(fw, w0))
    moved |= differs(fn, n0)
    assert not (moved & ~on).any() and (moved & on).any()            # the fresh plans themselves differ inside the set only
    if meth == "gls":
        assert moved[changed].all(), "every changed flag moves its GLS row"
    if meth == "gls" and add_neumann:
        UL._oracle_check(oracle_lib, _OracleCtx(C, change["mesh1"]), C.K0, w, nws, "composite, flags changed")


class _OracleCtx:
    """UL._oracle_check's view of a context: the mesh carrying the new flags"""

    def __init__(self, c, mesh):
        self.mesh, self.esup, self.esup_ptr, self.P, self.E = mesh, c.esup, c.esup_ptr, c.P, c.E


@pytest.mark.parametrize("meth", METHODS)
def test_nothing_else_is_written(C, change, meth):
    torch = _torch()
    I, plan, marked, clean = UL._start(C, meth, True)
    changed, to_dir = change["changed"], change["to_dir"]
    I.update_neumann_flags("u", on_device(change["f1"]))            # the whole array: the same change
    assert I.grid.dirty_nodes == len(changed)
    on = np.zeros(C.P, dtype=bool)
    on[changed] = True
    on_rows = on[C.rows]
    marked[0][:] = KEPT
    marked[1][:] = KEPT
    n = plan.launch_dirty(marked[0].data_ptr(), marked[1].data_ptr(), stream(), clear=False)
    assert n == len(changed) and I.grid.dirty_nodes == len(changed)
    fw, fn = _fresh1(change, meth, True)
    w, nws = _host(marked)
    assert (w[~on_rows] == KEPT).all() and (nws[~on] == KEPT).all(), "a row outside the set was written"
    assert (w[on_rows] != KEPT).all() and (nws[on] != KEPT).all(), "a row of the set was not written"
    assert same(w[on_rows], fw[on_rows]) and same(nws[on], fn[on])
    gone = np.zeros(C.P, dtype=bool)
    gone[to_dir] = True
    assert gone.sum() > 0 and (w[gone[C.rows]] == 0.0).all() and (nws[gone] == 0.0).all(), "rows turned Dirichlet are the zero row"
    assert not np.signbit(w[gone[C.rows]]).any() and not np.signbit(nws[gone]).any()
    n = plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream())
    assert n == len(changed) and I.grid.dirty_nodes == 0
    assert same(_host(clean)[0], fw) and same(_host(clean)[1], fn)


# ---- 4. switching the variable ---------------------------------------------------------------------------------------------------------
def two_variable_mesh():
    mesh = M.attach_fields(M.mixed_mesh(5, 4, 3, jitter=0.1, seed=5), "u", perm="LIN", neumann_plane=PLANE, seed=5)
    other = M.attach_fields(copy.deepcopy(mesh), "v", perm="LIN", neumann_plane=(0, 0.0), seed=6)
    mesh.cell_data["v"] = other.cell_data["v"]
    mesh.point_data["neumann_flag_v"] = other.point_data["neumann_flag_v"]
    mesh.point_data["neumann_v"] = other.point_data["neumann_v"]
    return mesh


@pytest.mark.parametrize("meth", METHODS)
def test_variable_switch(meth):
    from ninpol_amd.interpolator import DevicePlan
    mesh = two_variable_mesh()
    I = _loaded(mesh)
    fu, fv = row_of(I, "u"), row_of(I, "v")
    differ = int(np.count_nonzero(bits_of(fu) != bits_of(fv)))
    assert 0 < differ < I.grid.n_points // 2
    plan_u = DevicePlan(I, "u", meth)
    b = _buffers(plan_u, FULL)
    plan_u.launch(b[0].data_ptr(), b[1].data_ptr(), stream())
    I.grid.clear_dirty(stream())                                    # the buffers hold u's weights
    wu = fresh_launch(mesh, meth, variable="u")
    assert same(_host(b)[0], wu[0]) and same(_host(b)[1], wu[1])
    with pytest.raises(ValueError, match="resident"):
        I.update_neumann_flags("v", on_device(fv[:3]), nodes=ids_on_device(np.arange(3)))
    I.update_neumann_flags("v", on_device(fv))
    assert I.grid.dirty_nodes == differ and I.grid._fields_variable == "v" and I.neumann_flags_on_device
    plan_v = DevicePlan(I, "v", meth)                               # its refresh() finds v's flags resident and current
    assert I.grid.dirty_nodes == differ and I.neumann_flags_on_device
    assert plan_v.launch_dirty(b[0].data_ptr(), b[1].data_ptr(), stream()) == differ
    wv = fresh_launch(mesh, meth, variable="v")
    assert same(_host(b)[0], wv[0]) and same(_host(b)[1], wv[1])
    assert not same(wu[0], wv[0]) or meth != "gls"
    with pytest.raises(ValueError, match="resident"):
        I.update_neumann_flags("u", on_device(fu[:3]), nodes=ids_on_device(np.arange(3)))
    # and back, with bytes
    I.update_neumann_flags("u", bytes_on_device(bits_of(fu), np.bool_))
    assert I.grid.dirty_nodes == differ
    assert plan_u.launch_dirty(b[0].data_ptr(), b[1].data_ptr(), stream()) == differ
    assert same(_host(b)[0], wu[0]) and same(_host(b)[1], wu[1])
    # a plan whose variable is not the resident one uploads its own host row at its next launch: then every node is dirty
    plan_v.launch(b[0].data_ptr(), b[1].data_ptr(), stream())
    assert I.grid.dirty_nodes == -1 and not I.neumann_flags_on_device and I.grid._fields_variable == "v"
    assert same(_host(b)[0], wv[0]) and same(_host(b)[1], wv[1])


# ---- 5. refused ids ----------------------------------------------------------------------------------------------------------------------
def test_ids_outside_the_mesh(C, change):
    from ninpol_amd._lib import NinpolError
    I, plan, marked, clean = UL._start(C, "gls", True)
    changed, f1 = change["changed"], change["f1"]
    half = len(changed) // 2
    ids = np.concatenate([changed[:half], [C.P], changed[half:], [-1]])
    vals = np.concatenate([f1[changed[:half]], [1.0], f1[changed[half:]], [1.0]])
    bits = bits_of(f1)
    for dt in (np.int64, np.int32):
        I.update_neumann_flags("u", on_device(vals), nodes=ids_on_device(ids, dt))
        probe = _buffers(plan, KEPT)
        with pytest.raises(NinpolError, match=r"\b2 node ids outside \[0, %d\) were given to nin_fields_scatter_flags_device" % C.P):
            plan.launch_dirty(probe[0].data_ptr(), probe[1].data_ptr(), stream())
        assert same(I.grid.fetch_flags(), bits.astype(np.uint8)), "the valid entries were written, and nothing else"
        assert I.grid.dirty_nodes == len(changed), "the set is kept"
        assert (_host(probe)[0] == KEPT).all() and (_host(probe)[1] == KEPT).all(), "nothing was launched"
        assert plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream(), clear=(dt is np.int32)) == len(changed)
    assert I.grid.dirty_nodes == 0
    fw, fn = _fresh1(change, "gls", True)
    assert same(_host(clean)[0], fw) and same(_host(clean)[1], fn)


# ---- 6. precedence between the host row and the device copy --------------------------------------------------------------------------------
def test_precedence_between_the_host_row_and_the_device_copy():
    torch = _torch()
    from ninpol_amd.interpolator import DevicePlan
    mesh = M.attach_fields(M.mixed_mesh(5, 4, 3, jitter=0.1, seed=5), "u", perm="LIN", neumann_plane=PLANE, seed=5)
    I = _loaded(mesh)
    P = int(I.grid.n_points)
    f0 = row_of(I)
    rng = np.random.default_rng(9)
    f1 = f0.copy()
    flip = rng.choice(P, size=P // 6, replace=False)
    f1[flip] = 1.0 - f1[flip]
    F1 = _loaded(with_flags(mesh, f1))
    u = rng.uniform(-1.0, 1.0, (2, int(I.grid.n_elems)))
    plan = DevicePlan(I, "u", "gls")
    I.update_neumann_flags("u", on_device(f1))
    assert I.neumann_flags_on_device and same(row_of(I), f0)
    assert plan.any_neumann_flag() == bool(bits_of(f0).any())        # the host row's answer, until fetch_neumann_flags()
    torch.cuda.current_stream().synchronize()
    plan.refresh()
    assert I.neumann_flags_on_device and same(I.grid.fetch_flags(), bits_of(f1).astype(np.uint8))
    for meth in METHODS:
        UF.assert_csr_same(I.interpolate("u", meth), F1.interpolate("u", meth), ("interpolate", meth))
        got, ref = I.apply("u", meth, values=u), F1.apply("u", meth, values=u)
        assert same(got[0], ref[0]) and same(got[1], ref[1]), ("apply", meth)
        assert same(I.apply_transpose("u", meth, got[0]), F1.apply_transpose("u", meth, ref[0])), ("apply_transpose", meth)
    assert I.neumann_flags_on_device and same(I.grid.fetch_flags(), bits_of(f1).astype(np.uint8)) and same(row_of(I), f0)
    # an in-place edit of the host row wins at the next call that reads the tables
    f2 = f0.copy()
    f2[flip[:5]] = 1.0 - f2[flip[:5]]
    I.points_data[I.variable_to_index["points"]["neumann_flag_u"], :P] = f2
    I.grid.clear_dirty()
    plan.refresh()
    assert not I.neumann_flags_on_device and same(I.grid.fetch_flags(), bits_of(f2).astype(np.uint8))
    assert I.grid.dirty_nodes == -1                                  # nobody recorded which rows the upload changed
    UF.assert_csr_same(I.interpolate("u", "gls"), _loaded(with_flags(mesh, f2)).interpolate("u", "gls"), "after the edit")
    # fetch_neumann_flags writes the bits back and the row becomes the resident one
    I.update_neumann_flags("u", bytes_on_device(bits_of(f1), np.uint8))
    assert I.neumann_flags_on_device and same(row_of(I), f2)
    got = I.fetch_neumann_flags("u")
    assert same(got, bits_of(f1).astype(np.float64)) and same(row_of(I), got) and not I.neumann_flags_on_device
    plan.refresh()
    assert same(I.grid.fetch_flags(), bits_of(f1).astype(np.uint8))
    UF.assert_csr_same(I.interpolate("u", "gls"), F1.interpolate("u", "gls"), "after the fetch")
    with pytest.raises(ValueError, match="not found in points data"):
        I.update_neumann_flags("w", on_device(f1))


def test_numpy_flags_follow_on_the_device(C, change):
    """the host path on a grid whose resident flags are the host row's: row, resident bytes and dirty set move together"""
    I, plan, marked, clean = UL._start(C, "gls", True)
    changed, f1 = change["changed"], change["f1"]
    n0 = I.grid.flag_updates
    I.update_neumann_flags("u", f1[changed], nodes=changed)
    assert same(row_of(I), f1) and not I.neumann_flags_on_device and I.grid.flag_updates == n0 + 1
    assert I.grid.dirty_nodes == len(changed) and same(I.grid.fetch_flags(), bits_of(f1).astype(np.uint8))
    plan.refresh()                                                   # uploads the same bytes: the set survives
    assert I.grid.dirty_nodes == len(changed)
    assert plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream()) == len(changed)
    fw, fn = _fresh1(change, "gls", True)
    assert same(_host(clean)[0], fw) and same(_host(clean)[1], fn)
    f0 = np.array(C.mesh.point_data["neumann_flag_u"], dtype=np.float64)
    I.update_neumann_flags("u", f0)                                  # the whole array, back
    assert same(row_of(I), f0) and I.grid.dirty_nodes == len(changed) and I.grid.flag_updates == n0 + 2
    assert plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), stream()) == len(changed)
    w0, nw0 = C.fresh(C.K0, "gls", True, "K0")
    assert same(_host(clean)[0], w0) and same(_host(clean)[1], nw0)


# ---- 7. one step, three sources ------------------------------------------------------------------------------------------------------------
def test_one_step_three_sources(C, change):
    from ninpol_amd.interpolator import DevicePlan
    torch = _torch()
    I, plan, marked, clean = UL._start(C, "gls", True)
    rng = np.random.default_rng(55)
    cells = rng.choice(C.E, size=max(C.E // 100, 2), replace=False)
    nodes = rng.choice(C.P, size=max(C.P // 200, 2), replace=False)
    K1 = UF.K_of(C.mesh, "ALH", 61)
    K_now = C.K0.copy()
    K_now[cells] = K1[cells]
    X0 = np.ascontiguousarray(np.asarray(C.mesh.points, dtype=np.float64))
    X1 = X0.copy()
    X1[nodes] += 0.003 * np.sin(37.0 * X0[nodes] + 1.0)
    changed, f1 = change["changed"], change["f1"]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        I.update_permeability(on_device(K1[cells]), cells=ids_on_device(cells))
        I.update_points(on_device(X1[nodes]), nodes=ids_on_device(nodes))
        I.update_neumann_flags("u", on_device(f1[changed]), nodes=ids_on_device(changed))
        n = plan.launch_dirty(clean[0].data_ptr(), clean[1].data_ptr(), st.cuda_stream)
    st.synchronize()
    union = np.union1d(np.union1d(verts_of(C.inpoel, cells), LH.verts_around(C.inpoel, C.esup, C.esup_ptr, nodes)), changed)
    assert n == len(union) and I.grid.dirty_nodes == 0
    assert len(union) > max(len(changed), len(verts_of(C.inpoel, cells)))
    fw, fn = fresh_launch(UP.with_points(with_K(with_flags(C.mesh, f1), K_now), X1), "gls")
    assert same(_host(clean)[0], fw) and same(_host(clean)[1], fn)


# ---- 8. CellToNode.recompute_weights(dirty_only=True) ----------------------------------------------------------------------------------------
def test_cell_to_node_dirty_only(monkeypatch):
    torch = _torch()
    from ninpol_amd.torch_ops import CellToNode
    monkeypatch.setenv("NIN_APPLY_NO_FUSION", "1")
    small = M.attach_fields(M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    I = _loaded(small)
    E, P = int(I.grid.n_elems), int(I.grid.n_points)
    f0 = row_of(I)
    boundary = np.array(I.grid.boundary_points) != 0
    flip = np.random.default_rng(4).choice(np.flatnonzero(boundary), size=8, replace=False)
    f1 = f0.copy()
    f1[flip] = 1.0 - f1[flip]
    assert bits_of(f0)[flip].any() and not bits_of(f0)[flip].all()     # both directions
    op = CellToNode(I, "u", "gls")
    I.grid.clear_dirty()                                   # op.weights is a full result as of now
    u = torch.from_numpy(np.random.default_rng(17).uniform(0.5, 1.5, E)).cuda().requires_grad_(True)
    g_out = torch.from_numpy(np.random.default_rng(18).uniform(-1.0, 1.0, P)).cuda()
    y_old = op(u)
    old_weights = op.weights
    I.update_neumann_flags("u", on_device(f1[flip]), nodes=ids_on_device(flip))
    assert same(op(u).detach().cpu().numpy(), y_old.detach().cpu().numpy())      # nothing recomputes behind the caller's back
    op.recompute_weights(dirty_only=True)
    assert I.grid.dirty_nodes == 0 and op.weights is not old_weights
    fresh_op = CellToNode(_loaded(with_flags(small, f1)), "u", "gls")
    assert same(op.weights.cpu().numpy(), fresh_op.weights.cpu().numpy())
    assert same(op.neumann_ws.cpu().numpy(), fresh_op.neumann_ws.cpu().numpy())
    assert not same(op.weights.cpu().numpy(), old_weights.cpu().numpy())
    u2 = u.detach().clone().requires_grad_(True)
    uf = u.detach().clone().requires_grad_(True)
    y_new, y_fresh = op(u2), fresh_op(uf)
    assert same(y_new.detach().cpu().numpy(), y_fresh.detach().cpu().numpy())
    y_new.backward(g_out)
    y_fresh.backward(g_out)
    assert same(u2.grad.cpu().numpy(), uf.grad.cpu().numpy())
    # an output computed before the update keeps its old weights in backward
    y_old.backward(g_out)
    old_op = CellToNode(_loaded(small), "u", "gls")
    uo = u.detach().clone().requires_grad_(True)
    old_op(uo).backward(g_out)
    assert same(u.grad.cpu().numpy(), uo.grad.cpu().numpy())
    assert not same(u.grad.cpu().numpy(), u2.grad.cpu().numpy())


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------
def test_input_errors():
    torch = _torch()
    import ninpol_amd
    small = M.attach_fields(M.mixed_mesh(4, 3, 3, jitter=0.1, seed=2), "u", perm="LIN", neumann_plane=PLANE, seed=3)
    I = _loaded(small)
    P = int(I.grid.n_points)
    f = on_device(np.ones(P))
    five = on_device(np.ones(5))
    ids = ids_on_device(np.arange(5))
    host_row = row_of(I)
    for bad in (f.float(), f.half(), f.long(), f.to(torch.int8)):
        with pytest.raises(TypeError, match="float64, bool or uint8"):
            I.update_neumann_flags("u", bad)
    with pytest.raises(TypeError, match="float64, bool or uint8"):
        I.update_neumann_flags("u", five.float(), nodes=ids)
    with pytest.raises(TypeError, match="int32 or int64"):
        I.update_neumann_flags("u", five, nodes=ids.to(torch.int16))
    with pytest.raises(TypeError, match="int32 or int64"):
        I.update_neumann_flags("u", five, nodes=ids.double())
    for bad in (f[:-1], f.reshape(P, 1), torch.cat([f, f])):
        with pytest.raises(ValueError, match="shape"):
            I.update_neumann_flags("u", bad)
    with pytest.raises(ValueError, match="shape"):
        I.update_neumann_flags("u", five, nodes=ids.reshape(5, 1))
    with pytest.raises(ValueError, match="shape"):
        I.update_neumann_flags("u", five[:4], nodes=ids)
    with pytest.raises(ValueError, match="shape"):
        I.update_neumann_flags("u", f, nodes=ids)
    # mixed host / device arguments
    with pytest.raises(TypeError, match="flags must be"):
        I.update_neumann_flags("u", np.ones(5), nodes=ids)
    with pytest.raises(TypeError, match="flags must be"):
        I.update_neumann_flags("u", five.cpu(), nodes=ids)
    with pytest.raises(TypeError, match="nodes must be"):
        I.update_neumann_flags("u", five, nodes=np.arange(5))
    with pytest.raises(TypeError, match="nodes must be"):
        I.update_neumann_flags("u", five, nodes=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="not found in points data"):
        I.update_neumann_flags("w", f)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="must be on cuda:0"):
            I.update_neumann_flags("u", f.to(torch.device("cuda", 1)))
    else:       # one GPU visible: an Interpolator made for another device sees these tensors on the wrong one
        J = ninpol_amd.Interpolator(device=1)
        J.load_mesh(mesh_obj=small)
        with pytest.raises(ValueError, match="must be on cuda:1"):
            J.update_neumann_flags("u", f)
        with pytest.raises(ValueError, match="must be on cuda:1"):
            J.update_neumann_flags("u", five, nodes=ids)
        assert J.grid.device == -1
    assert I.grid.device == -1 and not I.neumann_flags_on_device               # every refusal came before any side effect
    assert same(row_of(I), host_row)
    # the C entry point: a subset cannot be patched before any flags are resident
    from ninpol_amd import _lib
    I.grid.to_device(0)
    rc = _lib.load().nin_fields_scatter_flags_device(I.grid._h, ids.data_ptr(), 1, 5, five.data_ptr(), 0, None)
    assert rc == _lib.NIN_ESTATE and "resident" in _lib.load().nin_last_error().decode()
    assert I.grid.fetch_flags() is None and I.grid.flag_updates == 0
    # ... and the Python layer sends the host row first
    I.update_neumann_flags("u", five, nodes=ids)
    expect = bits_of(host_row)
    expect[:5] = True
    assert same(I.grid.fetch_flags(), expect.astype(np.uint8)) and I.neumann_flags_on_device and I.grid._fields_variable == "u"
