"""Kept GLS Jacobians follow local updates: relinearize_dirty of what DevicePlan.linearize / linearize_reduced /
linearize_points return (GlsDirtyJacobian, GlsDirtyReducedJacobian, GlsShapeJacobian), Grid.mark_dirty and the update() of the scipy
operators.

The yardstick everywhere is a FRESH object's full linearisation at the same state -- the unchanged path that
tests/test_gpu_gls_jacobian.py, test_gpu_gls_reduced_jacobian.py and test_gpu_gls_shape_jacobian.py hold to the 80-bit models -- so
every comparison is tobytes() equality and there is no tolerance.

The meshes, the Neumann plane z = 0 and the ALH tensor are those of tests/test_gpu_gls_shape_adjoint.py (each mesh loaded again here:
these tests rewrite K, the points and the flags); the random-cloud Delaunay mesh populates every bin of the adjoint kernel.  Every
check runs for the K Jacobian ("K"), the reduced one with the resident permeability as its one basis tensor ("R1") and with six tensors
per cell ("R6"), and the shape Jacobian ("X").  Every test starts from the same baseline: the original K, points and flags written
whole (which makes every node dirty), an object linearised at (u0, b0), the dirty set cleared."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the child process of test_forced_global_class: the paths tests/conftest.py sets up
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import test_gpu_gls_shape_adjoint as SA  # noqa: E402
from ninpol_amd import mesh as M  # noqa: E402

pytestmark = pytest.mark.gpu

MESHES = SA.MESHES
KINDS = ("K", "R1", "R6", "X")
N_DIR = 5


def _torch():
    import torch
    return torch


class Case:
    """one mesh on the device (its own Interpolator), the original tables on the host and on the device, two cell fields and two sets of
    node values, directions for the products"""

    def __init__(self, name):
        import ninpol_amd
        from ninpol_amd.interpolator import DevicePlan
        torch = _torch()
        self.name = name
        mesh = M.attach_fields(MESHES[name](), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
        self.I = I = ninpol_amd.Interpolator()
        I.load_mesh(mesh_obj=mesh)
        self.plan = DevicePlan(I, "u", "gls")
        g = self.grid = I.grid
        self.P, self.E, self.nnz = int(g.n_points), int(g.n_elems), int(g.nnz_esup)
        self.dev = torch.device("cuda", int(I.device))
        perm, _ = I._perm_rows()
        self.K0 = np.array(perm).reshape(self.E, 9)
        self.X0 = np.array(g.point_coords, dtype=np.float64).reshape(self.P, 3)
        self.flag0 = np.array(np.asarray(I.points_data)[I.variable_to_index["points"]["neumann_flag_u"]][:self.P]).astype(np.int64)
        self.inpoel = np.array(g.inpoel).astype(np.int64)
        self.boundary = np.asarray(g.boundary_points).astype(np.int64) != 0
        self.node_of_esup = np.repeat(np.arange(self.P), np.diff(np.asarray(g.esup_ptr).astype(np.int64)))
        self.node_of_fsup = np.repeat(np.arange(self.P), np.diff(np.asarray(g.fsup_ptr).astype(np.int64)))
        rng = np.random.default_rng(71)
        self.u0, self.b0 = rng.uniform(-1.0, 1.0, self.E), rng.uniform(-1.0, 1.0, self.P)
        self.u2 = self.u0 + rng.uniform(0.5, 1.0, self.E)                # differs from u0 (and from every u1 below) everywhere
        self.basis6 = self.to_dev(rng.uniform(-1.0, 1.0, (self.E, 6, 9)))
        self.d = {"K": rng.uniform(-1.0, 1.0, (N_DIR, self.E, 9)), "R1": rng.uniform(-1.0, 1.0, (N_DIR, self.E, 1)),
                  "R6": rng.uniform(-1.0, 1.0, (N_DIR, self.E, 6)), "X": rng.uniform(-1.0, 1.0, (N_DIR, self.P, 3))}
        self.vs = rng.uniform(-1.0, 1.0, (N_DIR, self.P))
        self.rng = rng

    # ---- plumbing ----
    def stream(self):
        return _torch().cuda.current_stream(self.dev).cuda_stream

    def sync(self):
        _torch().cuda.synchronize(self.dev)

    def to_dev(self, a, dtype=np.float64):
        return _torch().from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def vertices(self, cells):
        v = self.inpoel[np.asarray(cells, dtype=np.int64)]
        return np.unique(v[v >= 0])

    def around(self, nodes):
        """the vertices of the cells around `nodes`: what a local move of those nodes marks"""
        return self.vertices(np.nonzero(np.isin(self.inpoel, nodes).any(axis=1))[0])

    # ---- the three objects behind one interface ----
    def fresh(self, kind, u, b):
        ud, bd = self.to_dev(u), self.to_dev(b)
        if kind == "K":
            J = self.plan.linearize(ud.data_ptr(), bd.data_ptr(), self.stream())
        elif kind == "R1":
            J = self.plan.linearize_reduced(ud.data_ptr(), 1, 0, True, bd.data_ptr(), self.stream())
        elif kind == "R6":
            J = self.plan.linearize_reduced(ud.data_ptr(), 6, self.basis6.data_ptr(), True, bd.data_ptr(), self.stream())
        else:
            J = self.plan.linearize_points(ud.data_ptr(), bd.data_ptr(), self.stream())
        self.sync()
        return J

    def never_linearised(self, kind):
        from ninpol_amd.interpolator import GlsDirtyJacobian, GlsDirtyReducedJacobian, GlsShapeJacobian
        if kind == "K":
            return GlsDirtyJacobian(self.grid, plan=self.plan)
        if kind in ("R1", "R6"):
            return GlsDirtyReducedJacobian(self.grid, int(kind[1]), plan=self.plan)
        return GlsShapeJacobian(self.grid, plan=self.plan)

    def redo(self, J, kind, u, b, clear=True):
        ud, bd = self.to_dev(u), self.to_dev(b)
        if kind == "R1":
            n = J.relinearize_dirty(ud.data_ptr(), 0, True, bd.data_ptr(), self.stream(), clear=clear)
        elif kind == "R6":
            n = J.relinearize_dirty(ud.data_ptr(), self.basis6.data_ptr(), True, bd.data_ptr(), self.stream(), clear=clear)
        else:
            n = J.relinearize_dirty(ud.data_ptr(), bd.data_ptr(), self.stream(), clear=clear)
        self.sync()
        return n

    def buffers(self, J, kind):
        """[(name, array, node of every row or None for a buffer that is recomputed whole)]"""
        if kind == "K":
            contrib, fold = J.fetch()
            return [("contrib", contrib, self.node_of_esup), ("fold", fold, None)]
        if kind in ("R1", "R6"):
            return [("R", J.fetch(), self.node_of_esup)]
        cell, face, own = J.fetch()
        return [("cell", cell, self.node_of_esup), ("face", face, self.node_of_fsup), ("own", own, np.arange(self.P))]

    def products(self, J, kind):
        """launch_jvp and launch_vjp for n = 1 and N_DIR, each into a NaN-filled buffer"""
        torch = _torch()
        per = {"K": (self.E, 9), "R1": (self.E, 1), "R6": (self.E, 6), "X": (self.P, 3)}[kind]
        out = []
        for n in (1, N_DIR):
            xd, vd = self.to_dev(self.d[kind][:n]), self.to_dev(self.vs[:n])
            jv = torch.full((n, self.P), float("nan"), dtype=torch.float64, device=self.dev)
            vj = torch.full((n,) + per, float("nan"), dtype=torch.float64, device=self.dev)
            J.launch_jvp(xd.data_ptr(), jv.data_ptr(), n=n, stream=self.stream())
            J.launch_vjp(vd.data_ptr(), vj.data_ptr(), n=n, stream=self.stream())
            self.sync()
            out += [jv.cpu().numpy(), vj.cpu().numpy()]
        assert all(np.all(np.isfinite(a)) for a in out)
        return out

    def assembled(self, J):
        torch = _torch()
        n = J.pattern(self.stream())[0]
        vals = torch.full((n, 3), float("nan"), dtype=torch.float64, device=self.dev)
        J.launch_assemble(vals.data_ptr(), self.stream())
        self.sync()
        return vals.cpu().numpy()

    def same(self, J, kind, F, what, products=True):
        for (name, a, _), (_, b, _) in zip(self.buffers(J, kind), self.buffers(F, kind)):
            assert a.tobytes() == b.tobytes(), (self.name, kind, what, name, int(np.count_nonzero(a != b)))
        if products:
            for i, (a, b) in enumerate(zip(self.products(J, kind), self.products(F, kind))):
                assert a.tobytes() == b.tobytes(), (self.name, kind, what, "product", i)
        assert J.is_current() and J.stamp == F.stamp

    # ---- the state of the grid ----
    def baseline(self, kind=None):
        """the original K, points and flags written whole, the object linearised at (u0, b0), the dirty set cleared"""
        I = self.I
        I.update_permeability(self.to_dev(self.K0))
        I.update_points(self.to_dev(self.X0))
        I.update_neumann_flags("u", self.to_dev(self.flag0, np.uint8))
        J = self.fresh(kind, self.u0, self.b0) if kind else None
        self.grid.clear_dirty(self.stream())
        self.sync()
        assert self.grid.dirty_nodes == 0
        return J

    def some_cells(self, seed=0):
        """about 5 % of the cells, new rows for them (the old ones scaled: still symmetric positive definite) and a u that differs there"""
        rng = np.random.default_rng(100 + seed)
        ids = np.sort(rng.choice(self.E, max(2, self.E // 20), replace=False))
        rows = self.K0[ids] * rng.uniform(1.5, 3.0, (len(ids), 1))
        u1 = self.u0.copy()
        u1[ids] += rng.uniform(0.5, 1.0, len(ids))
        return ids, rows, u1

    def update_cells(self, ids, rows):
        self.I.update_permeability(self.to_dev(rows), cells=self.to_dev(ids, np.int64))


_CASES = {}


def get_case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=sorted(MESHES))
def case(request):
    return get_case(request.param)


@pytest.fixture(params=KINDS)
def kind(request):
    return request.param


def test_every_bin_is_populated_on_the_delaunay_mesh():
    c = get_case("delaunay")
    c.baseline("K")
    plan = c.grid.gls_adjoint_plan()
    assert list(plan) == ["lds1", "lds2", "lds4", "global"] and all(v > 0 for v in plan.values()), plan
    assert sum(plan.values()) == c.P


# ---- 1 and 2: the permeability; exactly the marked rows ------------------------------------------------------------------------------

def check_permeability(c, kind):
    J = c.baseline(kind)
    ids, rows, u1 = c.some_cells()
    marked = c.vertices(ids)
    c.update_cells(ids, rows)
    assert not J.is_current()
    n = c.redo(J, kind, u1, c.b0)
    assert n == len(marked) and 0 < n < c.P, (c.name, kind, n, len(marked), c.P)
    assert c.grid.dirty_nodes == 0
    F1 = c.fresh(kind, u1, c.b0)
    c.same(J, kind, F1, "permeability")
    return J, F1, ids, rows, marked


def test_permeability(case, kind):
    check_permeability(case, kind)


def test_exactly_the_marked_rows(case, kind):
    c = case
    J, F1, ids, rows, marked = check_permeability(c, kind)
    c.update_cells(ids, rows)                       # the same rows again: K stays, the same nodes are marked
    n = c.redo(J, kind, c.u2, c.b0)
    assert n == len(marked)
    F2 = c.fresh(kind, c.u2, c.b0)
    is_marked = np.zeros(c.P, dtype=bool)
    is_marked[marked] = True
    for (name, a, node), (_, f1, _), (_, f2, _) in zip(c.buffers(J, kind), c.buffers(F1, kind), c.buffers(F2, kind)):
        if node is None:                            # fold: recomputed whole, from the same K
            assert a.tobytes() == f2.tobytes() == f1.tobytes()
            continue
        m = is_marked[node]
        assert m.any() and not m.all()
        assert a[m].tobytes() == f2[m].tobytes(), (c.name, kind, name, "a marked row is not the one at u2")
        assert a[~m].tobytes() == f1[~m].tobytes(), (c.name, kind, name, "an unmarked row was touched")
        assert f1[~m].tobytes() != f2[~m].tobytes()  # (u2 does move the unmarked rows: the check above is not empty)


# ---- 3: the points ---------------------------------------------------------------------------------------------------------------------

def test_points(case, kind):
    c = case
    J = c.baseline(kind)
    pattern = tuple(a.copy() for a in J.fetch_pattern()) if kind == "X" else None
    rng = np.random.default_rng(5)
    ids = np.sort(rng.choice(c.P, max(2, c.P // 40), replace=False))
    rows = c.X0[ids] + rng.uniform(-0.01, 0.01, (len(ids), 3))
    marked = c.around(ids)
    c.I.update_points(c.to_dev(rows), nodes=c.to_dev(ids, np.int64))
    if kind == "X":                                  # the records are applied through the resident geometry: refused until relinearised
        from ninpol_amd import _lib
        with pytest.raises(_lib.NinpolError) as e:
            c.products(J, kind)
        assert e.value.code == _lib.NIN_ESTATE
    n = c.redo(J, kind, c.u0, c.b0)
    assert n == len(marked) and 0 < n < c.P, (c.name, kind, n, len(marked))
    F = c.fresh(kind, c.u0, c.b0)
    c.same(J, kind, F, "points")
    if kind == "X":
        after = J.fetch_pattern()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pattern, after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(pattern, F.fetch_pattern()))
        assert c.assembled(J).tobytes() == c.assembled(F).tobytes()


# ---- 4: the flags ----------------------------------------------------------------------------------------------------------------------

def test_flags(case, kind):
    c = case
    J = c.baseline(kind)
    on, off = np.nonzero(c.boundary & (c.flag0 != 0))[0], np.nonzero(c.boundary & (c.flag0 == 0))[0]
    assert len(on) >= 2 and len(off) >= 2
    to_dirichlet, to_neumann = on[:: max(1, len(on) // 3)][:3], off[:: max(1, len(off) // 3)][:3]
    ids = np.concatenate([to_dirichlet, to_neumann])
    values = np.concatenate([np.zeros(len(to_dirichlet)), np.ones(len(to_neumann))])
    c.I.update_neumann_flags("u", c.to_dev(values), nodes=c.to_dev(ids, np.int64))
    n = c.redo(J, kind, c.u0, c.b0)
    assert n == len(ids) and 0 < n < c.P
    F = c.fresh(kind, c.u0, c.b0)
    c.same(J, kind, F, "flags")
    for name, a, node in c.buffers(J, kind):
        if node is not None:
            assert not a[np.isin(node, to_dirichlet)].any(), (c.name, kind, name, "a node turned Dirichlet keeps records")
    got = np.asarray(c.grid.fetch_flags()).astype(np.int64)
    assert not got[to_dirichlet].any() and got[to_neumann].all()


# ---- 5: marks without an update ----------------------------------------------------------------------------------------------------

def test_mark_dirty(case, kind):
    c = case
    J = c.baseline(kind)
    ids, _, u1 = c.some_cells(seed=1)
    stamp = J.stamp
    c.grid.mark_dirty(cells=c.to_dev(ids, np.int32))                  # (int32 ids on the device)
    marked = c.vertices(ids)
    assert c.grid.dirty_nodes == len(marked) and J.is_current()      # K, the points and the flags did not change
    assert c.redo(J, kind, u1, c.b0) == len(marked)
    c.same(J, kind, c.fresh(kind, u1, c.b0), "mark_dirty(cells=)", products=False)
    nodes = np.sort(np.random.default_rng(9).choice(c.P, max(2, c.P // 30), replace=False))
    b1 = c.b0.copy()
    b1[nodes] += 1.0
    c.grid.mark_dirty(nodes=nodes)                                     # (numpy ids: checked on the host, marked before the call returns)
    assert c.grid.dirty_nodes == len(nodes)
    assert c.redo(J, kind, u1, b1) == len(nodes) and J.stamp == stamp
    c.same(J, kind, c.fresh(kind, u1, b1), "mark_dirty(nodes=)")


def test_mark_dirty_argument_errors():
    c = get_case("hex")
    c.baseline()
    g, torch = c.grid, _torch()
    for kw in ({}, {"cells": [0], "nodes": [0]}):
        with pytest.raises(ValueError, match="exactly one"):
            g.mark_dirty(**kw)
    with pytest.raises(TypeError, match="must be integers"):
        g.mark_dirty(nodes=np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="must have shape"):
        g.mark_dirty(cells=np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match=r"must lie in \[0, %d\)" % c.E):
        g.mark_dirty(cells=[0, c.E])
    with pytest.raises(ValueError, match=r"must lie in \[0, %d\)" % c.P):
        g.mark_dirty(nodes=[-1])
    with pytest.raises(TypeError, match="int32 or int64"):
        g.mark_dirty(nodes=torch.zeros(2, dtype=torch.float64, device=c.dev))
    with pytest.raises(ValueError, match="must have shape"):
        g.mark_dirty(nodes=torch.zeros((2, 2), dtype=torch.int64, device=c.dev))
    assert g.dirty_nodes == 0                                          # a refused call marked nothing
    g.mark_dirty(nodes=np.zeros(0, dtype=np.int64))                    # nothing to mark is not an error
    g.mark_dirty(nodes=torch.tensor([1, 1, 3], device=c.dev), stream=c.stream())
    c.sync()
    assert g.dirty_nodes == 2


# ---- 6: special states -------------------------------------------------------------------------------------------------------------

def test_everything_dirty(case, kind):
    c = case
    J = c.baseline(kind)
    ids, rows, u1 = c.some_cells(seed=2)
    c.update_cells(ids, rows)
    c.grid.mark_all_dirty()
    assert c.grid.dirty_nodes == -1
    assert c.redo(J, kind, c.u2, c.b0) == c.P                          # u2 differs everywhere: only a full pass can follow it
    assert c.grid.dirty_nodes == 0
    c.same(J, kind, c.fresh(kind, c.u2, c.b0), "everything dirty")


def test_empty_set(case, kind):
    c = case
    J = c.baseline(kind)
    before = [a.copy() for _, a, _ in c.buffers(J, kind)]
    nodes = np.nonzero(c.boundary)[0][:4]
    c.I.update_neumann_flags("u", c.to_dev(c.flag0[nodes], np.uint8), nodes=c.to_dev(nodes, np.int64))     # equal values: an update that marks nothing
    assert not J.is_current() and c.grid.dirty_nodes == 0
    assert c.redo(J, kind, c.u2, c.b0) == 0                            # whatever u holds: no row is in the set
    assert J.is_current()
    for a, (name, b, _) in zip(before, c.buffers(J, kind)):
        assert a.tobytes() == b.tobytes(), (c.name, kind, name)
    c.products(J, kind)                                                # (and the shape Jacobian answers)


def test_clear_false_serves_several_consumers(case):
    c, torch = case, _torch()
    c.baseline()
    w = torch.full((c.nnz,), float("nan"), dtype=torch.float64, device=c.dev)
    nws = torch.full((c.P,), float("nan"), dtype=torch.float64, device=c.dev)
    c.plan.launch(w.data_ptr(), nws.data_ptr(), c.stream())
    JK, JX = c.fresh("K", c.u0, c.b0), c.fresh("X", c.u0, c.b0)
    ids, rows, u1 = c.some_cells(seed=3)
    marked = c.vertices(ids)
    c.update_cells(ids, rows)
    assert c.redo(JK, "K", u1, c.b0, clear=False) == len(marked)
    assert c.grid.dirty_nodes == len(marked)
    assert c.redo(JX, "X", u1, c.b0, clear=False) == len(marked)
    assert c.plan.launch_dirty(w.data_ptr(), nws.data_ptr(), c.stream(), clear=True) == len(marked)
    c.sync()
    assert c.grid.dirty_nodes == 0
    w2, nws2 = torch.full_like(w, float("nan")), torch.full_like(nws, float("nan"))
    c.plan.launch(w2.data_ptr(), nws2.data_ptr(), c.stream())
    c.sync()
    assert w.cpu().numpy().tobytes() == w2.cpu().numpy().tobytes() and nws.cpu().numpy().tobytes() == nws2.cpu().numpy().tobytes()
    c.same(JK, "K", c.fresh("K", u1, c.b0), "clear=False", products=False)
    c.same(JX, "X", c.fresh("X", u1, c.b0), "clear=False", products=False)


def test_refused_ids(case, kind):
    from ninpol_amd import _lib
    c = case
    J = c.baseline(kind)
    before = [a.copy() for _, a, _ in c.buffers(J, kind)]
    stamp = J.stamp
    ids, rows, u1 = c.some_cells(seed=4)
    bad = np.concatenate([ids, [c.E + 5, -1]])
    c.update_cells(bad, np.concatenate([rows, rows[:2]]))
    with pytest.raises(_lib.NinpolError) as e:
        c.redo(J, kind, u1, c.b0)
    assert e.value.code == _lib.NIN_EINVAL and e.value.text.startswith("2 cell ids outside [0, %d)" % c.E), e.value.text
    assert "nothing was launched, the dirty set is kept" in e.value.text
    assert J.stamp == stamp
    for a, (name, b, _) in zip(before, c.buffers(J, kind)):
        assert a.tobytes() == b.tobytes(), (c.name, kind, name)
    marked = c.vertices(ids)
    assert c.redo(J, kind, u1, c.b0) == len(marked)                   # the good ids were written and marked: the next call goes through
    c.same(J, kind, c.fresh(kind, u1, c.b0), "after refused ids", products=False)


def test_never_linearised(kind):
    from ninpol_amd import _lib
    c = get_case("hex")
    c.baseline()
    J = c.never_linearised(kind)
    with pytest.raises(_lib.NinpolError) as e:
        c.redo(J, kind, c.u0, c.b0)
    assert e.value.code == _lib.NIN_ESTATE and "has not been linearised" in e.value.text
    assert J.stamp == (-1, -1, -1)


def test_the_seed_buffer_is_counted(kind):
    c = get_case("tet")
    J = c.baseline(kind)
    before = J.nbytes
    c.grid.mark_dirty(nodes=[0, 1])
    assert c.redo(J, kind, c.u0, c.b0) == 2 and J.nbytes == before + 8 * c.nnz
    c.grid.mark_dirty(nodes=[2])
    assert c.redo(J, kind, c.u0, c.b0) == 1 and J.nbytes == before + 8 * c.nnz     # made once, kept
    c.grid.release_scratch()                                           # the bins and the per-node bin byte go, and come back
    c.grid.mark_dirty(nodes=[0, 3])
    assert c.redo(J, kind, c.u0, c.b0) == 2
    c.same(J, kind, c.fresh(kind, c.u0, c.b0), "after release_scratch")


# ---- 7: determinism, and every system in global-memory scratch ---------------------------------------------------------------------

def test_two_dirty_calls_agree_bit_for_bit(case, kind):
    c = case
    Ja = c.baseline(kind)
    Jb = c.fresh(kind, c.u0, c.b0)
    ids, rows, u1 = c.some_cells(seed=6)
    c.update_cells(ids, rows)
    na = c.redo(Ja, kind, u1, c.b0, clear=False)
    nb = c.redo(Jb, kind, u1, c.b0, clear=False)
    first = [a.copy() for _, a, _ in c.buffers(Ja, kind)]
    assert na == nb == c.redo(Ja, kind, u1, c.b0, clear=True)
    for a, (name, b, _), (_, b2, _) in zip(first, c.buffers(Ja, kind), c.buffers(Jb, kind)):
        assert a.tobytes() == b.tobytes() == b2.tobytes(), (c.name, kind, name)


def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    c = get_case("hex")
    for kind in KINDS:
        check_permeability(c, kind)
    plan = c.grid.gls_adjoint_plan()
    assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": c.P}, plan
    print("CHILD OK")


def test_forced_global_class():
    """the hexahedron mesh again with every system in global-memory scratch, in a fresh process (the switch is read when the bins are
    made)"""
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


# ---- 8: the scipy layer ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ("permeability", "reduced", "points"))
def test_scipy_operators_update(which):
    import ninpol_amd
    mesh = M.attach_fields(MESHES["mixed"](), "u", perm="ALH", neumann_plane=(2, 0.0), seed=3)
    I = ninpol_amd.Interpolator()
    I.load_mesh(mesh_obj=mesh)
    g = I.grid
    P, E = int(g.n_points), int(g.n_elems)
    rng = np.random.default_rng(23)
    u0, b = rng.uniform(-1.0, 1.0, E), rng.uniform(-1.0, 1.0, P)
    basis = rng.uniform(-1.0, 1.0, (E, 3, 9)) if which == "reduced" else None

    def make(u):
        if which == "points":
            return I.points_jacobian("u", u, b)
        return I.permeability_jacobian("u", u, b, basis=basis)

    op = make(u0)
    g.clear_dirty()
    inpoel = np.array(g.inpoel).astype(np.int64)
    if which == "points":
        ids = np.sort(rng.choice(P, 3, replace=False))
        X = np.array(g.point_coords, dtype=np.float64).reshape(P, 3)
        I.update_points(X[ids] + rng.uniform(-0.01, 0.01, (3, 3)), nodes=ids)
        v = inpoel[np.isin(inpoel, ids).any(axis=1)]
        u1 = u0
        with pytest.raises(RuntimeError):
            op @ np.ones(op.shape[1])
    else:
        ids = np.sort(rng.choice(E, max(2, E // 20), replace=False))
        K = np.array(I._perm_rows()[0]).reshape(E, 9)
        I.update_permeability(2.0 * K[ids], cells=ids)
        v = inpoel[ids]
        u1 = u0.copy()
        u1[ids] += 1.0
    marked = np.unique(v[v >= 0])
    n = op.update(u1, b)
    assert n == len(marked) and 0 < n < P, (n, len(marked))
    new = make(u1)
    x, y = rng.uniform(-1.0, 1.0, op.shape[1]), rng.uniform(-1.0, 1.0, P)
    assert (op @ x).tobytes() == (new @ x).tobytes() and (op.T @ y).tobytes() == (new.T @ y).tobytes()
    A, B = (op.assemble(), new.assemble()) if which == "points" else (op.to_scipy(), new.to_scipy())
    assert A.data.tobytes() == B.data.tobytes() and A.indices.tobytes() == B.indices.tobytes() and A.indptr.tobytes() == B.indptr.tobytes()
    assert op.jacobian.is_current()
    assert op.update(u1, b) == 0                                       # nothing is dirty any more


if __name__ == "__main__":
    _child()
