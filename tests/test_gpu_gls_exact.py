"""Every GLS kernel of the launch plan against the 80-bit solution of the same float64 system (tests/gls_exact.py; the yardstick
itself is validated in tests/test_gls_exact.py).  The parity tests ask "within WEIGHT_RTOL = 1e-10 of the oracle"; on most cases
the oracle is 1e-14 .. 3e-11 from exact, so that bar leaves up to four digits unexamined.  Here, for a pool S of sampled nodes that
one kernel (or one kernel family) computed, with the oracle run on the same mesh in the same test:

    dist(hip[S], exact[S])  <=  min(slack x dist(oracle[S], exact[S]), WEIGHT_RTOL)        (weights, and neumann_ws likewise;
                                                                                            never below RESOLUTION = 4 ulp)

slack = util.gls_exact_slack(kernel): util.FAN_EXACT_SLACK unless util.py gives the kernel a value of its own with the reason.
The bar is on the maxima of a pool, never per node (a single node's ratio reaches 3.6 for a correct elimination).

  * unit box: the meshes of gls_exact.unit_cases() with the ALH and the FAN tensor; which kernel owns which rows comes from
    util.gls_kernel_owners (NIN_GLS_ONLY); per kernel up to 32 computed nodes (the 8 with the most cells + a seeded draw);
    a kernel with fewer than 16 sampled nodes on a case is pooled with its family;
  * every entry of util.GLS_ROUTES forced on four small meshes, the plan asserted to have changed as the route says;
  * off the unit box and beyond eta = 1 (gls_exact.TRANSFORMS): grid arrays, IDW / LS, GLS against the oracle, GLS against exact.
One line per (case, pool) is printed (`pytest -s`): nodes, the oracle's distance, the HIP path's, the ratio."""
import numpy as np
import pytest

import gls_exact as X
import util
from ninpol_amd import mesh as M

pytestmark = pytest.mark.gpu

TIGHT = 1e-14
FAMILIES = {"block*+scratch": ("block1", "block2", "block4", "block8", "scratch"), "small*": ("small4", "small8", "small12"),
            "mfx_*": ("mfx_6x10", "mfx_7x11", "mfx_8x13", "mfx_9x15", "mfx_10x16", "mfx_boundary", "mfx_4x7", "mfx_7x12"),
            "mfw_*": ("mfw_large", "mfw_small", "mfw_general")}
FAMILY_OF = {k: fam for fam, ks in FAMILIES.items() for k in ks}
POOL_MIN = 16
# What the yardstick itself resolves: the exact rows are ROUNDED to float64 (half an ulp of each entry) and both computed rows are
# float64 (one ulp apart at the row's scale), so a distance is known to +- 1.5 ulp of the row's largest weight and no bar is set
# below 4 ulp = 8.9e-16 -- on one-node pools of the ALH tensor the oracle's distance itself is 2 .. 4 ulp.
RESOLUTION = 4 * np.finfo(np.float64).eps
# Every kernel of the plan that the default routing can give a regular node.  Two cannot get one and are held to the bar by forced
# routes instead (test_kernels_outside_the_default_routing): kernels_gls_mfw.hip's general kind runs only behind
# NIN_GLS_MFW_GENERAL; and the block kernel's one-wavefront class takes a 3-D node only if the small-node kernel refuses it (more
# than 12 cells, or more than 64 rows) AND (n + 1) (m | 1) doubles fit 10 KiB of LDS (device_grid.hpp): with ne >= 13 cells a system
# that has a solution row has n + 1 >= 41 columns and m >= 40 rows -- 1681 doubles; with m > 64 rows, 65 (n + 1) <= 1280 leaves at most 5 cells,
# which have at most 15 faces around the node: m <= 50.  Neither exists.
ROUTED_ONLY = {"mfw_general": ("general_kind", "mixed"), "block1": ("block_only", "hex")}
DEFAULT_KERNELS = lambda names: [k for k in names if k not in ROUTED_ONLY]


def _interp():
    import ninpol_amd
    return ninpol_amd.Interpolator()


class _Case:
    """One mesh with its fields: the oracle's rows, and exact rows on demand (each node solved once, whatever the route)."""

    def __init__(self, oracle_lib, mesh, label):
        self.mesh, self.label = mesh, label
        self.o = oracle_lib.OracleInterpolator("port", threads=8)
        self.o.load_mesh(mesh)
        self.G = self.o.grid
        self.wo, self.no = self.o.prepare("gls", "u")
        self.flag = mesh.point_data["neumann_flag_u"].astype(bool)
        self.computed = X.computed_nodes(self.G, self.flag)
        self.ne = np.diff(np.asarray(self.G.esup_ptr))
        self._exact = {}

    def exact(self, nodes):
        """(exact rows, exact neumann_ws, keep) of `nodes`; keep = the exact solve is regular and the oracle's row is not all zero"""
        new = [int(p) for p in nodes if int(p) not in self._exact]
        if new:
            rows, ok = X.exact_rows(self.o, self.mesh, "u", new)
            for p, r, k in zip(new, rows, ok):
                self._exact[p] = (r, bool(k))
        rows = np.array([self._exact[int(p)][0] for p in nodes]).reshape(len(nodes), -1)
        ok = np.array([self._exact[int(p)][1] for p in nodes], dtype=bool)
        nws = X.exact_neumann_ws(rows, ok, self.G, self.flag, nodes)
        return rows, nws, ok & np.abs(self.wo[nodes]).any(axis=1)

    def run(self, switches=()):
        """the HIP path under `switches`: (plan, weights and neumann_ws of all nodes, {kernel: the computed nodes it owns})"""
        with pytest.MonkeyPatch.context() as mp:
            for sw in switches:
                mp.setenv(sw, "1")
            I = _interp()
            I.load_mesh(mesh_obj=self.mesh)
            I.grid.to_device(0)
            plan = I.grid.gls_plan()
            P = int(I.grid.n_points)
            w, nw = I.prepare_interpolator("gls", "u", np.arange(P))
            owners = util.gls_kernel_owners(I, plan)
        seen = np.zeros(P, dtype=np.int64)
        for name, (mine, _, _) in owners.items():
            assert len(mine) == plan[name], name
            seen[mine] += 1
        assert seen.min() == 1 and seen.max() == 1, "every row is written by exactly one kernel"
        assert sum(plan.values()) == P
        neu = self.computed[self.flag[self.computed]]
        same = nw[neu] == w[neu, self.ne[neu] - 1]
        print(f"{self.label} {'+'.join(switches) or 'default'}: neumann_ws is the last cell's weight bit for bit on {int(same.sum())} of {len(neu)} Neumann nodes")
        return plan, w, nw, {k: np.intersect1d(v[0], self.computed) for k, v in owners.items()}, I

    def pools(self, owned, what, by_family=False):
        """{pool name: (kernels, sampled nodes, which of the kernels owns each)}: per kernel the seeded sample of its computed nodes;
        a kernel with fewer than POOL_MIN of them (by_family: every kernel) joins its family's pool"""
        pools = {}
        for name, nodes in owned.items():
            s = X.sample_nodes(nodes, self.G, f"{self.label}/{what}/{name}")
            if not len(s):
                continue
            fam = FAMILY_OF.get(name)
            key = fam if fam and (by_family or len(s) < POOL_MIN) else name
            ks, ns, who = pools.get(key, ((), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))
            pools[key] = (ks + (name,), np.concatenate([ns, s]), np.concatenate([who, np.full(len(s), len(ks))]))
        return pools

    def hold(self, w, nw, pools, what):
        """The bar on every pool; prints one line each.  Returns (failures, the kernels that contributed a node)."""
        failures, contributed = [], set()
        for key, (kernels, nodes, who) in pools.items():
            exact, nws, keep = self.exact(nodes)
            nodes, exact, nws, who = nodes[keep], exact[keep], nws[keep], who[keep]
            if not len(nodes):
                print(f"{self.label} {what} {key}: no regular node in the sample of {kernels}")
                continue
            slack = max(util.gls_exact_slack(k) for k in kernels)
            d_o, d_h = X.dist(self.wo[nodes], exact), X.dist(w[nodes], exact)
            n_o = X.dist_scaled(np.abs(self.no[nodes] - nws), exact)
            n_h = X.dist_scaled(np.abs(nw[nodes] - nws), exact)
            n_neu = int(self.flag[nodes].sum())
            bound, nbound = min(max(slack * d_o, RESOLUTION), util.WEIGHT_RTOL), min(max(slack * n_o, RESOLUTION), util.WEIGHT_RTOL)
            name = key if kernels == (key,) else f"{key}[{'+'.join(kernels)}]"
            print(f"{self.label} | {what} | {name} | {len(nodes)} nodes ({n_neu} Neumann, up to {int(self.ne[nodes].max())} cells) | "
                  f"oracle {d_o:.2e} | HIP {d_h:.2e} | ratio {d_h / d_o if d_o else float('inf') if d_h else 0.0:.2f} | "
                  f"neumann_ws: oracle {n_o:.2e} HIP {n_h:.2e} ratio {n_h / n_o if n_o else float('inf') if n_h else 0.0:.2f}")
            if not d_h <= bound:
                failures.append((what, name, "weights", d_h, d_o, bound))
            if not n_h <= nbound:
                failures.append((what, name, "neumann_ws", n_h, n_o, nbound))
            contributed.update(kernels[i] for i in set(who.tolist()))
        return failures, contributed


# ---- section 3: the unit box ------------------------------------------------------------------------------------------------

_UNIT = {}


def _unit(oracle_lib, name, perm):
    if (name, perm) not in _UNIT:
        case = _Case(oracle_lib, X.unit_mesh(name, perm), f"{name}/{perm}")
        plan, w, nw, owned, _ = case.run()
        print(f"{case.label} plan: { {k: v for k, v in plan.items() if v} }")
        pools = case.pools(owned, "default")
        failures, contributed = case.hold(w, nw, pools, "default")
        _UNIT[name, perm] = (plan, failures, contributed, set(pools))
    return _UNIT[name, perm]


@pytest.mark.parametrize("perm", X.TENSORS)
@pytest.mark.parametrize("name", list(X.unit_cases()))
def test_unit_box_kernels_against_exact(oracle_lib, name, perm):
    """Each kernel the case's plan holds, on its seeded sample, no further from exact than slack x the oracle's own distance."""
    plan, failures, contributed, _ = _unit(oracle_lib, name, perm)
    assert contributed, "no kernel contributed a node"
    assert not failures, failures


def test_every_kernel_of_the_plan_is_held_to_the_bar(oracle_lib):
    """Non-vacuity, from the plans: between them the unit-box cases give every kernel of Grid.PLAN_KERNELS that the default
    routing can produce a non-empty list, and every one contributes at least one regular node to a pool."""
    from ninpol_amd.grid import Grid
    total, contributed = {k: 0 for k in Grid.PLAN_KERNELS}, set()
    for name in X.unit_cases():
        for perm in X.TENSORS:
            plan, _, c, _ = _unit(oracle_lib, name, perm)
            for k in total:
                total[k] += plan[k]
            contributed |= c
    print("nodes per kernel over all unit-box cases:", total)
    assert total["mfw_general"] == 0 and not (contributed & set(ROUTED_ONLY))
    missing = [k for k in DEFAULT_KERNELS(Grid.PLAN_KERNELS) if not total[k] or k not in contributed]
    assert not missing, (missing, total)


# ---- forced routes ------------------------------------------------------------------------------------------------------------

ROUTE_MESHES = {"hex": lambda: M.hex_mesh(7, jitter=0.15, seed=11), "tet": lambda: M.tet_mesh(5, jitter=0.1, seed=11),
                "wedge": lambda: M.wedge_mesh(5, 4, 4, jitter=0.05, seed=11), "mixed": lambda: M.mixed_mesh(8, 4, 4, jitter=0.1, seed=11)}
_SMALL = FAMILIES["small*"]
_HEAVY = FAMILIES["block*+scratch"]
_sum = lambda plan, ks: sum(plan[k] for k in ks)


def _route_bites(route, d, r):
    """Does the route change which kernel (or which form of a kernel) computes some node of this mesh?  d: the default plan,
    r: the route's.  What the route promises of the plan is asserted here whether it bites or not."""
    every = sum(d.values())
    assert sum(r.values()) == every
    if route == "default":
        assert dict(r) == dict(d)
        return True
    if route == "no_cube_kernel":
        assert r["hex8"] == 0 and r["mfw_small"] >= d["mfw_small"] + d["hex8"]
        return d["hex8"] > 0
    if route == "mfw_lane_columns":          # (a form chosen at launch: both instantiations)
        assert r["hex8"] == 0
        return r["mfw_large"] + r["mfw_small"] > 0
    if route == "mfw_row_lanes":             # (at launch: the large instantiation)
        assert dict(r) == dict(d)
        return d["mfw_large"] > 0
    if route == "mfw_small_strips":          # (at launch: the small instantiation)
        assert r["hex8"] == 0
        return r["mfw_small"] > 0
    if route == "general_kind":
        assert (r["mfw_general"] > 0) == (r["mfx"] < d["mfx"]) and d["mfw_general"] == 0
        return r["mfw_general"] > 0
    if route == "no_general_kind":
        assert r["mfw_general"] == 0 and r["mfx"] == 0
        assert _sum(r, _HEAVY) + _sum(r, _SMALL) >= _sum(d, _HEAVY) + _sum(d, _SMALL) + d["mfx"]
        return d["mfx"] > 0
    if route == "wide_for_two_coloured":
        assert r["mfw_large"] == 0 and r["mfw_small"] == 0 and r["mfx"] >= d["mfw_large"] + d["mfx"]
        return d["mfw_large"] + d["mfw_small"] > 0
    if route == "no_quad_kernel":
        assert r["quad4"] == 0 and _sum(r, _SMALL) == _sum(d, _SMALL) + d["quad4"]
        return d["quad4"] > 0
    if route == "no_small_kernel":
        assert r["quad4"] == 0 and _sum(r, _SMALL) == 0
        return _sum(d, _SMALL) + d["quad4"] > 0
    if route == "small_where_it_fits":
        assert r["hex8"] == 0 and r["mfw_large"] == 0 and r["mfw_small"] == 0 and _sum(r, _SMALL) >= _sum(d, _SMALL)
        return d["hex8"] + d["mfw_large"] + d["mfw_small"] > 0
    if route == "no_boundary_in_wide":
        assert r["mfx_boundary"] == 0 and r["mfx"] == d["mfx"]
        return d["mfx_boundary"] > 0
    if route == "block_only":
        assert _sum(r, _HEAVY) == every
        return _sum(d, _HEAVY) < every
    if route == "global_scratch":
        assert all(r[k] == 0 for k in ("hex8", "mfw_large", "mfw_small", "mfw_general", "mfx", "mfx_boundary", "quad4") + _SMALL)
        return r["scratch"] > d["scratch"]
    raise KeyError(route)


# the mesh kinds on which each route must bite (elsewhere its plan is still checked and its rows are still held to the bar)
ROUTE_KINDS = {
    "default": ("hex", "tet", "wedge", "mixed"),
    "no_cube_kernel": ("hex", "mixed"),
    "mfw_lane_columns": ("hex", "tet", "wedge", "mixed"),
    "mfw_row_lanes": ("tet", "mixed"),
    "mfw_small_strips": ("hex", "wedge", "mixed"),
    "general_kind": ("mixed",),
    "no_general_kind": ("mixed",),
    "wide_for_two_coloured": ("tet", "wedge", "mixed"),
    "no_quad_kernel": ("hex", "wedge", "mixed"),
    "no_small_kernel": ("hex", "tet", "wedge", "mixed"),
    "small_where_it_fits": ("hex", "tet", "wedge", "mixed"),
    "no_boundary_in_wide": ("mixed",),
    "block_only": ("hex", "tet", "wedge", "mixed"),
    "global_scratch": ("hex", "tet", "wedge", "mixed"),
}
assert set(ROUTE_KINDS) == set(util.GLS_ROUTES) and all(ROUTE_KINDS.values()), "no route may run empty"

_ROUTE_CASES, _ROUTE_DEFAULT = {}, {}


def _route_case(oracle_lib, kind, perm):
    if (kind, perm) not in _ROUTE_CASES:
        mesh = M.attach_fields(ROUTE_MESHES[kind](), "u", perm=perm, neumann_plane=(2, 0.0), seed=7)
        case = _Case(oracle_lib, mesh, f"route {kind}/{perm}")
        _ROUTE_CASES[kind, perm] = case
        _ROUTE_DEFAULT[kind, perm] = case.run()[0]
    return _ROUTE_CASES[kind, perm], _ROUTE_DEFAULT[kind, perm]


_ROUTES = {}


def _route(oracle_lib, route, kind, perm):
    if (route, kind, perm) not in _ROUTES:
        case, d = _route_case(oracle_lib, kind, perm)
        plan, w, nw, owned, _ = case.run(util.GLS_ROUTES[route])
        print(f"{case.label} {route} plan: { {k: v for k, v in plan.items() if v} }")
        e = max(util.rowscaled_err(w, case.wo), util.rowscaled_err(nw, case.no))
        pools = case.pools(owned, route)
        failures, contributed = case.hold(w, nw, pools, route)
        _ROUTES[route, kind, perm] = (case.label, d, plan, e, failures, contributed, set(pools))
    return _ROUTES[route, kind, perm]


@pytest.mark.parametrize("perm", X.TENSORS)
@pytest.mark.parametrize("kind", list(ROUTE_MESHES))
@pytest.mark.parametrize("route", list(util.GLS_ROUTES))
def test_forced_routes_against_exact(oracle_lib, route, kind, perm):
    """Every way a node can reach a GLS kernel (util.GLS_ROUTES: the lane-column, row-lane and small-strip forms of the
    one-wavefront multifrontal kernel, its general kind, block-only, global scratch, ...) under the same bar, the plan asserted to
    have changed as the route says."""
    label, d, plan, e, failures, contributed, _ = _route(oracle_lib, route, kind, perm)
    assert _route_bites(route, d, plan) == (kind in ROUTE_KINDS[route]), (route, kind, dict(plan), dict(d))
    assert e <= util.WEIGHT_RTOL, e
    assert contributed
    assert not failures, failures


def test_kernels_outside_the_default_routing(oracle_lib):
    """The two kernels no unit-box case can reach (ROUTED_ONLY) contribute regular nodes to a pool through their forced routes."""
    for kernel, (route, kind) in ROUTED_ONLY.items():
        for perm in X.TENSORS:
            _, _, plan, _, failures, contributed, _ = _route(oracle_lib, route, kind, perm)
            assert plan[kernel] > 0 and kernel in contributed, (kernel, route, kind, perm, dict(plan))
            assert not [f for f in failures if kernel in f[1]], failures


# ---- section 4: off the unit box and beyond eta = 1 ----------------------------------------------------------------------------

@pytest.mark.parametrize("transform", list(X.TRANSFORMS))
@pytest.mark.parametrize("name", X.TRANSFORM_MESHES)
def test_off_the_unit_box_against_oracle_and_exact(oracle_lib, name, transform):
    """Size, stretch, offset, eta > 1 (fields attached on the unit mesh, then points <- points * A + b; or the LIN tensor scaled
    down): the grid arrays bit-equal to the oracle's, IDW and LS at 1e-14, GLS over all nodes at WEIGHT_RTOL -- the oracle is
    <= 7.5e-12 from exact on every one of these cases (tests/test_gls_exact.py), so a correct kernel must meet it -- and GLS on
    the sample against exact under the bar above, pooled by kernel family."""
    case = _Case(oracle_lib, X.transformed_mesh(name, transform), f"{name}/{transform}")
    plan, w, nw, owned, I = case.run()
    for k in util.GRID_SCALARS:
        assert int(getattr(I.grid, k)) == int(getattr(case.G, k)), k
    for k in util.GRID_ARRAYS:
        np.testing.assert_array_equal(np.asarray(getattr(I.grid, k)), np.asarray(getattr(case.G, k)), err_msg=k)
    full = np.arange(int(I.grid.n_points))
    for meth in ("idw", "ls"):
        wo, no = case.o.prepare(meth, "u")
        wm, nm = I.prepare_interpolator(meth, "u", full)
        e = max(util.rowscaled_err(wm, wo), util.rowscaled_err(nm, no))
        print(f"{case.label} {meth}: HIP vs oracle {e:.2e}")
        assert e <= TIGHT, (meth, e)
    e = max(util.rowscaled_err(w, case.wo), util.rowscaled_err(nw, case.no))
    print(f"{case.label} gls, all nodes: HIP vs oracle {e:.2e}")
    pools = case.pools(owned, "default", by_family=True)
    failures, contributed = case.hold(w, nw, pools, "default")
    assert e <= util.WEIGHT_RTOL, e
    assert contributed
    assert not failures, failures
