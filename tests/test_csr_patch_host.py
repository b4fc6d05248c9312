"""nin_csr_patch_rows (csrc/csr_patch.cpp) through ctypes, without a GPU: the host half of HostMatrix.update().  The yardstick is a
numpy model that rebuilds the matrix row by row; every comparison is bit for bit (np.array_equal)."""
import ctypes

import numpy as np
import pytest

SIZES = (1, 63, 64, 65, 1000)
MAX_ROW = 90
EINVAL, ERANGE = -1, -5


@pytest.fixture(scope="module")
def patch():
    from ninpol_amd import build as nbuild
    nbuild.build()
    from ninpol_amd import _lib
    return _lib.load().nin_csr_patch_rows


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def random_rows(rng, n, n_cols=5000, lengths=None):
    """n rows of 0 .. MAX_ROW sorted distinct columns with non-zero values (a NaN now and then: it survives eliminate_zeros)"""
    if lengths is None:
        lengths = rng.integers(0, MAX_ROW + 1, n)
    rows = []
    for k in lengths:
        cols = np.sort(rng.choice(n_cols, size=int(k), replace=False)).astype(np.int32)
        vals = rng.uniform(0.5, 2.0, int(k)) * rng.choice([-1.0, 1.0], int(k))
        if k and rng.random() < 0.1:
            vals[rng.integers(0, k)] = np.nan
        rows.append((cols, vals))
    return rows


def csr_of(rows):
    indptr = np.zeros(len(rows) + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(c) for c, _ in rows])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return indptr, cat([c for c, _ in rows] + [np.zeros(0, np.int32)], np.int32), cat([v for _, v in rows] + [np.zeros(0)], np.float64)


def pack_of(nodes, new_rows, new_nws):
    counts = np.array([len(new_rows[i][0]) for i in range(len(nodes))], dtype=np.int32)
    off = np.zeros(len(nodes) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    _, pi, pd = csr_of(new_rows)
    return {"nodes": np.ascontiguousarray(nodes, dtype=np.int32), "counts": counts, "off": off, "pi": pi, "pd": pd,
            "pn": np.ascontiguousarray(new_nws, dtype=np.float64)}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


class Case:
    """a random P-row matrix, its neumann_ws, and room for the out_* arrays (sentinel-filled, with slack behind the new matrix)"""

    def __init__(self, P, seed):
        self.rng = np.random.default_rng(seed)
        self.P = P
        self.rows = random_rows(self.rng, P)
        self.indptr, self.indices, self.data = csr_of(self.rows)
        self.nws = self.rng.uniform(-1.0, 1.0, P)

    def call(self, patch, pk, out=False, arrays=None, P=None, m=None):
        a = arrays or {}
        cap = len(self.indices) + MAX_ROW * len(pk["nodes"]) + 8
        self.out = (np.full(self.P + 1, -7, np.int32), np.full(cap, -7, np.int32), np.full(cap, -7.0)) if out else (None, None, None)
        get = lambda k, default: a[k] if k in a else default
        args = [get("indptr", self.indptr), get("indices", self.indices), get("data", self.data), get("nws", self.nws)]
        packs = [get(k, pk[k]) for k in ("nodes", "counts", "off", "pi", "pd", "pn")]
        outs = [get("out%d" % i, self.out[i]) for i in range(3)]
        return patch(self.P if P is None else P, *map(ptr, args), len(pk["nodes"]) if m is None else m, *map(ptr, packs), *map(ptr, outs))

    def model(self, nodes, new_rows, new_nws):
        rows = list(self.rows)
        nws = self.nws.copy()
        for i, p in enumerate(nodes):
            rows[int(p)] = new_rows[i]
            nws[int(p)] = new_nws[i]
        return csr_of(rows) + (nws,)

    def snapshot(self):
        return [x.copy() for x in (self.indptr, self.indices, self.data, self.nws)]

    def untouched(self, snap):
        return all(same(x, y) for x, y in zip((self.indptr, self.indices, self.data, self.nws), snap))


def node_sets(P, rng):
    """m = 0, 1 and P, a random subset in random order, the first and the last row"""
    sets = {"m0": np.zeros(0, np.int64), "m1": rng.choice(P, 1), "all": rng.permutation(P), "first": np.array([0]), "last": np.array([P - 1]),
            "ends": np.array([P - 1, 0])[: min(P, 2)], "some": rng.permutation(P)[: max(P // 3, 1)]}
    return sets


@pytest.mark.parametrize("P", SIZES)
def test_in_place_equal_counts_other_pattern(patch, P):
    for name, nodes in node_sets(P, np.random.default_rng(P)).items():
        c = Case(P, 100 + P)
        lengths = [len(c.rows[int(p)][0]) for p in nodes]
        new_rows = random_rows(c.rng, len(nodes), lengths=lengths)        # equal counts, other columns and values
        new_nws = c.rng.uniform(-1.0, 1.0, len(nodes))
        want = c.model(nodes, new_rows, new_nws)
        indptr0 = c.indptr.copy()
        assert c.call(patch, pack_of(nodes, new_rows, new_nws)) == 0, name
        assert same(c.indptr, indptr0) and same(c.indptr, want[0]), name
        assert same(c.indices, want[1]) and same(c.data, want[2]) and same(c.nws, want[3]), name
        if len(nodes) and sum(lengths):
            assert not same(c.indices, csr_of(c.rows)[1]), (name, "the pattern was not rewritten")


def _reshaped(c, nodes):
    """new rows for `nodes`: growing, shrinking, becoming empty, becoming non-empty, in turn"""
    lengths = []
    for i, p in enumerate(nodes):
        k = len(c.rows[int(p)][0])
        lengths.append((min(k + 1 + i % 7, MAX_ROW), max(k - 1 - i % 5, 0), 0, k if k else 3)[i % 4])
    return random_rows(c.rng, len(nodes), lengths=lengths)


@pytest.mark.parametrize("P", SIZES)
def test_new_structure(patch, P):
    for name, nodes in node_sets(P, np.random.default_rng(P + 1)).items():
        c = Case(P, 200 + P)
        if name in ("first", "last"):           # the first row: empty, then filled; the last row: filled, then empty
            c.rows[int(nodes[0])] = random_rows(c.rng, 1, lengths=[0 if name == "first" else 5])[0]
            c.indptr, c.indices, c.data = csr_of(c.rows)
        new_rows = _reshaped(c, nodes)
        if name == "last":
            new_rows[0] = random_rows(c.rng, 1, lengths=[0])[0]
        new_nws = c.rng.uniform(-1.0, 1.0, len(nodes))
        want = c.model(nodes, new_rows, new_nws)
        snap = c.snapshot()
        assert c.call(patch, pack_of(nodes, new_rows, new_nws), out=True) == 0, name
        nnz = int(want[0][-1])
        assert same(c.out[0], want[0]), name
        assert same(c.out[1][:nnz], want[1]) and same(c.out[2][:nnz], want[2]), name
        assert (c.out[1][nnz:] == -7).all() and (c.out[2][nnz:] == -7.0).all(), (name, "written past the new matrix")
        assert same(c.nws, want[3]), name
        assert all(same(x, y) for x, y in zip((c.indptr, c.indices, c.data), snap[:3])), (name, "the old matrix is an input")
        if len(nodes) and name != "m0":
            changed = [len(new_rows[i][0]) != len(c.rows[int(p)][0]) for i, p in enumerate(nodes)]
            if any(changed):   # in place, such a pack is refused
                assert c.call(patch, pack_of(nodes, new_rows, new_nws)) == EINVAL and same(c.indices, snap[1]) and same(c.data, snap[2]), name


def test_rows_appear_and_vanish(patch):
    """an empty matrix gets rows, and a full one loses all of them"""
    c = Case(65, 7)
    c.rows = [(np.zeros(0, np.int32), np.zeros(0))] * 65
    c.indptr, c.indices, c.data = csr_of(c.rows)
    nodes = c.rng.permutation(65)[:40]
    new_rows = random_rows(c.rng, 40, lengths=c.rng.integers(1, MAX_ROW + 1, 40))
    want = c.model(nodes, new_rows, np.ones(40))
    assert c.call(patch, pack_of(nodes, new_rows, np.ones(40)), out=True) == 0
    assert same(c.out[0], want[0]) and same(c.out[1][: want[0][-1]], want[1]) and same(c.out[2][: want[0][-1]], want[2])
    c = Case(65, 8)
    nodes = c.rng.permutation(65)
    empty = random_rows(c.rng, 65, lengths=[0] * 65)
    assert c.call(patch, pack_of(nodes, empty, np.zeros(65)), out=True) == 0
    assert (c.out[0] == 0).all() and (c.out[1] == -7).all() and same(c.nws, np.zeros(65))


REJECTED = ("null_indptr", "null_indices", "null_data", "null_nws", "null_nodes", "null_counts", "null_off", "null_pack_indices",
            "null_pack_data", "null_pack_nws", "only_out_indptr", "no_out_data", "node_P", "node_negative", "duplicate", "off_gap",
            "off_start", "off_short", "negative_count", "negative_P", "negative_m", "in_place_other_count")


# (a count that is not the row's length is what out_* is for: refused in place only)
@pytest.mark.parametrize("what,out", [(w, o) for w in REJECTED for o in (False, True) if not (o and w == "in_place_other_count")])
def test_rejected_inputs_change_nothing(patch, what, out):
    P = 65
    c = Case(P, 300)
    nodes = c.rng.permutation(P)[:20]
    lengths = [len(c.rows[int(p)][0]) for p in nodes]
    new_rows = random_rows(c.rng, 20, lengths=lengths)
    pk = pack_of(nodes, new_rows, np.ones(20))
    arrays, kw = {}, {}
    null = {"null_indptr": "indptr", "null_indices": "indices", "null_data": "data", "null_nws": "nws", "null_nodes": "nodes",
            "null_counts": "counts", "null_off": "off", "null_pack_indices": "pi", "null_pack_data": "pd", "null_pack_nws": "pn"}
    if what in null:
        arrays[null[what]] = None
    elif what == "only_out_indptr":
        if out:
            arrays["out1"] = arrays["out2"] = None
        else:
            arrays["out0"] = np.zeros(P + 1, np.int32)
    elif what == "no_out_data":
        if out:
            arrays["out2"] = None
        else:
            arrays["out0"], arrays["out1"] = np.zeros(P + 1, np.int32), np.zeros(len(c.indices) + 8, np.int32)
    elif what == "node_P":
        pk["nodes"][7] = P
    elif what == "node_negative":
        pk["nodes"][0] = -1
    elif what == "duplicate":
        pk["nodes"][19] = pk["nodes"][3]
    elif what == "off_gap":
        pk["off"][5:] += 1
    elif what == "off_start":
        pk["off"] += 1
    elif what == "off_short":
        pk["off"][-1] -= 1
    elif what == "negative_count":
        pk["counts"][4] = -1
        pk["off"][5:] -= pk["off"][5] - pk["off"][4] + 1
    elif what == "negative_P":
        kw["P"] = -1
    elif what == "negative_m":
        kw["m"] = -1
    elif what == "in_place_other_count":
        k = int(np.argmax(np.array(lengths) > 0))
        pk["counts"][k] -= 1
        pk["off"][k + 1:] -= 1
    snap = c.snapshot()
    packs = {k: v.copy() for k, v in pk.items()}
    assert c.call(patch, pk, out=out, arrays=arrays, **kw) == EINVAL
    assert c.untouched(snap) and all(same(pk[k], packs[k]) for k in pk)
    if out:
        assert all(o is None or (o == -7).all() for o in (c.out[0], c.out[1], c.out[2])), "an out array was written before the refusal"
