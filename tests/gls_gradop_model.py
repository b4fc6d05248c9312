"""A numpy model of the kept corner-gradient operator: its layout and its two products as the stated sums.

Node p with ne = esup_ptr[p + 1] - esup_ptr[p] cells cells[0 .. ne) owns G_p [3 ne x ne], stored by columns:

    gop[gop_ptr[p] + j * 3 ne + i],  i = 3 * (cell slot) + component,  gop_ptr = the exclusive sum of 3 ne^2

Column j is the 3 ne corner gradients of p for the cell field that is 1 on cells[j] and 0 elsewhere.  A field that is 1 on a set of
cells no two of which share a node is that indicator at every node at once, so a greedy colouring of the cells turns the columns of
every node into a few global fields (`colour_cells`, `indicator_fields`, `gop_from_fields`).

    apply:            grad[t][pos][c] = sum_j gop[base_p + j * 3 ne + 3 i + c] * u[t][cells[j]],  pos = esup_ptr[p] + i, j ascending from 0.0
    apply_transpose:  ubar[t][e] = sum_{(p, j): cells_p[j] = e} sum_i gop[base_p + j * 3 ne + i] * gbar[t][3 esup_ptr[p] + i],
                      first i ascending within a column, from 0.0, then the cell's columns in ascending node id, from 0.0

Each product is rounded, then added (no fused multiply-add).  In dtype = numpy.float64 the functions restate the device's arithmetic
operation for operation; in numpy.longdouble they are the yardstick of the summation bound

    |computed - exact| <= (n_terms + 2) u sum |terms|,   u = 2^-53

the standard bound of recursive summation in any order: a sum of n products has n - 1 additions and one rounding per product, so a
factor (1 + u)^n at most on every term -- n u to first order; + 2 covers the higher orders (n u < 0.01 here) and the yardstick's own
80-bit rounding.  n_terms is ne for an entry of the apply and the number of (p, j, i) triples of the cell for the transpose.

Not a test module (no test_ prefix).  Plain numpy."""
import numpy as np

U64 = 2.0 ** -53


def gop_ptr(esup_ptr):
    ne = np.diff(np.asarray(esup_ptr).astype(np.int64))
    return np.concatenate(([0], np.cumsum(3 * ne * ne))).astype(np.int64)


def colour_cells(esup_ptr, esup, n_elems):
    """colour [E] (int64), greedy in cell order: no two cells of a colour share a node"""
    esup_ptr, esup = np.asarray(esup_ptr).astype(np.int64), np.asarray(esup).astype(np.int64)
    P = len(esup_ptr) - 1
    cell_nodes = [[] for _ in range(int(n_elems))]
    for p in range(P):
        for e in esup[esup_ptr[p]:esup_ptr[p + 1]]:
            cell_nodes[e].append(p)
    colour = np.full(int(n_elems), -1, dtype=np.int64)
    for e in range(int(n_elems)):
        used = set()
        for p in cell_nodes[e]:
            used.update(colour[esup[esup_ptr[p]:esup_ptr[p + 1]]].tolist())
        c = 0
        while c in used:
            c += 1
        colour[e] = c
    return colour


def indicator_fields(colour):
    n = int(colour.max()) + 1 if len(colour) else 0
    return (colour[None, :] == np.arange(n)[:, None]).astype(np.float64)


def gop_from_fields(esup_ptr, esup, colour, grad):
    """grad [n_colours][nnz_esup][3] of the indicator fields -> gop: column j of node p is the node's slice of the field of colour[cells[j]]"""
    esup_ptr, esup = np.asarray(esup_ptr).astype(np.int64), np.asarray(esup).astype(np.int64)
    ptr = gop_ptr(esup_ptr)
    gop = np.empty(int(ptr[-1]), dtype=np.asarray(grad).dtype)
    for p in range(len(esup_ptr) - 1):
        eb, ee = esup_ptr[p], esup_ptr[p + 1]
        ne = ee - eb
        block = np.asarray(grad)[colour[esup[eb:ee]], eb:ee].reshape(ne, 3 * ne)       # row j = column j of G_p
        gop[ptr[p]:ptr[p + 1]] = block.reshape(-1)
    return gop


def _blocks(esup_ptr, esup, ptr, gop):
    for p in range(len(esup_ptr) - 1):
        eb, ee = int(esup_ptr[p]), int(esup_ptr[p + 1])
        ne = ee - eb
        if ne:
            yield eb, ne, esup[eb:ee], gop[ptr[p]:ptr[p + 1]].reshape(ne, 3 * ne)


def apply(esup_ptr, esup, gop, u, dtype=np.float64, magnitude=False):
    """u [k][E] -> grad [k][nnz_esup][3] in dtype, the stated sum; magnitude: sum_j |term| instead (the scale of the bound)"""
    esup_ptr, esup = np.asarray(esup_ptr).astype(np.int64), np.asarray(esup).astype(np.int64)
    ptr = gop_ptr(esup_ptr)
    G, U = np.asarray(gop).astype(dtype), np.atleast_2d(u).astype(dtype)
    out = np.zeros((U.shape[0], 3 * int(esup_ptr[-1])), dtype=dtype)
    for eb, ne, cells, B in _blocks(esup_ptr, esup, ptr, G):
        acc = np.zeros((U.shape[0], 3 * ne), dtype=dtype)
        for j in range(ne):
            term = B[j][None, :] * U[:, cells[j]][:, None]
            acc = acc + (np.abs(term) if magnitude else term)
        out[:, 3 * eb:3 * (eb + ne)] = acc
    return out.reshape(U.shape[0], -1, 3)


def apply_transpose(esup_ptr, esup, gop, gbar, n_elems, dtype=np.float64, magnitude=False):
    """gbar [k][nnz_esup][3] -> ubar [k][E] in dtype, the stated sums: a column's product i ascending, then the cell's columns in ascending
    node id (a node holds a cell once, so adding node after node is that order)"""
    esup_ptr, esup = np.asarray(esup_ptr).astype(np.int64), np.asarray(esup).astype(np.int64)
    ptr = gop_ptr(esup_ptr)
    G = np.asarray(gop).astype(dtype)
    V = np.asarray(gbar).astype(dtype)
    V = V.reshape(-1, 3 * int(esup_ptr[-1])) if V.ndim == 3 else V.reshape(1, -1)
    out = np.zeros((V.shape[0], int(n_elems)), dtype=dtype)
    for eb, ne, cells, B in _blocks(esup_ptr, esup, ptr, G):
        dots = np.zeros((V.shape[0], ne), dtype=dtype)
        for i in range(3 * ne):
            term = B[:, i][None, :] * V[:, 3 * eb + i][:, None]
            dots = dots + (np.abs(term) if magnitude else term)
        out[:, cells] = out[:, cells] + dots
    return out


def apply_terms(esup_ptr):
    """n_terms of every entry of the apply [nnz_esup][3]: ne of the node that owns the row"""
    ne = np.diff(np.asarray(esup_ptr).astype(np.int64))
    return np.repeat(np.repeat(ne, ne), 3).reshape(-1, 3)


def transpose_terms(esup_ptr, esup, n_elems):
    """n_terms of every entry of the transposed apply [E]: the sum of 3 ne over the nodes of the cell"""
    ne = np.diff(np.asarray(esup_ptr).astype(np.int64))
    out = np.zeros(int(n_elems), dtype=np.int64)
    np.add.at(out, np.asarray(esup).astype(np.int64), np.repeat(3 * ne, ne))
    return out


def dense(esup_ptr, esup, gop, n_elems):
    """the operator as a dense (3 nnz_esup, E) array, entry by entry from the layout"""
    esup_ptr, esup = np.asarray(esup_ptr).astype(np.int64), np.asarray(esup).astype(np.int64)
    ptr = gop_ptr(esup_ptr)
    A = np.zeros((3 * int(esup_ptr[-1]), int(n_elems)), dtype=np.asarray(gop).dtype)
    for p in range(len(esup_ptr) - 1):
        eb, ne = int(esup_ptr[p]), int(esup_ptr[p + 1] - esup_ptr[p])
        for j in range(ne):
            for i in range(3 * ne):
                A[3 * eb + i, esup[eb + j]] = gop[ptr[p] + j * 3 * ne + i]
    return A
