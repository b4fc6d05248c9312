"""A numpy model of the GLS Jacobian in the node coordinates assembled as a block-CSR matrix.

The kept Jacobian is a set of records: cell [nnz_esup][3] = dF_p / d centroid_e, face [nnz_fsup][6] = (dF_p / d face
centre_f, dF_p / d unit normal_f), own [P][3] = dF_p / d x_p.  The matrix has block (p, q) = dF_p / d x_q [3] for q in

    C(p) = {p} + the vertices of the cells in esup[p] + the points of the faces in fsup[p],   ascending in q, each once,

and block (p, q) is summed in this order, which the device follows:
  1. own[p] if q == p;
  2. for the cells e of esup[p] in row order that contain q:  + cell[pos(p, e)] / n_e;
  3. for the faces f of fsup[p] in row order with q = point k of f:  + slot k of the face chain of csrc/gls_shape_chain.hpp applied to
     the one record face[pos(p, f)] = (Fb, Nb):  share = Fb / npofa;  nbar = (Nb - (Nb . N) N) / |n| with n = v1 x v2, v1 = x_0 - x_1,
     v2 = x_2 - x_1 and N the resident normal;  v1bar = v2 x nbar, v2bar = nbar x v1;  slot 0 = share + v1bar,
     slot 1 = share - (v1bar + v2bar), slot 2 = share + v2bar, slot 3 (a quadrilateral's fourth point) = share.

`pattern` needs the connectivity only; `assemble` takes the records as input, so it needs no GLS solve -- the chain is linear in them.
The scale of a block is the sum of the absolute contributions carried through the same chain with every sign made a plus, the way
tests/gls_shape_model.py builds its own (SM._cross_abs).

Not a test module (no test_ prefix).  Plain numpy."""
import numpy as np

from gls_exact import LD
from gls_shape_model import _cross_abs, cell_points, face_points


def _rows(grid):
    """(esup_ptr, esup, fsup_ptr, fsup) as int64"""
    return tuple(np.asarray(getattr(grid, k)).astype(np.int64) for k in ("esup_ptr", "esup", "fsup_ptr", "fsup"))


def candidates(grid, inpoel, inpofa):
    """per row the candidate list before deduplication: the vertices of its cells, the points of its faces, the node itself"""
    eptr, esup, fptr, fsup = _rows(grid)
    cpts, fpts = cell_points(inpoel), face_points(inpofa)
    out = []
    for p in range(len(eptr) - 1):
        c = [q for e in esup[eptr[p]:eptr[p + 1]] for q in cpts[e]] + [q for f in fsup[fptr[p]:fptr[p + 1]] for q in fpts[f]] + [p]
        out.append(np.asarray(c, dtype=np.int64))
    return out


def pattern(grid, inpoel, inpofa):
    """(block_ptr [P + 1] int64, block_col [n_blocks] int32): the columns of every row ascending, each once"""
    cols = [np.unique(c) for c in candidates(grid, inpoel, inpofa)]
    block_ptr = np.zeros(len(cols) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cols], out=block_ptr[1:])
    return block_ptr, (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)


def assemble(cell, face, own, grid, coords, normals, inpoel, inpofa, dtype=LD):
    """(values [n_blocks][3], scale [n_blocks][3]) in dtype from the records cell [nnz_esup][3], face [nnz_fsup][6], own [P][3], the
    coordinates [P][3] and the resident normals [F][3]; the blocks in the order of pattern()"""
    eptr, esup, fptr, fsup = _rows(grid)
    block_ptr, block_col = pattern(grid, inpoel, inpofa)
    cpts, fpts = cell_points(inpoel), face_points(inpofa)
    X = np.asarray(coords, dtype=np.float64).reshape(-1, 3).astype(dtype)
    Nres = np.asarray(normals, dtype=np.float64).reshape(-1, 3).astype(dtype)
    cell, face, own = (np.asarray(a, dtype=dtype) for a in (cell, face, own))
    values, scale = np.zeros((len(block_col), 3), dtype=dtype), np.zeros((len(block_col), 3), dtype=dtype)
    for p in range(len(eptr) - 1):
        b0 = block_ptr[p]
        at = {int(q): b0 + i for i, q in enumerate(block_col[b0:block_ptr[p + 1]])}
        values[at[p]] = own[p]
        scale[at[p]] = np.abs(own[p])
        for pos in range(eptr[p], eptr[p + 1]):
            v = cpts[esup[pos]]
            for q in v:
                values[at[int(q)]] += cell[pos] / dtype(len(v))
                scale[at[int(q)]] += np.abs(cell[pos]) / dtype(len(v))
        for pos in range(fptr[p], fptr[p + 1]):
            f = fsup[pos]
            v = fpts[f]
            if len(v) < 3:
                continue
            Fb, Nb, N = face[pos, :3], face[pos, 3:], Nres[f]
            v1, v2 = X[v[0]] - X[v[1]], X[v[2]] - X[v[1]]
            n = np.cross(v1, v2)
            nn = np.sqrt(n @ n)
            nbar, nabs = (Nb - (Nb @ N) * N) / nn, (np.abs(Nb) + (np.abs(Nb) @ np.abs(N)) * np.abs(N)) / nn
            v1b, v2b = np.cross(v2, nbar), np.cross(nbar, v1)
            v1a, v2a = _cross_abs(v2, nabs), _cross_abs(nabs, v1)
            share, sabs = Fb / dtype(len(v)), np.abs(Fb) / dtype(len(v))
            slots = [(share + v1b, sabs + v1a), (share - (v1b + v2b), sabs + (v1a + v2a)), (share + v2b, sabs + v2a), (share, sabs)]
            for k, q in enumerate(v):
                values[at[int(q)]] += slots[k][0]
                scale[at[int(q)]] += slots[k][1]
    return values, scale
