"""The corner-gradient operator of the GLS reconstruction as an object the caller keeps: GlsGradientOperator over the C
object nin_gls_gradop (device pointers, asynchronous) and GradientOperator, the scipy LinearOperator Interpolator.gradient_operator
returns over it (numpy, host-synchronous).  The handle, the stamp and the lifetime are jacobian._KeptJacobian's.
ninpol_amd.interpolator re-exports both names."""
import ctypes

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import _lib
from ._lib import _ptr, _vp
from .jacobian import DTYPE_F, _KeptJacobian


class GlsGradientOperator(_KeptJacobian):
    """The linear map G from a cell field u [n_elems] to the corner gradients g [nnz_esup][3] of DevicePlan.launch_corner_gradients,
    factorised ONCE and resident on the device (nin_gls_gradop).  G depends on the node coordinates, the permeability
    and the Neumann flags alone and is block diagonal over the nodes: node p with ne cells owns the 3 ne x ne block at
    `gop[gop_ptr[p] + j * 3 ne + i]`, column j = the corner gradients of p for the indicator of its cell j, i = 3 * (cell slot) +
    component -- bit for bit what launch_corner_gradients writes for such a field.  `launch_apply` is G . u, `launch_apply_transpose`
    G^T . v, each a streaming pass over the buffer per four fields, asynchronous on the caller's stream, bitwise reproducible.  Unlike
    the kept Jacobians the operator IS the state of the grid: after any update of the permeability, the points or the flags both
    launches raise (NinpolError, a RuntimeError, NIN_ESTATE) and write nothing until `factorize()` (`stale` says so beforehand).  Made by
    DevicePlan.gradient_operator(); its buffers (`nbytes`: 24 sum ne^2 bytes, 15.4 GB at 216^3 hexahedra) are its own."""

    _C = "nin_gls_gradop"

    def __init__(self, grid, plan=None):
        self._create(grid, plan)

    def factorize(self, stream=0):
        """Factorise every node again at what is resident now (nin_gls_gradop_factorize): one launch of the adjoint kernel's gradient
        mode with the unit columns as its fields, every entry of the buffer written.  Asynchronous on `stream`."""
        if self.plan is not None:
            self.plan.ensure_current()
        _lib.check(self._c("factorize")(self._handle(), ctypes.c_void_p(stream)))

    def launch_apply(self, u_ptr, grad_ptr, n=1, flux_ptr=0, node_gradient_ptr=0, stream=0):
        """G . u for n fields (nin_gls_gradop_apply): u [n][n_elems] -> grad [n][nnz_esup][3], every entry written, exact zeros where
        the row is zero; flux [n][nnz_esup][3] = -K_e grad and node_gradient [n][n_points][3] (0: not wanted) as
        launch_corner_gradients derives them.  Per entry the sum over the node's cells in row order from 0.0."""
        _lib.check(self._c("apply")(self._handle(), int(n), _vp(u_ptr), _vp(grad_ptr), _vp(flux_ptr), _vp(node_gradient_ptr),
                                    ctypes.c_void_p(stream)))

    def launch_apply_transpose(self, gbar_ptr, ubar_ptr, n=1, stream=0):
        """G^T . gbar for n fields (nin_gls_gradop_apply_transpose): gbar [n][nnz_esup][3] -> ubar [n][n_elems].  Asynchronous on
        `stream` (the first call on a grid without the transpose index builds it and synchronises); no atomics."""
        _lib.check(self._c("apply_transpose")(self._handle(), int(n), _vp(gbar_ptr), _vp(ubar_ptr), ctypes.c_void_p(stream)))

    def _records(self):
        p, g, n, s = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._c("records")(self._handle(), ctypes.byref(p), ctypes.byref(g), ctypes.byref(n), ctypes.byref(s)))
        return int(p.value or 0), int(g.value or 0), int(n.value), int(s.value)

    @property
    def record_ptrs(self):
        """the device addresses of (gop_ptr int64 [n_points + 1], gop float64 [n_values]), read-only"""
        return self._records()[:2]

    @property
    def n_values(self):
        return self._records()[2]

    @property
    def nbytes(self):
        """the operator (8 n_values) plus what the object holds beside it: gop_ptr, the node of every esup position, and the per-column
        products of the transposed apply once a call made them"""
        r = self._records()
        return 8 * r[2] + r[3]

    @property
    def stale(self):
        """True before the first factorize() and after any update of the permeability, the points or the flags: the products raise"""
        return not self.is_current()

    def fetch(self):
        """(gop_ptr (n_points + 1,) int64, gop (n_values,) float64) on the host (waits for the device)"""
        h = self._handle()
        gop_ptr = np.empty(int(self.grid.n_points) + 1, dtype=np.int64)
        gop = np.empty(self.n_values, dtype=DTYPE_F)
        _lib.check(self._c("fetch_host")(h, _ptr(gop_ptr), _ptr(gop)))
        return gop_ptr, gop


def block_csr(esup_ptr, esup, gop_ptr, gop, n_elems):
    """The csr_matrix (3 nnz_esup, n_elems) of a fetched operator: row 3 pos + c of node p's row holds the ne entries
    gop[gop_ptr[p] + j * 3 ne + i] at the columns esup[esup_ptr[p] + j], j ascending (esup is ascending within a row, so the indices are
    sorted); explicit zeros kept, int64 indices."""
    esup_ptr, esup = np.asarray(esup_ptr).astype(np.int64), np.asarray(esup).astype(np.int64)
    gop_ptr = np.asarray(gop_ptr).astype(np.int64)
    ne = np.diff(esup_ptr)
    nnz = int(esup_ptr[-1])
    row_ne = np.repeat(np.repeat(ne, ne), 3)                         # [3 nnz]: ne of the node that owns the row
    indptr = np.concatenate(([0], np.cumsum(row_ne)))
    node = np.repeat(np.arange(len(ne), dtype=np.int64), ne)        # [nnz]
    row_node = np.repeat(node, 3)                                    # [3 nnz]
    i = np.arange(3 * nnz, dtype=np.int64) - 3 * esup_ptr[row_node]  # the row's index within its block
    entry_row = np.repeat(np.arange(3 * nnz, dtype=np.int64), row_ne)
    j = np.arange(int(indptr[-1]), dtype=np.int64) - indptr[entry_row]
    p = row_node[entry_row]
    data = np.asarray(gop)[gop_ptr[p] + j * (3 * ne[p]) + i[entry_row]]
    indices = esup[esup_ptr[p] + j]
    A = sp.csr_matrix((data, indices, indptr), shape=(3 * nnz, int(n_elems)))
    A.indices, A.indptr = indices, indptr       # (the constructor narrows index arrays that fit int32)
    A.has_sorted_indices = True
    return A


class GradientOperator(spla.LinearOperator):
    """Interpolator.gradient_operator's result: the (3 nnz_esup, n_elems) map from a cell field to the corner gradients of
    `corner_gradients(variable)` (row 3 pos + c: component c of the gradient at esup position pos), as a scipy LinearOperator over a
    GlsGradientOperator: numpy in and out, host-synchronous, one launch per matvec / rmatvec and one per batched matmat / rmatmat."""

    def __init__(self, op, interp=None, variable=None):
        g = op.grid
        self.operator = op
        self._interp, self._variable = interp, variable
        self._rows, self._E = 3 * int(g.nnz_esup), int(g.n_elems)
        super().__init__(dtype=np.dtype(DTYPE_F), shape=(self._rows, self._E))

    def _apply(self, u):        # u (k, E) -> (k, 3 nnz)
        u = np.ascontiguousarray(u, dtype=DTYPE_F)
        out = np.empty((len(u), self._rows), dtype=DTYPE_F)
        _lib.check(self.operator._c("apply_host")(self.operator._handle(), len(u), _ptr(u), _ptr(out), None, None))
        return out

    def _apply_transpose(self, v):      # v (k, 3 nnz) -> (k, E)
        v = np.ascontiguousarray(v, dtype=DTYPE_F)
        out = np.empty((len(v), self._E), dtype=DTYPE_F)
        _lib.check(self.operator._c("apply_transpose_host")(self.operator._handle(), len(v), _ptr(v), _ptr(out)))
        return out

    def _matvec(self, x):
        return self._apply(np.asarray(x).reshape(1, -1))[0]

    def _rmatvec(self, x):
        return self._apply_transpose(np.asarray(x).reshape(1, -1))[0]

    def _matmat(self, X):
        return self._apply(np.asarray(X).T).T

    def _rmatmat(self, X):
        return self._apply_transpose(np.asarray(X).T).T

    def update(self):
        """Factorise again at the grid's state as it is now -- after update_permeability(), update_points() or
        update_neumann_flags(), whole or local, the products raise until this call.  Every node is factorised (following the dirty
        set is not provided).  Host-synchronous."""
        I = self._interp
        if I is not None:
            if I.grid is not self.operator.grid:
                raise ValueError("the Interpolator has loaded another mesh since this operator was made")
            I._check_call(variable=self._variable)
            I._gls_tables_to_device(self._variable)
        _lib.check(self.operator._c("factorize_host")(self.operator._handle()))

    def to_scipy(self):
        """The explicit csr_matrix (3 nnz_esup, n_elems) from the fetched buffer and the connectivity, explicit zeros kept (the rows
        the forward gives as zero keep their pattern): the gradient stencil dg/du an implicit flux scheme assembles from."""
        g = self.operator.grid
        gop_ptr, gop = self.operator.fetch()
        return block_csr(g.esup_ptr, g.esup, gop_ptr, gop, g.n_elems)

    def release(self):
        self.operator.release()
