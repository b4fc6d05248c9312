"""The GLS Jacobians as objects the caller keeps: in the permeability GlsJacobian and GlsReducedJacobian over
the C objects nin_gls_jacobian / nin_gls_rjacobian, in the node coordinates GlsShapeJacobian over nin_gls_xjacobian
(device pointers, asynchronous), and the scipy LinearOperators Interpolator.permeability_jacobian and Interpolator.points_jacobian
return over them (numpy, host-synchronous).  What they share is written once: _KeptJacobian -- the handle, the stamp, the lifetime
-- and _JacobianOperator -- the two host products.  ninpol_amd.interpolator re-exports every public name."""
import ctypes

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import _lib
from ._lib import _ptr, _vp

DTYPE_F = np.float64


class _KeptJacobian:
    """What GlsJacobian, GlsReducedJacobian and GlsShapeJacobian share: the C object `_C`_create made, its stamp, and giving it back."""

    _C = None       # the prefix of the C entry points: "nin_gls_jacobian", "nin_gls_rjacobian" or "nin_gls_xjacobian"

    def _create(self, grid, plan, *args):
        self.grid, self.plan = grid, plan
        self._h = None
        h = ctypes.c_void_p()
        _lib.check(self._c("create")(grid._h, *args, ctypes.byref(h)))
        self._h = h

    def _c(self, name):
        return getattr(_lib.load(), f"{self._C}_{name}")

    def _handle(self):
        if self._h is None:
            raise ValueError(f"this {type(self).__name__} was released")
        return self._h

    def _linearize(self, *args):
        if self.plan is not None:
            self.plan.ensure_current()
        _lib.check(self._c("linearize")(self._handle(), *args))

    _seeded = False     # the object keeps the cotangent buffer of its dirty relinearisations (8 bytes per entry of esup)

    def _linearize_dirty(self, *args, clear=True):
        """What the three relinearize_dirty share (nin_gls_*jacobian_linearize_dirty): the arguments of `_linearize`,
        then clear; returns the number of rows recomputed."""
        if self.plan is not None:
            self.plan.ensure_current()
        n = ctypes.c_int64(0)
        _lib.check(self._c("linearize_dirty")(self._handle(), *args, int(bool(clear)), ctypes.byref(n)))
        self._count_seed()
        return int(n.value)

    def _count_seed(self):
        """the first dirty relinearisation that went through made the object's cotangent buffer: `nbytes` counts it from here on (the
        shape Jacobian's nbytes asks the C object, which counts it itself)"""
        if not self._seeded:
            self._seeded = True
            if "nbytes" in self.__dict__:
                self.nbytes += 8 * int(self.grid.nnz_esup)

    @property
    def stamp(self):
        """the grid's (field_updates, geometry_updates, flag_updates) at the last linearisation"""
        s = np.zeros(3, dtype=np.int64)
        _lib.check(self._c("stamp")(self._handle(), _ptr(s)))
        return tuple(int(x) for x in s)

    def is_current(self):
        """Is the grid's resident permeability, geometry and flag set still the one this object was linearised at?  (Device-side updates
        count; launch_jvp / launch_vjp answer for the linearisation point either way.)"""
        g = self.grid
        return self.stamp == (g.field_updates, g.geometry_updates, g.flag_updates)

    def release(self):
        """Give the device buffers back (waits for the device); the object is unusable afterwards."""
        if self._h is not None:
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:       # interpreter shutdown
            pass


class GlsJacobian(_KeptJacobian):
    """The sparse Jacobian of `F(K) = W(K) u + neumann_ws(K) * b` with respect to the permeability at ONE linearisation point, resident
    on the device (nin_gls_jacobian): `contrib_ptr` [nnz_esup][10] holds, per (node, cell) pair in esup position, dF_p / d
    perm_e[0..9) and dF_p / d diff_mag_e; `fold_ptr` [n_elems] the derivative of the table's diff_mag = (1 - 3 / tr K)^2 there.
    `launch_jvp` is J . dK, `launch_vjp` is J^T . v, each one streaming pass over the buffer per four directions, asynchronous on the
    caller's stream, bitwise reproducible.  Later updates of the permeability, the points or the flags do not change the answers: the
    object is the Jacobian where it was linearised (`stamp`; `is_current()` says whether the grid is still there).  `relinearize`
    moves it.  Made by DevicePlan.linearize(); its device buffers (`nbytes`) are its own: a launch_weights_backward in between does not
    disturb it."""

    _C = "nin_gls_jacobian"

    def __init__(self, grid, plan=None):
        self._create(grid, plan)
        self.nbytes = 80 * int(grid.nnz_esup) + 8 * int(grid.n_elems)       # (+ 8 nnz_esup from the first relinearize_dirty on: its cotangent)

    def relinearize(self, u_ptr, neumann_values_ptr=0, stream=0):
        """Linearise again, at what is resident now, for u [n_elems] (and b [n_points], 0: none), device pointers: what a fresh
        DevicePlan.linearize would hold, bit for bit, in the buffers this object already owns."""
        self._linearize(_vp(u_ptr), _vp(neumann_values_ptr), ctypes.c_void_p(stream))

    def launch_jvp(self, dperm_ptr, out_ptr, n=1, ddm_ptr=0, stream=0):
        """J . dK for n directions (nin_gls_jacobian_apply): dperm [n][n_elems][9] -> out [n][n_points], every entry written.  ddm
        [n][n_elems]: the table's diff_mag as an independent input with its own direction; 0: its chain folded, at the permeability of
        the linearisation.  Asynchronous on `stream`."""
        _lib.check(_lib.load().nin_gls_jacobian_apply(self._handle(), int(n), _vp(dperm_ptr), _vp(ddm_ptr), _vp(out_ptr), ctypes.c_void_p(stream)))

    def launch_vjp(self, v_ptr, grad_perm_ptr, n=1, grad_dm_ptr=0, stream=0):
        """J^T . v for n node fields (nin_gls_jacobian_apply_transpose): v [n][n_points] -> grad_perm [n][n_elems][9] (and grad_dm
        [n][n_elems]; 0: folded into the diagonal of grad_perm).  v = 1 is launch_weights_backward(grad_csr = u[esup], grad_neumann_ws =
        b) at the linearisation point, bit for bit.  Asynchronous on `stream` (the first call on a grid without the transpose index
        builds it and synchronises)."""
        _lib.check(_lib.load().nin_gls_jacobian_apply_transpose(self._handle(), int(n), _vp(v_ptr), _vp(grad_perm_ptr), _vp(grad_dm_ptr),
                                                                ctypes.c_void_p(stream)))

    def _buffers(self):
        c, f = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.load().nin_gls_jacobian_contrib(self._handle(), ctypes.byref(c), ctypes.byref(f)))
        return int(c.value or 0), int(f.value or 0)

    @property
    def contrib_ptr(self):
        return self._buffers()[0]

    @property
    def fold_ptr(self):
        return self._buffers()[1]

    def fetch(self):
        """(contrib (nnz_esup, 10), fold (n_elems,)) on the host (waits for the device)"""
        g = self.grid
        contrib, fold = np.empty((int(g.nnz_esup), 10), dtype=DTYPE_F), np.empty(int(g.n_elems), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_jacobian_fetch_host(self._handle(), _ptr(contrib), _ptr(fold)))
        return contrib, fold


class GlsDirtyJacobian(GlsJacobian):
    """A GlsJacobian that follows local updates: what DevicePlan.linearize() returns.  Everything of GlsJacobian, and
    `relinearize_dirty`, which recomputes only the rows of the grid's dirty nodes.  (A class of its own because the public names of
    GlsJacobian are a pinned, closed set.)"""

    def relinearize_dirty(self, u_ptr, neumann_values_ptr=0, stream=0, clear=True):
        """relinearize for the rows of the grid's dirty nodes only (nin_gls_jacobian_linearize_dirty) -- after
        Interpolator.update_permeability(cells=), update_points(nodes=), update_neumann_flags(nodes=) or Grid.mark_dirty() -- and return
        how many rows that were.  If the object was the Jacobian at the grid's state as of the last clear, and u (b) differs from
        the u (b) of that linearisation only in cells all of whose vertices are marked (only at marked nodes), the buffers hold
        afterwards what relinearize(u, b) would write now, bit for bit, `fold` included; no other row is touched.  One 32-byte
        read-back waits for `stream`; everything else is asynchronous on it.  clear=False keeps the set (another consumer follows:
        DevicePlan.launch_dirty, a HostMatrix, a second Jacobian -- one grid, one stream, the last with clear=True).  While every node
        is dirty (Grid.dirty_nodes == -1) this is relinearize() and returns n_points; with an empty set it launches no adjoint kernel
        and returns 0.  Either way `is_current()` is true afterwards.  Raises what launch_dirty raises if ids outside the mesh were
        scattered since the last dirty launch (nothing is launched, the set and the object are kept, the next call goes through), and
        NinpolError (NIN_ESTATE) on an object that was never linearised."""
        return self._linearize_dirty(_vp(u_ptr), _vp(neumann_values_ptr), ctypes.c_void_p(stream), clear=clear)


REDUCED_N_PARAMS = (1, 3, 6)


def _check_n_params(n_params, basis_ptr=1):
    if isinstance(n_params, bool) or not isinstance(n_params, (int, np.integer)) or int(n_params) not in REDUCED_N_PARAMS:
        raise ValueError(f"n_params must be one of {REDUCED_N_PARAMS}, not {n_params!r}")
    if not basis_ptr and int(n_params) != 1:
        raise ValueError(f"basis_ptr = 0 (the resident permeability as the basis) needs n_params = 1, not {n_params}")


def reduced_basis(basis, n_elems):
    """Interpolator.permeability_jacobian's `basis` as (M, B, per_cell): B a C-contiguous float64 array (n_elems, M, 9) (per_cell) or
    (M, 9) (shared by every cell), or None for "scale" (M = 1: the resident permeability itself)."""
    if isinstance(basis, str):
        if basis == "scale":
            return 1, None, False
        if basis == "diagonal":
            B = np.zeros((3, 3, 3), dtype=DTYPE_F)
            for d in range(3):
                B[d, d, d] = 1.0
            return 3, B.reshape(3, 9), False
        if basis == "symmetric":
            B = np.zeros((6, 3, 3), dtype=DTYPE_F)
            for m, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                B[m, i, j] = B[m, j, i] = 1.0
            return 6, B.reshape(6, 9), False
        raise ValueError(f"basis must be 'scale', 'diagonal', 'symmetric' or an ndarray, not '{basis}'")
    if not isinstance(basis, np.ndarray):
        raise ValueError(f"basis must be 'scale', 'diagonal', 'symmetric' or a float64 ndarray, not {type(basis).__name__}")
    if basis.dtype != DTYPE_F:
        raise ValueError(f"basis must be float64, not {basis.dtype} (no silent cast)")
    E = int(n_elems)
    shape = tuple(basis.shape)
    per_cell = len(shape) >= 3 and shape[0] == E and shape[2:] in ((9,), (3, 3))     # (the last axis tells (E, M, 9) from (M, 3, 3))
    shared = len(shape) >= 2 and shape[1:] in ((9,), (3, 3))
    M = shape[1] if per_cell else shape[0] if shared else None
    if M not in REDUCED_N_PARAMS:
        raise ValueError(f"basis must have shape ({E}, M, 9), ({E}, M, 3, 3), (M, 9) or (M, 3, 3) with M in {REDUCED_N_PARAMS}, not {shape}")
    return M, np.ascontiguousarray(basis).reshape((E, M, 9) if per_cell else (M, 9)), per_cell


class GlsReducedJacobian(_KeptJacobian):
    """The Jacobian of `F = W(K) u + neumann_ws(K) * b` in a reduced parametrisation of the permeability, perm_e = sum_m theta_(e,m)
    B_(e,m) with `n_params` = M = 1, 3 or 6 per cell, at ONE linearisation point, resident on the device (nin_gls_rjacobian, DESIGN.md
    4.14): `buffer_ptr` [nnz_esup][M] holds dF_p / d theta_(e,m) per (node, cell) pair in esup position, the diff_mag chain folded --
    `nbytes` = 8 M nnz_esup, where a GlsJacobian keeps 80 nnz_esup.  `launch_jvp` is J_theta . dtheta, `launch_vjp` J_theta^T . v, one
    streaming pass per four directions each, asynchronous, bitwise reproducible.  Later updates of the permeability, the points or the
    flags do not change the answers (`stamp`, `is_current()`); `relinearize` moves it, to another basis too.  Made by
    DevicePlan.linearize_reduced(); its device buffer is its own."""

    _C = "nin_gls_rjacobian"

    def __init__(self, grid, n_params=1, plan=None):
        _check_n_params(n_params)
        self.n_params = int(n_params)
        self._create(grid, plan, self.n_params)
        self.nbytes = 8 * self.n_params * int(grid.nnz_esup)                 # (+ 8 nnz_esup from the first relinearize_dirty on: its cotangent)

    def relinearize(self, u_ptr, basis_ptr=0, basis_per_cell=True, neumann_values_ptr=0, stream=0):
        """Linearise again, at what is resident now, for u [n_elems], the basis (see DevicePlan.linearize_reduced) and b [n_points]
        (0: none), device pointers: what a fresh linearize_reduced would hold, bit for bit, in the buffer this object already owns."""
        _check_n_params(self.n_params, basis_ptr)
        self._linearize(_vp(u_ptr), _vp(neumann_values_ptr), _vp(basis_ptr), int(bool(basis_per_cell)), ctypes.c_void_p(stream))

    def launch_jvp(self, dtheta_ptr, out_ptr, n=1, stream=0):
        """J_theta . dtheta for n directions (nin_gls_rjacobian_apply): dtheta [n][n_elems][M] -> out [n][n_points], every entry
        written.  Asynchronous on `stream`."""
        _lib.check(_lib.load().nin_gls_rjacobian_apply(self._handle(), int(n), _vp(dtheta_ptr), _vp(out_ptr), ctypes.c_void_p(stream)))

    def launch_vjp(self, v_ptr, grad_theta_ptr, n=1, stream=0):
        """J_theta^T . v for n node fields (nin_gls_rjacobian_apply_transpose): v [n][n_points] -> grad_theta [n][n_elems][M].
        Asynchronous on `stream` (the first call on a grid without the transpose index builds it and synchronises)."""
        _lib.check(_lib.load().nin_gls_rjacobian_apply_transpose(self._handle(), int(n), _vp(v_ptr), _vp(grad_theta_ptr), ctypes.c_void_p(stream)))

    @property
    def buffer_ptr(self):
        r, m = ctypes.c_void_p(), ctypes.c_int(0)
        _lib.check(_lib.load().nin_gls_rjacobian_buffer(self._handle(), ctypes.byref(r), ctypes.byref(m)))
        return int(r.value or 0)

    def fetch(self):
        """R (nnz_esup, M) on the host (waits for the device)"""
        R = np.empty((int(self.grid.nnz_esup), self.n_params), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_rjacobian_fetch_host(self._handle(), _ptr(R)))
        return R


class GlsDirtyReducedJacobian(GlsReducedJacobian):
    """A GlsReducedJacobian that follows local updates: what DevicePlan.linearize_reduced() returns.  Everything of
    GlsReducedJacobian, and `relinearize_dirty`."""

    def relinearize_dirty(self, u_ptr, basis_ptr=0, basis_per_cell=True, neumann_values_ptr=0, stream=0, clear=True):
        """relinearize for the rows of the grid's dirty nodes only (nin_gls_rjacobian_linearize_dirty): the contract
        of GlsDirtyJacobian.relinearize_dirty, with the basis of this call -- the one the object was linearised with, if the other rows
        are to stay its Jacobian -- read again for the listed rows only.  Returns how many rows were recomputed."""
        _check_n_params(self.n_params, basis_ptr)
        return self._linearize_dirty(_vp(u_ptr), _vp(neumann_values_ptr), _vp(basis_ptr), int(bool(basis_per_cell)), ctypes.c_void_p(stream),
                                     clear=clear)


XJAC_APPLY_CHUNK, XJAC_TRANSPOSE_CHUNK = 4, 2      # directions per pass over the records (csrc/launch.hpp: kXjacApplyChunk, kXjacTransposeChunk)


class GlsShapeJacobian(_KeptJacobian):
    """The Jacobian of `F(X) = W(X) u + neumann_ws(X) * b` with respect to the node coordinates at ONE linearisation point, resident on
    the device (nin_gls_xjacobian) and kept factored through the mesh geometry: per computed node the derivative of F_p
    in the centroids of its cells ([nnz_esup][3]), the centres and unit normals of its faces ([nnz_fsup][6]) and its own position
    ([n_points][3]) -- what one launch of the adjoint kernel's coordinate mode leaves for the cotangent u[esup], b.  `launch_jvp` is
    J . dX, `launch_vjp` is J^T . v, streaming passes over those records instead of a factorisation of every node, asynchronous on the
    caller's stream, bitwise reproducible.  The geometry chain between the records and the vertices reads the grid's RESIDENT
    coordinates and normals, so -- unlike a GlsJacobian -- the object answers only while they are those of the linearisation: after
    Interpolator.update_points() both launches raise (NinpolError, a RuntimeError, NIN_ESTATE) and write nothing until `relinearize`.
    Updates of the permeability or the flags do not change the answers and are not refused (`stamp`, `is_current()`).  Made by
    DevicePlan.linearize_points(); records and scratch (`nbytes`) are its own: a launch_weights_backward_points in between does not
    disturb it, and none of the grid's buffers of that call or of launch_weights_tangent_points is made.  One launch at a time per
    object (the launches share its scratch)."""

    _C = "nin_gls_xjacobian"

    def __init__(self, grid, plan=None):
        self._create(grid, plan)

    @property
    def record_bytes(self):
        g = self.grid
        return 24 * int(g.nnz_esup) + 48 * int(g._scalar("nnz_fsup")) + 24 * int(g.n_points)

    @property
    def nbytes(self):
        """records plus the scratch the launches have made so far: 24 bytes per cell and 48 per face for each of the up to four
        directions of a launch_jvp chunk, 24 per cell and 96 per face for each of the up to two fields of a launch_vjp chunk, and
        8 (n_points + 1) + 4 n_blocks for the pattern of the assembled matrix once pattern() or launch_assemble made it"""
        return self.record_bytes + self._buffers()[3]

    def relinearize(self, u_ptr, neumann_values_ptr=0, stream=0):
        """Linearise again, at what is resident now, for u [n_elems] (and b [n_points], 0: none), device pointers: what a fresh
        DevicePlan.linearize_points would hold, bit for bit, in the buffers this object already owns."""
        self._linearize(_vp(u_ptr), _vp(neumann_values_ptr), ctypes.c_void_p(stream))

    def relinearize_dirty(self, u_ptr, neumann_values_ptr=0, stream=0, clear=True):
        """relinearize for the records of the grid's dirty nodes only (nin_gls_xjacobian_linearize_dirty): the
        contract of GlsDirtyJacobian.relinearize_dirty.  After Interpolator.update_points(nodes=) the dirty nodes are exactly those whose
        cells or faces moved, so the records of every other node are still those of the resident geometry: launch_jvp, launch_vjp
        and launch_assemble, which raise after the update, answer again after this call -- for the new point, bit for bit what a
        fresh DevicePlan.linearize_points gives.  The pattern of the assembled matrix is kept.  Returns how many nodes were
        recomputed; `nbytes` counts the cotangent this path keeps (8 bytes per entry of esup) from the first call on."""
        return self._linearize_dirty(_vp(u_ptr), _vp(neumann_values_ptr), ctypes.c_void_p(stream), clear=clear)

    def launch_jvp(self, dX_ptr, out_ptr, n=1, stream=0):
        """J . dX for n directions (nin_gls_xjacobian_apply): dX [n][n_points][3] -> out [n][n_points], every entry written (exact
        zeros for the rows the forward gives as zero).  Asynchronous on `stream`."""
        _lib.check(_lib.load().nin_gls_xjacobian_apply(self._handle(), int(n), _vp(dX_ptr), _vp(out_ptr), ctypes.c_void_p(stream)))

    def launch_vjp(self, v_ptr, grad_points_ptr, n=1, stream=0):
        """J^T . v for n node fields (nin_gls_xjacobian_apply_transpose): v [n][n_points] -> grad_points [n][n_points][3].  v = 1 is
        launch_weights_backward_points(grad_csr = u[esup], grad_neumann_ws = b) at the linearisation point, bit for bit.  Asynchronous
        on `stream` (the first call on a grid without the transpose index builds it and synchronises)."""
        _lib.check(_lib.load().nin_gls_xjacobian_apply_transpose(self._handle(), int(n), _vp(v_ptr), _vp(grad_points_ptr), ctypes.c_void_p(stream)))

    def _buffers(self):
        c, f, o, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0)
        _lib.check(_lib.load().nin_gls_xjacobian_records(self._handle(), ctypes.byref(c), ctypes.byref(f), ctypes.byref(o), ctypes.byref(b)))
        return int(c.value or 0), int(f.value or 0), int(o.value or 0), int(b.value)

    @property
    def record_ptrs(self):
        """the device addresses of (cell records, face records, own records), read-only"""
        return self._buffers()[:3]

    def fetch(self):
        """(cell (nnz_esup, 3), face (nnz_fsup, 6), own (n_points, 3)) on the host (waits for the device)"""
        g = self.grid
        cell, face = np.empty((int(g.nnz_esup), 3), dtype=DTYPE_F), np.empty((int(g._scalar("nnz_fsup")), 6), dtype=DTYPE_F)
        own = np.empty((int(g.n_points), 3), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_xjacobian_fetch_host(self._handle(), _ptr(cell), _ptr(face), _ptr(own)))
        return cell, face, own

    # ---- the assembled matrix: block (p, q) = dF_p / d x_q [3] for q in C(p) = {p} + the vertices of the cells of
    #      esup[p] + the points of the faces of fsup[p], ascending ----
    def pattern(self, stream=0):
        """(n_blocks, block_ptr_ptr, block_col_ptr): the block-CSR pattern of the assembled Jacobian as the object's own device arrays
        (nin_gls_xjacobian_pattern) -- block_ptr [n_points + 1] int64, block_col [n_blocks] int32, ascending within a row -- valid
        until release().  Made by the first call (one wait for `stream`), from the connectivity alone: it needs no linearisation and
        survives relinearize and every update of the grid, the same addresses and the same bytes.  `nbytes` counts it from then on."""
        n, bp, bc = ctypes.c_int64(0), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.load().nin_gls_xjacobian_pattern(self._handle(), ctypes.byref(n), ctypes.byref(bp), ctypes.byref(bc), ctypes.c_void_p(stream)))
        return int(n.value), int(bp.value or 0), int(bc.value or 0)

    def launch_pattern_copy(self, block_ptr_ptr, block_col_ptr, stream=0):
        """the pattern copied device-to-device into the caller's buffers (nin_gls_xjacobian_pattern_copy): int64 [n_points + 1] and
        int32 [n_blocks].  Asynchronous on `stream` once the pattern exists."""
        _lib.check(_lib.load().nin_gls_xjacobian_pattern_copy(self._handle(), _vp(block_ptr_ptr), _vp(block_col_ptr), ctypes.c_void_p(stream)))

    def fetch_pattern(self):
        """(block_ptr (n_points + 1,) int64, block_col (n_blocks,) int32) on the host (waits for the device)"""
        L, n = _lib.load(), ctypes.c_int64(0)
        block_ptr = np.empty(int(self.grid.n_points) + 1, dtype=np.int64)
        _lib.check(L.nin_gls_xjacobian_pattern_host(self._handle(), _ptr(block_ptr), None, ctypes.byref(n)))
        block_col = np.empty(int(n.value), dtype=np.int32)
        _lib.check(L.nin_gls_xjacobian_pattern_host(self._handle(), _ptr(block_ptr), _ptr(block_col), ctypes.byref(n)))
        return block_ptr, block_col

    def launch_assemble(self, values_ptr, stream=0):
        """values [n_blocks][3] = the blocks of the Jacobian at the linearisation point (nin_gls_xjacobian_assemble), every entry
        written, exact zeros for the rows the forward gives as zero, two calls bit for bit the same.  Asynchronous on `stream` once
        the pattern exists.  Like launch_jvp it reads the resident coordinates: NinpolError (NIN_ESTATE) before the first
        linearisation and after Interpolator.update_points(), nothing written."""
        _lib.check(_lib.load().nin_gls_xjacobian_assemble(self._handle(), _vp(values_ptr), ctypes.c_void_p(stream)))

    def fetch_assembled(self):
        """values (n_blocks, 3) float64 on the host: one launch_assemble and the copy down (waits for the device)"""
        values = np.empty((self.pattern()[0], 3), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_xjacobian_assemble_host(self._handle(), _ptr(values)))
        return values


class _JacobianOperator(spla.LinearOperator):
    """What PermeabilityJacobian, ReducedPermeabilityJacobian and PointsJacobian share: a (n_points, cols n_elems) -- or, with per =
    n_points, (n_points, cols n_points) -- operator over a kept Jacobian whose two products are the *_apply_host and
    *_apply_transpose_host entry points of that object, one launch for k directions each."""

    _diff_mag = ()      # the optional diff_mag argument of the full Jacobian's two entry points: (None,) there, its chain folded

    def __init__(self, jac, cols, per=None):
        g = jac.grid
        self.jacobian = jac
        self._P, self._cols = int(g.n_points), int(cols)
        self._E = int(g.n_elems) if per is None else int(per)       # what a column block belongs to: a cell, or (PointsJacobian) a node
        super().__init__(dtype=np.dtype(DTYPE_F), shape=(self._P, self._cols * self._E))

    def _jvp(self, d):        # d (k, cols E) -> (k, P)
        d = np.ascontiguousarray(d, dtype=DTYPE_F)
        out = np.empty((len(d), self._P), dtype=DTYPE_F)
        _lib.check(self.jacobian._c("apply_host")(self.jacobian._handle(), len(d), _ptr(d), *self._diff_mag, _ptr(out)))
        return out

    def _vjp(self, v):        # v (k, P) -> (k, cols E)
        v = np.ascontiguousarray(v, dtype=DTYPE_F)
        out = np.empty((len(v), self._cols * self._E), dtype=DTYPE_F)
        _lib.check(self.jacobian._c("apply_transpose_host")(self.jacobian._handle(), len(v), _ptr(v), _ptr(out), *self._diff_mag))
        return out

    def _matvec(self, x):
        return self._jvp(np.asarray(x).reshape(1, -1))[0]

    def _rmatvec(self, x):
        return self._vjp(np.asarray(x).reshape(1, -1))[0]

    def _matmat(self, X):
        return self._jvp(np.asarray(X).T).T

    def _rmatmat(self, X):
        return self._vjp(np.asarray(X).T).T

    def release(self):
        self.jacobian.release()


class _FollowsUpdates:
    """update() for an operator that Interpolator.permeability_jacobian or Interpolator.points_jacobian made: it knows the Interpolator,
    the variable and the basis of that call.  Mixed into PointsJacobian and into the two classes those methods return for the permeability."""

    _interp = _variable = None
    _basis = ()         # the reduced operator's (B or None, per_cell): the basis arguments of its linearisation, kept for update()

    def _bind(self, interp, variable, basis=()):
        """what update() needs of the call that made the operator: the Interpolator, its variable, the basis"""
        self._interp, self._variable, self._basis = interp, variable, tuple(basis)
        return self

    def update(self, cell_values=None, neumann_values=None, clear=True):
        """Bring the operator to the grid's state as it is now by recomputing only the rows of the grid's dirty nodes
        (nin_gls_*jacobian_linearize_dirty_host) -- after update_permeability(cells=), update_points(nodes=),
        update_neumann_flags(nodes=) or Grid.mark_dirty() -- and return how many rows that were.  `cell_values` / `neumann_values` as
        for the call that made the operator (default: the cell variable itself / None); they may differ from the earlier ones only
        in cells all of whose vertices are dirty / at dirty nodes.  Afterwards the products, to_scipy() and assemble() are those of a
        newly made operator, bit for bit.  clear=False keeps the dirty set for another consumer.  Host-synchronous."""
        I = self._interp
        if I is None:
            raise ValueError("update() needs an operator made by Interpolator.permeability_jacobian or Interpolator.points_jacobian")
        jac = self.jacobian
        if I.grid is not jac.grid:
            raise ValueError("the Interpolator has loaded another mesh since this operator was made")
        I._check_call(variable=self._variable)
        u, _ = I._derivative_inputs(self._variable, (), cell_values, None)
        b = None
        if neumann_values is not None:
            b = np.ascontiguousarray(neumann_values, dtype=DTYPE_F)
            if b.shape != (self._P,):
                raise ValueError(f"neumann_values must have shape ({self._P},), not {b.shape}.")
        I._gls_tables_to_device(self._variable)
        basis = (_ptr(self._basis[0]), int(self._basis[1])) if self._basis else ()
        n = ctypes.c_int64(0)
        _lib.check(jac._c("linearize_dirty_host")(jac._handle(), _ptr(u), _ptr(b), *basis, int(bool(clear)), ctypes.byref(n)))
        jac._count_seed()
        return int(n.value)


class ReducedPermeabilityJacobian(_JacobianOperator):
    """Interpolator.permeability_jacobian(basis=...)'s result: the (n_points, M n_elems) Jacobian of `apply(variable, "gls")`'s node
    values in the parameters theta of perm_e = sum_m theta_(e,m) B_(e,m) (column M e + m), as a scipy LinearOperator over a
    GlsReducedJacobian: numpy in and out, host-synchronous, one launch per matvec / rmatvec and one per batched matmat / rmatmat."""

    def __init__(self, jac):
        super().__init__(jac, jac.n_params)
        self._M = self._cols

    # (scipy's hooks and release named on the class itself, as tests/test_gls_reduced_jacobian_host.py looks for them)
    _matvec, _rmatvec, _matmat, _rmatmat = (_JacobianOperator._matvec, _JacobianOperator._rmatvec, _JacobianOperator._matmat,
                                            _JacobianOperator._rmatmat)
    release = _JacobianOperator.release

    def to_scipy(self):
        """The explicit csr_matrix (n_points, M n_elems) from the fetched buffer: row p, column M e + m."""
        g = self.jacobian.grid
        R = self.jacobian.fetch()
        esup = np.asarray(g.esup).astype(np.int64)
        cols = self._M * esup[:, None] + np.arange(self._M)
        indptr = self._M * np.asarray(g.esup_ptr).astype(np.int64)
        return sp.csr_matrix((R.reshape(-1), cols.reshape(-1), indptr), shape=self.shape)


class PermeabilityJacobian(_JacobianOperator):
    """Interpolator.permeability_jacobian's result: the (n_points, 9 n_elems) Jacobian of `apply(variable, "gls")`'s node values in
    the permeability table (column 9 e + k is entry k of cell e's row-major 3 x 3 tensor; the diff_mag chain folded), as a
    scipy LinearOperator over a GlsJacobian: numpy in and out, host-synchronous, one launch per matvec / rmatvec and one per batched
    matmat / rmatmat."""

    _diff_mag = (None,)

    def __init__(self, jac):
        super().__init__(jac, 9)

    # (scipy's hooks and release named on the class itself, as tests/test_gls_jacobian_host.py looks for them)
    _matvec, _rmatvec, _matmat, _rmatmat = (_JacobianOperator._matvec, _JacobianOperator._rmatvec, _JacobianOperator._matmat,
                                            _JacobianOperator._rmatmat)
    release = _JacobianOperator.release

    def to_scipy(self):
        """The explicit csr_matrix (n_points, 9 n_elems) from the fetched buffer: row p, column 9 e + k, the fold applied."""
        g = self.jacobian.grid
        contrib, fold = self.jacobian.fetch()
        esup = np.asarray(g.esup).astype(np.int64)
        data = contrib[:, :9].copy()
        data[:, (0, 4, 8)] += (contrib[:, 9] * fold[esup])[:, None]
        cols = 9 * esup[:, None] + np.arange(9)
        indptr = 9 * np.asarray(g.esup_ptr).astype(np.int64)
        return sp.csr_matrix((data.reshape(-1), cols.reshape(-1), indptr), shape=self.shape)


class UpdatablePermeabilityJacobian(_FollowsUpdates, PermeabilityJacobian):
    """What Interpolator.permeability_jacobian() returns: a PermeabilityJacobian with `update()`, which follows local updates by
    recomputing only the rows of the grid's dirty nodes.  (A class of its own because the public names of
    PermeabilityJacobian are a pinned, closed set -- and an operator made from a bare GlsJacobian has no tables to update from.)"""


class UpdatableReducedPermeabilityJacobian(_FollowsUpdates, ReducedPermeabilityJacobian):
    """What Interpolator.permeability_jacobian(basis=...) returns: a ReducedPermeabilityJacobian with `update()`; the basis of the call
    is kept and read again for the recomputed rows."""


class PointsJacobian(_FollowsUpdates, _JacobianOperator):
    """Interpolator.points_jacobian's result: the (n_points, 3 n_points) Jacobian of `apply(variable, "gls")`'s node values in the node
    coordinates (column 3 q + c is coordinate c of node q), as a scipy LinearOperator over a GlsShapeJacobian: numpy in and out,
    host-synchronous, one launch per matvec / rmatvec and one per batched matmat / rmatmat.  The Jacobian is kept factored through
    the mesh geometry; assemble() builds the explicit matrix from it on the device.  There is no
    to_scipy(): where the other two operators reshape a fetched buffer on the host, assemble() launches kernels and reads the resident
    geometry, so it can raise.  After Interpolator.update_points() the products and assemble() raise (NinpolError, a RuntimeError):
    build a new operator at the new point, or after update_points(nodes=) call update(): the numeric pass of assemble() is then run
    whole again, the pattern is kept."""

    def __init__(self, jac):
        super().__init__(jac, 3, per=jac.grid.n_points)

    def assemble(self):
        """The explicit scipy.sparse.csr_matrix (n_points, 3 n_points): row p, column 3 q + c for every q of
        C(p) = {p} + the vertices of the cells around p + the points of the faces around p, sorted, int64 indices, explicit zeros kept
        (the rows the forward gives as zero keep their pattern).  The pattern depends on the connectivity alone and is made once per
        operator; the values are assembled on the device from the kept records and copied down."""
        jac = self.jacobian
        block_ptr, block_col = jac.fetch_pattern()
        values = jac.fetch_assembled()
        indices = (3 * block_col.astype(np.int64)[:, None] + np.arange(3, dtype=np.int64)).reshape(-1)
        A = sp.csr_matrix((values.reshape(-1), indices, 3 * block_ptr), shape=self.shape)
        A.indices, A.indptr = indices, 3 * block_ptr       # (the constructor narrows index arrays that fit int32)
        A.has_sorted_indices = True
        return A

    _matvec, _rmatvec, _matmat, _rmatmat = (_JacobianOperator._matvec, _JacobianOperator._rmatvec, _JacobianOperator._matmat,
                                            _JacobianOperator._rmatmat)
    release = _JacobianOperator.release
