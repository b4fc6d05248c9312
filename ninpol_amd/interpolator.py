"""`Interpolator`: the drop-in boundary.  Same class surface as the reference's
`ninpol.Interpolator` (ninpol/_interpolator/interpolator.pyx, interpolator.pxd:27-58) -- constructor,
`load_mesh`, `interpolate`, `load_face_data`, `get_data`, `get_dict`, `supported_methods`, `grid` --
with the work done by libninpol_amd.so: the grid is built by the native host builder, pushed to HBM
once, and `interpolate()` runs the HIP kernels.  Python here is argument checking and table packing.

What is deliberately not reproduced (out of scope): the pickle grid cache
(interpolator.pyx:93-166,244-252) and the Logger class (plain prints behind `logging=`).
"""
import ctypes
import os
import time

import numpy as np
import scipy.sparse as sp

from . import _args as A
from . import _lib
from . import topology as T
from ._lib import _ptr, _vp
from .grid import Grid
from .jacobian import (GlsJacobian, GlsReducedJacobian, GlsShapeJacobian, PermeabilityJacobian, PointsJacobian,  # noqa: F401  (their import path of old)
                       REDUCED_N_PARAMS, ReducedPermeabilityJacobian, _check_n_params, reduced_basis)
from .jacobian import (GlsDirtyJacobian, GlsDirtyReducedJacobian, UpdatablePermeabilityJacobian,  # noqa: F401
                       UpdatableReducedPermeabilityJacobian)
from .gradop import GlsGradientOperator, GradientOperator  # noqa: F401

_pinned = _lib.PinnedPool()


def pinned_pool():
    """The pool of page-locked host buffers interpolate()'s results live in (`keep_bytes`, `trim()`, `idle_bytes()`)."""
    return _pinned

DTYPE_I = np.int64
DTYPE_F = np.float64


class _MethodPlugin:
    """The reference's method-plugin convention (interpolator.pyx:631-665 docstring + call):

        prepare(grid, cells_data, points_data, faces_data, variable_to_index, variable,
                target_points, weights[out, pre-zeroed, (n_target, MX_ELEMENTS_PER_POINT)],
                neumann_ws[out, pre-zeroed])

    replacing IDWInterpolation.prepare (idw.pyx:14-30), LSInterpolation.prepare (ls.pyx:21-31) and
    GLSInterpolation.prepare (gls.pyx:38-72).  Caller owns every buffer; nothing is retained."""

    def __init__(self, name):
        self.name = name
        self.logging = False

    def prepare(self, grid, cells_data, points_data, faces_data, variable_to_index, variable, target_points,
                weights, neumann_ws):
        csr, nws = _run_weights(grid, self.name, cells_data, points_data, variable_to_index, variable,
                                target_points, add_neumann=False)
        P = grid.n_points
        targets = np.asarray(target_points, dtype=DTYPE_I)
        ptr = grid.esup_ptr
        full = len(targets) == P and np.array_equal(targets, np.arange(P))
        rows_src = np.arange(P) if full else targets
        cnt = (ptr[1:] - ptr[:-1])[rows_src]
        dst_rows = np.repeat(np.arange(len(rows_src)), cnt)
        cols = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        src = np.repeat(ptr[:-1][rows_src], cnt) + cols
        w = np.asarray(weights)
        w[dst_rows, cols] = csr[src]
        np.asarray(neumann_ws)[:len(rows_src)] = nws[rows_src]

    __call__ = prepare


def _table_key(a):
    """Identity of a resident field table: address, size and a hash of ALL its bytes (nin_hash64, OpenMP: ~5 ms for the
    0.7 GB permeability table of a 10 M-cell mesh on 16 threads; single-threaded xxh3 took 30 ms of an 83 ms interpolate())
    -- a strided sample would miss an in-place edit between samples and leave a stale K on the device."""
    h = ctypes.c_uint64(0)
    a = np.ascontiguousarray(a)
    _lib.check(_lib.load().nin_hash64(_ptr(a), a.nbytes, ctypes.byref(h)))
    return (a.__array_interface__["data"][0], a.size, h.value)


def _perm_keys(perm, dmag):
    """The fingerprint Grid._perm_key holds: the permeability's and the diff_mag's."""
    return (_table_key(perm), _table_key(dmag))


def _set_fields(grid, perm, dmag, flag, nval, key):
    """nin_fields_set (a None keeps what is resident), and its record: a host table (fingerprint `key`) went over whatever a device update
    had left."""
    _lib.check(_lib.load().nin_fields_set(grid._h, _ptr(perm), _ptr(dmag), _ptr(flag), _ptr(nval)))
    if perm is not None:
        grid.host_permeability_resident(key)


def _follow_on_device(grid, launch, *arrays):
    """Host arrays given while the grid is on a device, and what is resident there are the host rows: the same values through `launch`
    (one of Grid's *_device methods) on the grid's device, and wait -- the resident copy and the dirty set follow.  Needs torch: False
    without it, and the rows then count as edited."""
    try:
        import torch
    except ImportError:
        return False
    where = torch.device("cuda", grid.device)
    with torch.cuda.device(where):
        launch(*[torch.from_numpy(a).to(where) for a in arrays])
        torch.cuda.current_stream(where).synchronize()
    return True


class _TableCheck:
    """Is the permeability / diff_mag resident on the device still the caller's?  The answer is a hash of all 0.8 GB of the
    two tables (10 M cells: 3-5 ms on the host's OpenMP team); it is computed on a thread WHILE the kernels already run with the
    resident copy -- ctypes releases the GIL for both -- and only a caller who really edited a table pays a second run."""

    def __init__(self, grid, perm, dmag):
        import threading
        self.grid, self.perm, self.dmag, self.key = grid, perm, dmag, None
        self._t = threading.Thread(target=self._hash)
        self._t.start()

    def _hash(self):
        self.key = _perm_keys(self.perm, self.dmag)

    def join(self):
        self._t.join()

    def stale(self):
        self._t.join()
        return self.key != self.grid._perm_key

    def upload(self, flag):
        # flag None: the flags resident on the device stay (_upload_fields found a device copy that is still the newer one)
        _set_fields(self.grid, self.perm, self.dmag, flag, None, self.key)


def _upload_fields(grid, method, cells_data, points_data, variable_to_index, variable, device=0, always_perm=False,
                   speculate=False):
    """Look the field rows up exactly as the plugins do (idw.pyx:27, ls.pyx:27, gls.pyx:47-59; a missing
    name is a KeyError there too) and hand them to the device.  always_perm: upload permeability / diff_mag whenever
    the mesh has them (a DevicePlan serves any method afterwards).  speculate: when a permeability is resident already,
    upload the flags only and return a _TableCheck (the caller launches at once and asks it afterwards); else None."""
    if grid.device < 0:   # the GPU its Interpolator was built for (a bare Grid handed to a plugin: device 0)
        grid.to_device(getattr(grid, "preferred_device", device))
    P, E = grid.n_points, grid.n_elems
    v2i = variable_to_index
    flag = np.ascontiguousarray(np.asarray(points_data)[v2i["points"]["neumann_flag_" + variable]][:P], dtype=DTYPE_F)
    # flags written from the device (Interpolator.update_neumann_flags) stay resident while the CONTENTS of this variable's host
    # row are what they were at that update; an in-place edit of the row, or another variable, wins -- the permeability's rule
    if grid._flags_from_device and grid._fields_variable == variable and grid._flags_key == _table_key(flag):
        flag = None
    perm = dmag = nval = None
    key = None
    check = None
    if method == "gls" or (always_perm and "permeability" in v2i["cells"]):
        cd = np.asarray(cells_data)
        perm = np.ascontiguousarray(cd[v2i["cells"]["permeability"]][:E * 9], dtype=DTYPE_F)
        dmag = np.ascontiguousarray(cd[v2i["cells"]["diff_mag"]][:E], dtype=DTYPE_F)
        if method == "gls":
            nval = np.ascontiguousarray(np.asarray(points_data)[v2i["points"]["neumann_" + variable]][:P], dtype=DTYPE_F)
        if speculate and grid._perm_key is not None:
            check = _TableCheck(grid, perm, dmag)
            perm = dmag = None
        else:
            # permeability and diff_mag belong to the mesh: 0.8 GB at 10 M cells, uploaded once per table contents
            key = _perm_keys(perm, dmag)
            if grid._perm_key == key and grid.device >= 0:
                perm = dmag = None
    _set_fields(grid, perm, dmag, flag, nval, key)
    if flag is not None:
        # the flags on the device belong to the GRID, not to a plan: it remembers whose they are (DevicePlan.ensure_current)
        grid.host_flags_uploaded(variable)
    if check is not None:
        check.flag = flag
    return check


def _run_weights(grid, method, cells_data, points_data, variable_to_index, variable, target_points, add_neumann):
    """Upload the fields and run the kernel; weights come back in CSR position (esup layout)."""
    L = _lib.load()
    _upload_fields(grid, method, cells_data, points_data, variable_to_index, variable)
    P = grid.n_points
    targets = np.ascontiguousarray(target_points, dtype=DTYPE_I)
    full = len(targets) == 0 or (len(targets) == P and np.array_equal(targets, np.arange(P)))
    csr = np.empty(grid.nnz_esup, dtype=DTYPE_F)
    nws = np.empty(P, dtype=DTYPE_F)
    _lib.check(L.nin_weights_host(grid._h, _lib.METHOD_ID[method], None if full else _ptr(targets),
                                  0 if full else len(targets), int(bool(add_neumann)), _ptr(csr), _ptr(nws)))
    return csr, nws


def _native_interpolate(g, method):
    """nin_interpolate_csr_host into page-locked buffers (57 against 10-15 GB/s over PCIe; recycled, see _lib.PinnedPool)."""
    P = g.n_points
    nnz_max = g.nnz_esup
    empty = np.empty if os.environ.get("NINPOL_AMD_NO_PINNED") else _pinned.empty
    indptr = empty(P + 1, dtype=np.int32)
    indices = empty(nnz_max, dtype=np.int32)
    data = empty(nnz_max, dtype=DTYPE_F)
    nws = empty(P, dtype=DTYPE_F)
    nnz = ctypes.c_int64(0)
    _lib.check(_lib.load().nin_interpolate_csr_host(g._h, _lib.METHOD_ID[method], _ptr(indptr), _ptr(indices),
                                                    _ptr(data), ctypes.byref(nnz), _ptr(nws)))
    return indptr, indices[:nnz.value], data[:nnz.value], nws


def _wrap_csr(data, indices, indptr, shape):
    """scipy.sparse.csr_matrix over the three arrays as they are.  The constructor's check_format pass (min / max over all
    indices, monotone indptr: ~25 ms on 80 M entries, a third of interpolate()) is skipped: the arrays come from the
    device-side compaction, whose output is canonical by construction -- sorted, duplicate-free columns in [0, n_elems),
    indptr[0] = 0, indptr[-1] = nnz (checked in tests/test_host.py and, against the reference's own CSR, in the GPU suite)."""
    W = sp.csr_matrix(shape, dtype=data.dtype)
    W.data, W.indices, W.indptr = data, indices, indptr
    W.has_canonical_format = True        # (sorted + no duplicates: spares sum_duplicates() passes later on)
    return W


class Interpolator:
    def __init__(self, name="interpolator", logging=False, build_edges=False, device=0, num_threads=0,
                 grid_build="host"):
        """Extra keywords next to the reference's: `device` (which GPU), `num_threads` (OpenMP threads of the host
        grid builder), `grid_build` = "host" (north_star: connectivity built on the host and pushed to HBM) or
        "device" (the same arrays built by HIP kernels on `device`, csrc/grid_device.hip)."""
        _lib.load()   # fail here, loudly, if the native library is missing
        if grid_build not in ("host", "device"):
            raise ValueError("grid_build must be 'host' or 'device'")
        self.grid_build = grid_build
        self.name = name
        self.point_ordering = T.POINT_ORDERING           # utils/point_ordering.yaml as data
        self.is_grid_initialized = False
        self.build_edges = int(build_edges)
        self.gls, self.idw, self.ls = _MethodPlugin("gls"), _MethodPlugin("idw"), _MethodPlugin("ls")
        self.supported_methods = {"gls": self.gls.prepare, "idw": self.idw.prepare, "ls": self.ls.prepare}
        self.variable_to_index = {"points": {}, "cells": {}, "faces": {}}
        self.types_per_dimension = {k: list(v) for k, v in T.TYPES_PER_DIMENSION.items()}
        self.cells_data = np.zeros((1, 1), dtype=DTYPE_F)
        self.cells_data_dimensions = np.zeros(1, dtype=DTYPE_I)
        self.points_data = np.zeros((1, 1), dtype=DTYPE_F)
        self.points_data_dimensions = np.zeros(1, dtype=DTYPE_I)
        self.faces_data = np.zeros((1, 1), dtype=DTYPE_F)
        self.faces_data_dimensions = np.zeros(1, dtype=DTYPE_I)
        self.logging = int(logging)
        self.device = int(device)
        self.num_threads = int(num_threads)
        self.mesh_obj = None
        self.grid = None
        self.points_coords = None

    @property
    def points_coords(self):
        """The node coordinates as load_mesh() / update_points() last saw them (after an update from a device tensor: read
        back from the grid on first use)."""
        if self._points_coords is None and self._points_on_device:
            self._points_coords = np.ascontiguousarray(self.grid.point_coords)
            self._points_on_device = False
        return self._points_coords

    @points_coords.setter
    def points_coords(self, value):
        self._points_coords = value
        self._points_on_device = False

    def _log(self, msg, kind="INFO"):
        if self.logging:
            print(f"[{kind:<5}] ({time.strftime('%H:%M:%S'):<8}) {msg}")

    _NOT_ASKED = object()

    def _check_call(self, method=_NOT_ASKED, variable=_NOT_ASKED):
        """What an entry point asks first: a mesh is loaded, `method` is known, `variable` is a cell variable (the last two if given)."""
        if not self.is_grid_initialized:
            raise ValueError("Grid not initialized. Please load a mesh first.")
        if method is not self._NOT_ASKED and method not in self.supported_methods:
            raise ValueError(f"Method '{method}' not supported. Supported methods are: "
                             f"{list(self.supported_methods.keys())}")
        if variable is not self._NOT_ASKED and variable not in self.variable_to_index["cells"]:
            raise ValueError(f"Variable '{variable}' not found in cells data. "
                             "Point -> Cell interpolation not supported yet.")

    def is_cached(self, filename):
        """The reference's pickle cache (interpolator.pyx:93-111) is not kept: nothing is ever cached."""
        return None

    # ---- load_mesh, interpolator.pyx:168-252 ----------------------------------------------------
    def load_mesh(self, filename="", mesh_obj=None):
        if filename == "" and mesh_obj is None:
            raise ValueError("Filename for the mesh or meshio.Mesh object must be provided.")
        if filename != "":
            self._log(f"Reading mesh from {filename}")
            try:
                import meshio   # the reference's reader (interpolator.pyx:188), when it is installed
                self.mesh_obj = meshio.read(filename)
            except ImportError as e:
                # without meshio: the format the reference's own tests write (legacy VTK, tests/accuracy_test.py:46) is read natively
                if not str(filename).lower().endswith(".vtk"):
                    raise ImportError("reading this mesh file needs meshio (only legacy .vtk files are read without it); "
                                      "pass mesh_obj= instead") from e
                from . import vtk_legacy
                self.mesh_obj = vtk_legacy.read(filename)
        else:
            self._log("Using mesh object")
            self.mesh_obj = mesh_obj
        t0 = time.time()
        args = self.process_mesh(self.mesh_obj)
        self.points_coords = np.ascontiguousarray(np.asarray(self.mesh_obj.points).astype(DTYPE_F))
        self.grid = Grid(*args, coords=self.points_coords, num_threads=self.num_threads,
                         build_device=self.device if self.grid_build == "device" else None)
        self.grid.preferred_device = self.device
        self._log(f"Grid built in {time.time() - t0:.2f} seconds")
        t0 = time.time()
        self.variable_to_index = {"points": {}, "cells": {}, "faces": {}}
        if self.mesh_obj.cell_data:
            self.load_cell_data()
        else:
            self.cells_data = np.zeros((1, 1), dtype=DTYPE_F)
            self.cells_data_dimensions = np.zeros(1, dtype=DTYPE_I)
        if self.mesh_obj.point_data:
            self.load_point_data()
        else:
            self.points_data = np.zeros((1, 1), dtype=DTYPE_F)
            self.points_data_dimensions = np.zeros(1, dtype=DTYPE_I)
        self._log(f"Data loaded in {time.time() - t0:.2f} seconds")
        self.is_grid_initialized = True
        self._log(f"Mesh loaded successfully: {self.grid.n_points} points and {self.grid.n_elems} elements.")

    def update_points(self, points, nodes=None):
        """Move the mesh: new node coordinates, same connectivity (ALE and free-surface steps, mesh smoothing, shape optimisation).
        `points`: an array of the shape load_mesh() saw, (n_points, 2 or 3) -- synchronous -- or a float64 torch tensor of that
        shape on this Interpolator's device: then the geometry is recomputed from device memory, asynchronously on torch's current
        stream, with no host copy; launches of a DevicePlan / CellToNode on that stream follow in order, the host-synchronous
        methods (interpolate, apply, apply_transpose) need `torch.cuda.current_stream().synchronize()` first.

        Afterwards every grid array and every result is bit for bit what a fresh load_mesh() of the moved mesh gives.  What stays:
        the connectivity, the fields (permeability, Neumann flags), the GLS launch plan, the transpose index, all scratch.  What
        does not follow by itself: weights already computed -- matrices returned earlier, the buffers a DevicePlan.launch wrote,
        the weights a CellToNode holds (call its refresh()) -- and `mesh_obj.points`, which is the caller's.

        `nodes` (1-D integer ids in [0, n_points), m of them): only those nodes move; `points` is then (m, coords_dim), row i the new
        position of node nodes[i] (coords_dim: the columns load_mesh() saw).  Duplicate ids with identical rows are fine; with
        different rows one of them wins, and which one is unspecified.  Only the geometry around the moved nodes is made again -- the
        result is the same bits -- and the whole mesh is NOT marked dirty: the nodes whose weights can move, the vertices of the cells
        around the moved nodes, join the grid's dirty set (Grid.dirty_nodes), and DevicePlan.launch_dirty() and
        CellToNode.recompute_weights(dirty_only=True) recompute exactly those rows (the whole-mesh form above makes every node dirty).
        `nodes` a torch tensor (int32 / int64) on this Interpolator's device, `points` a float64 tensor there: asynchronous on torch's
        current stream with the rules of the device path above; `points_coords` is read back from the grid on first use.  Ids are
        checked on the device: one outside [0, n_points) moves nothing and marks nothing, and the next launch_dirty() raises with the
        count.
        `nodes` a numpy array (or a list), `points` numpy: `points_coords` is patched in place; ids are checked here (ValueError);
        synchronous.  On a grid that is on a device the same kernels run and the dirty set follows; a grid on no device recomputes its
        host geometry (works without a GPU; there is no dirty set then: the first upload makes every node dirty anyway).
        Host and device arguments cannot be mixed (TypeError)."""
        self._check_call()
        if nodes is not None:
            return self._update_points_nodes(points, nodes)
        g = self.grid
        on_device = A.on_gpu(points)
        if on_device and g.device < 0:
            g.to_device(self.device)
        g.load_point_coords(points)
        if on_device:
            self._points_coords, self._points_on_device = None, True
        else:
            self.points_coords = np.ascontiguousarray(np.array(A.to_host(points), dtype=DTYPE_F))

    def _update_points_nodes(self, rows, nodes):
        g = self.grid
        cd = g._coords_dim
        if A.on_gpu(nodes):
            m = A.device_ids(nodes, "nodes", self.device)
            rows = A.device_tensor(rows, "points", self.device, "nodes", ((m, cd),))
            if m == 0:
                return
            if g.device < 0:
                g.to_device(self.device)
            g.scatter_point_coords(nodes.detach().contiguous(), rows)
            self._points_coords, self._points_on_device = None, True
            return
        if A.on_gpu(rows):
            raise TypeError(f"points must be on the host when nodes is (a numpy array), not on {rows.device}")
        ids = A.host_ids(A.to_host(nodes), "nodes", int(g.n_points))
        X = A.host_float64(A.to_host(rows), "points", ((len(ids), cd),))
        if len(ids) == 0:
            return
        pc = self.points_coords           # (after a device update: read back from the grid first)
        g.scatter_point_coords(ids, X)
        pc[ids] = X                       # duplicate ids with different rows: numpy keeps the last, the device an unspecified one

    # ---- changing permeability ---------------------------------------------------------------------
    def _perm_rows(self):
        """The `permeability` and `diff_mag` rows of cells_data as _upload_fields reads them (views: same addresses, same hash)."""
        self._check_call()
        v2i = self.variable_to_index["cells"]
        if "permeability" not in v2i or "diff_mag" not in v2i:
            raise ValueError("Variable 'permeability' not found in cells data: load a mesh that carries it.")
        E = self.grid.n_elems
        cd = np.asarray(self.cells_data)
        return cd[v2i["permeability"]][:E * 9], cd[v2i["diff_mag"]][:E]

    def update_permeability(self, K, scale=None, cells=None):
        """Replace the permeability of the loaded mesh: K of shape (n_elems, 3, 3) or (n_elems, 9), optionally times a per-cell
        factor `scale` of shape (n_elems,) (mobility times absolute permeability: one multiplication per entry, rounded once).
        diff_mag follows.  Connectivity, geometry, Neumann flags and the GLS launch plan stay.

        A numpy array (or a CPU torch tensor): the `permeability` and `diff_mag` rows of `cells_data` are rewritten in place -- what a
        fresh load_mesh() of the mesh with that K holds, bit for bit -- and the next interpolate() / apply() / DevicePlan.refresh()
        finds the table changed and uploads it, as after any in-place edit.  Works without a GPU.

        A float64 torch tensor on this Interpolator's device (`scale`, if given, one too): the resident table is rewritten from device
        memory by a kernel on torch's current stream -- no host copy, no synchronisation.  Launches of a DevicePlan / CellToNode
        (recompute_weights()) on that stream follow in order; the host-synchronous methods (interpolate, apply, apply_transpose)
        need `torch.cuda.current_stream().synchronize()` first.  The `cells_data` rows are NOT touched: fetch_permeability() brings
        the device's values back.  Precedence: the device copy stays resident, through any number of interpolate() / refresh()
        calls, until the CONTENTS of the host rows change; an in-place edit of `cells_data` made afterwards wins at the next call
        that reads the tables, exactly as an edit always did.

        `cells` (1-D integer ids in [0, n_elems), m of them): only those cells change; K is then (m, 3, 3) or (m, 9) and `scale` (m,),
        row i for cell cells[i].  Duplicate ids with identical rows are fine; with different rows one of them wins, and which one is
        unspecified.  The nodes whose weights can move -- the vertices of those cells -- join the grid's dirty set (Grid.dirty_nodes),
        and DevicePlan.launch_dirty() recomputes exactly their rows.
        `cells` a torch tensor (int32 / int64) on this Interpolator's device, K and scale float64 tensors there: the rows are scattered
        into the resident table by a kernel on torch's current stream, with the rules of the device path above (no host copy, the
        `cells_data` rows are not touched, fetch_permeability() brings the patched table back).  Ids are checked on the device: one
        outside [0, n_elems) writes nothing, and the next launch_dirty() raises with the count.
        `cells` a numpy array (or a list), K numpy: the rows of `cells_data` are rewritten in place for those cells; ids are checked
        here (ValueError).  Works without a GPU.  If the grid is on a device and its resident table is the host rows' (not a newer
        device copy), the same rows also go through the scatter (needs torch; synchronous), so the resident table and the dirty set
        follow and the next call uploads nothing; otherwise the edit is found and uploaded whole by the next call that reads the
        tables, as any in-place edit is -- and then every node is dirty.
        Host and device arguments cannot be mixed (TypeError)."""
        perm_row, dmag_row = self._perm_rows()
        if cells is not None:
            return self._update_permeability_cells(K, scale, cells, perm_row, dmag_row)
        g = self.grid
        E = g.n_elems
        if A.on_gpu(K):
            Kd = A.device_tensor(K, "K", self.device, "K", ((E, 3, 3), (E, 9)), cpu_tensor_passes=True)
            sd = None if scale is None else A.device_tensor(scale, "scale", self.device, "K", ((E,),), cpu_tensor_passes=True)
            if g.device < 0:
                g.to_device(self.device)
            g.load_permeability_device(Kd, sd)
            g.permeability_from_device(_perm_keys, perm_row, dmag_row)
            return
        if A.on_gpu(scale):
            raise ValueError(f"scale must be on the host when K is, not {scale.device}")
        K9 = A.host_float64(A.to_host(K), "K", ((E, 3, 3), (E, 9))).reshape(E, 9)
        if scale is not None:
            K9 = A.host_float64(A.to_host(scale), "scale", ((E,),))[:, None] * K9
        perm_row[:] = K9.reshape(-1)
        dmag_row[:] = self.compute_diffusion_magnitude(K9)
        g.host_permeability_edited()

    def _update_permeability_cells(self, K, scale, cells, perm_row, dmag_row):
        g = self.grid
        if A.on_gpu(cells):
            m = A.device_ids(cells, "cells", self.device)
            Kd = A.device_tensor(K, "K", self.device, "cells", ((m, 3, 3), (m, 9)))
            sd = None if scale is None else A.device_tensor(scale, "scale", self.device, "cells", ((m,),))
            cd = cells.detach().contiguous()
            if g.device < 0:
                g.to_device(self.device)
            if g._perm_key is None:
                # nothing was ever uploaded to this device copy: the host table goes over first (through the device path: the same bits)
                import torch
                g.load_permeability_device(torch.from_numpy(np.ascontiguousarray(perm_row)).to(f"cuda:{self.device}"))
            g.scatter_permeability_device(cd, Kd, sd)
            g.permeability_from_device(_perm_keys, perm_row, dmag_row)
            return
        if A.on_gpu(K) or A.on_gpu(scale):
            raise TypeError("K and scale must be on the host when cells is (a numpy array), not on " +
                            str((K if A.on_gpu(K) else scale).device))
        E = g.n_elems
        ids = A.host_ids(A.to_host(cells), "cells", E)
        m = len(ids)
        K9 = A.host_float64(A.to_host(K), "K", ((m, 3, 3), (m, 9))).reshape(m, 9)
        if scale is not None:
            K9 = A.host_float64(A.to_host(scale), "scale", ((m,),))[:, None] * K9
        if m == 0:
            return
        # is the resident table the host rows as they are NOW?  Only then can the device follow row by row
        in_step = (g.device >= 0 and g._perm_key is not None and not g._perm_from_device and
                   g._perm_key == _perm_keys(perm_row, dmag_row))
        perm_row.reshape(E, 9)[ids] = K9
        dmag_row[ids] = self.compute_diffusion_magnitude(K9)
        if in_step and _follow_on_device(g, g.scatter_permeability_device, ids, K9):
            g.host_permeability_resident(_perm_keys(perm_row, dmag_row))   # the rows ARE the resident table: nothing to upload
        else:
            g.host_permeability_edited()

    def fetch_permeability(self):
        """The permeability resident on the device read back into the `permeability` and `diff_mag` rows of `cells_data` (after
        update_permeability() from device tensors the rows still hold the older values); waits for the device.  The rows then ARE
        the resident table and are recorded as such: the next call uploads nothing.  Returns K as (n_elems, 3, 3).  With nothing
        resident on a device the rows are returned as they are."""
        perm_row, dmag_row = self._perm_rows()
        g = self.grid
        got = g.fetch_permeability()
        if got is not None:
            perm_row[:] = got[0].reshape(-1)
            dmag_row[:] = got[1]
            g.host_permeability_resident(_perm_keys(perm_row, dmag_row))
        return np.array(perm_row).reshape(g.n_elems, 3, 3)

    @property
    def permeability_on_device(self):
        """True while the permeability resident on the device came from update_permeability() with device tensors and is newer than
        the `cells_data` rows: until fetch_permeability(), a host-side update_permeability(), or the call that finds the host rows
        edited and uploads them.  It reports what has HAPPENED: an in-place edit of the rows that no call has read yet -- made
        before or after the device update -- does not show here until the next call that reads the tables uploads it."""
        g = self.grid
        return g is not None and g._perm_from_device

    # ---- changing boundary conditions ----------------------------------------------------------------
    def _flag_row(self, variable):
        """The `neumann_flag_<variable>` row of points_data as _upload_fields reads it (a view: same address, same hash)."""
        self._check_call()
        name = "neumann_flag_" + str(variable)
        if name not in self.variable_to_index["points"]:
            raise ValueError(f"Variable '{name}' not found in points data.")
        return np.asarray(self.points_data)[self.variable_to_index["points"][name]][:self.grid.n_points]

    def update_neumann_flags(self, variable, flags, nodes=None):
        """Change the boundary condition of `variable`: which nodes carry its Neumann flag (a boundary that switches between Dirichlet
        and Neumann, wells that open and close, two variables with different Neumann sets served in turn).  `flags` has shape
        (n_points,); a value is SET when, as an integer, it is not zero -- `.astype(int)`, truncation toward zero, as everywhere else:
        0.5 and -0.5 are not set -- or, for bool / uint8, when it is non-zero.  Connectivity, geometry, permeability and the GLS launch
        plan stay; Neumann VALUES are not part of the weights and are not touched.

        The flag of node n is read by row n only, so exactly the nodes whose bit CHANGES join the grid's dirty set (Grid.dirty_nodes), and
        DevicePlan.launch_dirty() / CellToNode.recompute_weights(dirty_only=True) recompute exactly those rows -- a node that became
        Dirichlet gets its zero row.  An update that rewrites equal values marks nothing.

        A torch tensor (float64, bool or uint8) on this Interpolator's device: the resident flags are rewritten by a kernel on torch's
        current stream -- no host copy, no synchronisation, `points_data` is NOT touched (fetch_neumann_flags() brings the bits back).
        `variable` may differ from the one whose flags are resident: the grid then holds `variable`'s flags, and only the nodes whose
        bit differs are dirty -- switching a weight buffer from u to v costs the differing rows, not a full launch.  Precedence as for
        update_permeability(): the device copy stays resident through refresh() / interpolate() / apply() / apply_transpose() until the
        CONTENTS of the host row change; an in-place edit of the row made afterwards wins at the next call that reads the tables (and
        then every node is dirty).  The host-synchronous methods need `torch.cuda.current_stream().synchronize()` first.

        `nodes` (1-D integer ids in [0, n_points), m of them): only those nodes change; `flags` is then (m,), value i for node nodes[i].
        Duplicate ids with equal values are fine; with different values one of them wins, and which one is unspecified.
        `nodes` a torch tensor (int32 / int64) on this Interpolator's device, `flags` a tensor there: scattered by a kernel on torch's
        current stream with the rules above.  `variable` must be the one whose flags are resident (ValueError: the other rows would
        belong to a different variable; with nothing resident yet its host row goes over first).  Ids are checked on the device: one
        outside [0, n_points) writes nothing and marks nothing, and the next launch_dirty() raises with the count.

        numpy arrays or lists (float64, integers or bool): the `neumann_flag_<variable>` row of `points_data` is rewritten in place with
        the values as given -- what a fresh load_mesh() of the mesh with those flags holds.  Works without a GPU; ids are checked here
        (ValueError).  If the grid is on a device and the resident flags are this variable's host row (not a newer device copy, not
        another variable's), the same values also go through the kernels (needs torch; synchronous), so the resident flags and the dirty
        set follow; otherwise the next call that reads the tables uploads the row, as after any in-place edit.
        Host and device arguments cannot be mixed (TypeError)."""
        row = self._flag_row(variable)
        g = self.grid
        P = len(row)                      # (n_points)
        if A.on_gpu(flags) or A.on_gpu(nodes):
            A.require_device_tensor(flags, "flags", self.device, "nodes")
            if nodes is not None:
                A.require_device_tensor(nodes, "nodes", self.device, "flags")
            Fd = A.device_tensor(flags, "flags", self.device, "nodes", also=("bool", "uint8"))
            if nodes is None:
                A.check_shape(Fd.shape, "flags", ((P,),))
                if g.device < 0:
                    g.to_device(self.device)
                g.load_flags_device(Fd)
                g.flags_from_device(variable, _table_key, row)   # only the nodes whose bit differs were marked: no mark_all_dirty()
                return
            m = A.device_ids(nodes, "nodes", self.device)
            A.check_shape(Fd.shape, "flags", ((m,),))
            if g.device >= 0 and g._fields_variable is not None and g._fields_variable != variable:
                raise ValueError(f"the flags resident on the device are those of '{g._fields_variable}', not of '{variable}': a subset of "
                                 "nodes can only be patched into its own variable (pass the whole array to switch)")
            if m == 0:
                return
            if g.device < 0:
                g.to_device(self.device)
            if g._fields_variable is None:
                # nothing is resident on this device copy yet: the host row goes over first (through the device path: the same bits)
                import torch
                g.load_flags_device(torch.from_numpy(np.ascontiguousarray(row, dtype=DTYPE_F)).to(f"cuda:{self.device}"))
            g.scatter_flags_device(nodes.detach().contiguous(), Fd)
            g.flags_from_device(variable, _table_key, row)
            return
        F = A.host_float64(A.to_host(flags), "flags", numbers_only=True)
        ids = None if nodes is None else A.host_ids(A.to_host(nodes), "nodes", P, empty_of_any_dtype=True)
        A.check_shape(F.shape, "flags", ((P,) if ids is None else (len(ids),),))
        if F.size == 0:
            return
        if ids is None:
            row[:] = F
        else:
            row[ids] = F                  # duplicate ids with different values: numpy keeps the last, the device an unspecified one
        # is what is resident this variable's host row (not a newer device copy, not another variable's)?  Then the device follows, and
        # the row still IS what is resident: nothing to record
        if g.device >= 0 and g._fields_variable == variable and not g._flags_from_device:
            if ids is None:
                _follow_on_device(g, g.load_flags_device, F)
            else:
                _follow_on_device(g, g.scatter_flags_device, ids, F)

    def fetch_neumann_flags(self, variable):
        """The Neumann bits resident on the device read back into the `neumann_flag_<variable>` row of `points_data` as 0.0 / 1.0 (after
        update_neumann_flags() from device tensors the row still holds the older values); waits for the device.  The row then IS what is
        resident and is recorded as such.  `variable` must be the one whose flags are resident (ValueError).  Returns the row (a copy).
        With nothing resident on a device the row is returned as it is."""
        row = self._flag_row(variable)
        g = self.grid
        if g.device >= 0 and g._fields_variable is not None:
            if g._fields_variable != variable:
                raise ValueError(f"the flags resident on the device are those of '{g._fields_variable}', not of '{variable}'")
            got = g.fetch_flags()
            if got is not None:
                row[:] = got
                g.flags_fetched()
        return np.array(row)

    @property
    def neumann_flags_on_device(self):
        """True while the Neumann flags resident on the device came from update_neumann_flags() with device tensors and are newer than
        the `points_data` row: until fetch_neumann_flags(), or the call that finds the host row edited (or another variable asked for)
        and uploads it.  Like permeability_on_device it reports what has HAPPENED: an in-place edit of the row that no call has read
        yet does not show here."""
        g = self.grid
        return g is not None and g._flags_from_device

    def load_arrays(self, points, cells, cell_data=None, point_data=None):
        """`load_mesh` from plain arrays, no meshio object.  `cells` is a list of
        (type name, (n, nodes per cell) int array) blocks in meshio's vertex order -- one block per type, as the
        reference's `cell_data_dict` assumes -- `cell_data[var]` one array over all cells in block order (or a list
        of per-block arrays), `point_data[var]` one array per node."""
        from .mesh import Mesh, CellBlock
        blocks = [CellBlock(t, np.asarray(d)) for t, d in cells]
        cd = {}
        for name, a in (cell_data or {}).items():
            if isinstance(a, (list, tuple)):
                cd[name] = [np.asarray(x) for x in a]
            else:
                a = np.asarray(a)
                cuts = np.cumsum([len(b) for b in blocks])[:-1]
                cd[name] = np.split(a, cuts)
        self.load_mesh(mesh_obj=Mesh(np.asarray(points), blocks, point_data=dict(point_data or {}), cell_data=cd))

    def process_mesh(self, mesh):
        """interpolator.pyx:255-369, vectorised: fixed-width -1 padded connectivity + topology tables."""
        dim = T.mesh_dimension([b.type for b in mesh.cells])
        npoel, nfael, lnofa, lpofa, nedel, lpoed = T.topology_tables(dim)
        blocks = [b for b in mesh.cells if b.type in self.types_per_dimension[dim]]
        n_elems = int(sum(len(b.data) for b in blocks))
        n_points = int(np.asarray(mesh.points).shape[0])
        connectivity = np.empty((max(n_elems, 0), T.MAX_POINTS_PER_ELEMENT), dtype=DTYPE_I)
        element_types = np.empty(max(n_elems, 0), dtype=DTYPE_I)
        # native packing (csrc/pack_host.cpp): -1 padded rows + types, block after block
        data = [np.ascontiguousarray(np.asarray(b.data), dtype=DTYPE_I).reshape(len(b.data), -1) for b in blocks]
        nb = len(blocks)
        ptrs = (ctypes.c_void_p * max(nb, 1))(*[d.ctypes.data for d in data])
        rows = np.array([d.shape[0] for d in data], dtype=DTYPE_I)
        cols = np.array([d.shape[1] for d in data], dtype=DTYPE_I)
        tids = np.array([T.ELEMENTS[b.type]["element_type"] for b in blocks], dtype=DTYPE_I)
        _lib.check(_lib.load().nin_pack_connectivity(nb, ptrs, _ptr(rows), _ptr(cols), _ptr(tids), _ptr(connectivity),
                                                     _ptr(element_types)))
        return (dim, n_elems, n_points, npoel, nfael, lnofa, lpofa, nedel, lpoed, connectivity, element_types,
                self.logging, self.build_edges)

    # ---- data tables, interpolator.pyx:372-509 --------------------------------------------------
    def load_data(self, data_dict, data_type):
        n_vars = len(data_dict)
        n = self.grid.n_elems if data_type == "cells" else self.grid.n_points
        dims = np.zeros(n_vars, dtype=DTYPE_I)
        max_shape = 1
        for index, variable in enumerate(data_dict):
            a = np.asarray(data_dict[variable])
            cur = a.shape[1] if a.ndim > 1 else 1
            max_shape = max(max_shape, cur)
            self.variable_to_index[data_type][variable] = index
            dims[index] = cur
        table = np.zeros((n_vars, n * max_shape), dtype=DTYPE_F)
        for variable in data_dict:
            self._log(f"Loading {data_type} data for variable '{variable}'")
            index = self.variable_to_index[data_type][variable]
            cur = int(dims[index])
            a = np.ascontiguousarray(data_dict[variable], dtype=DTYPE_F)
            if len(a) < n:
                raise IndexError(f"index {len(a)} is out of bounds for axis 0 with size {len(a)}")
            a2 = a.reshape(len(a), -1)     # row-major (len, src_cols); the native packer takes the first `cur` columns
            if n:
                _lib.check(_lib.load().nin_pack_table_row(_ptr(a2), n, a2.shape[1], cur, _ptr(table[index])))
        if data_type == "cells":
            self.cells_data_dimensions, self.cells_data = dims, table
        else:
            self.points_data_dimensions, self.points_data = dims, table

    def load_cell_data(self):
        dim = self.grid.dim
        cell_data_dict = self.mesh_obj.cell_data_dict
        cell_data = {}
        for variable in cell_data_dict:
            parts = [np.asarray(cell_data_dict[variable][t]) for t in cell_data_dict[variable]
                     if t in self.types_per_dimension[dim]]
            cell_data[variable] = np.concatenate(parts) if parts else np.array([])
            if variable == "permeability":
                cell_data["diff_mag"] = self.compute_diffusion_magnitude(cell_data["permeability"])
        self.load_data(cell_data, "cells")

    def load_point_data(self):
        self.load_data(self.mesh_obj.point_data, "points")

    def compute_diffusion_magnitude(self, permeability):
        """interpolator.pyx:501-509 AS COMPILED: `detKs ** (1 / 3)` has two C integer literals and the
        module is built with cdivision=True (setup.py:100-108), so the exponent is 0 and the value the
        reference uses is (1 - 3 / tr K)^2.  Only this form reproduces the GLS numbers the reference
        publishes (tests/test_kat.py)."""
        K = np.ascontiguousarray(np.reshape(np.asarray(permeability, dtype=DTYPE_F), (len(permeability), 9)))
        # det ** 0 == 1.0 for every float (0, inf and nan included), so the determinant is not computed:
        # (1 - 3 * 1.0 / tr)^2, tr in np.trace's order, is the value the reference's expression yields, bit for bit
        # (native: csrc/pack_host.cpp, built without FMA contraction)
        out = np.empty(len(K), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_diff_mag(_ptr(K), len(K), _ptr(out)))
        return out

    def load_face_data(self, data_dict, face_connectivity=np.array([[]], dtype=int)):
        """interpolator.pyx:456-499."""
        face_to_grid = np.arange(self.grid.n_faces, dtype=DTYPE_I)
        A = np.ascontiguousarray(face_connectivity)
        if len(A) > 0 and A.size > 0:
            B = np.ascontiguousarray(self.grid.inpofa).astype(A.dtype)
            A_view = A.view([("", A.dtype)] * A.shape[1]).ravel()
            B_view = B.view([("", B.dtype)] * B.shape[1]).ravel()
            order = np.argsort(B_view)
            face_to_grid = order[np.searchsorted(B_view[order], A_view)]
        self.faces_data = np.zeros((len(data_dict), self.grid.n_faces), dtype=DTYPE_F)
        self.faces_data_dimensions = np.zeros(len(data_dict), dtype=DTYPE_I)
        for i, variable in enumerate(data_dict):
            a = np.asarray(data_dict[variable])
            self.variable_to_index["faces"][variable] = i
            self.faces_data_dimensions[i] = a.shape[1] if a.ndim > 1 else 1
            self.faces_data[i] = a[face_to_grid].astype(DTYPE_F).reshape(self.grid.n_faces, -1)[:, 0]

    def get_dict(self):
        return {"point_ordering": self.point_ordering, "variable_to_index": self.variable_to_index,
                "cells_data": np.asarray(self.cells_data), "cells_data_dimensions": np.asarray(self.cells_data_dimensions),
                "points_data": np.asarray(self.points_data), "points_data_dimensions": np.asarray(self.points_data_dimensions)}

    def get_data(self, data_type, index, variable):
        if data_type == "cells":
            if variable not in self.variable_to_index["cells"]:
                raise ValueError(f"Variable '{variable}' not found in cells data.")
            return np.asarray(self.cells_data[self.variable_to_index["cells"][variable]])[index]
        if variable not in self.variable_to_index["points"]:
            raise ValueError(f"Variable '{variable}' not found in points data.")
        return np.asarray(self.points_data[self.variable_to_index["points"][variable]])[index]

    # ---- interpolate, interpolator.pyx:549-629 ---------------------------------------------------
    def interpolate(self, variable, method, target_points=np.array([], dtype=DTYPE_I)):
        self._check_call(method, variable)
        target_points = np.asarray(target_points, dtype=DTYPE_I)
        every_node = len(target_points) == 0    # interpolator.pyx:557-558: an empty list means all nodes
        if self.cells_data_dimensions[self.variable_to_index["cells"][variable]] > 1:
            raise ValueError(f"Variable '{variable}' has more than one dimension. Vector data not supported yet.")
        self._log(f"Interpolating variable '{variable}' using method '{method}'")
        g = self.grid
        if method == "gls" and g.dim == 2:
            # the reference's 2-D GLS system is rank deficient by construction (the z-gradient unknowns are tied only
            # to each other) and what dgels returns for it is an accident of its singularity exit: not reproduced
            import warnings
            warnings.warn("GLS on a 2-D mesh: the reference's result there is undefined (rank-deficient system); "
                          "values will not match ninpol's", RuntimeWarning, stacklevel=2)
        P, E = g.n_points, g.n_elems
        if g.device < 0:
            g.to_device(self.device)
        t0 = time.time()
        # (the identity list is only materialised when somebody asks for it: arange + compare cost 20 ms at 10 M nodes)
        full = every_node or (len(target_points) == P and np.array_equal(target_points, np.arange(P)))
        idx_t = np.int32 if max(g.nnz_esup, E, P) < np.iinfo(np.int32).max else np.int64
        if full and idx_t is np.int32:
            # one native call: kernel with `data[j] = weights + neumann_ws[row]` (interpolator.pyx:618) fused, then the
            # device-side csr_matrix + eliminate_zeros (interpolator.pyx:622-624); only the surviving entries cross PCIe
            # Speculation is adaptive (advisor, round 3): a caller who edits K before every call (nonlinear / time loops) would pay a
            # wasted run each time -- after a stale check the next calls hash first, and speculation comes back once a call has
            # found the resident table still current.
            key_before = g._perm_key
            check = _upload_fields(g, method, self.cells_data, self.points_data, self.variable_to_index, variable,
                                   speculate=not g._perm_edited_last_call)
            try:
                indptr, indices, data, nws = _native_interpolate(g, method)
            except BaseException:
                if check is not None:
                    check.join()                         # never leave the hash thread behind
                raise
            if check is None:                            # hashed first: was the table edited since the last call?
                edited = key_before is not None and g._perm_key != key_before
            else:
                edited = check.stale()
                if edited:                               # the caller's permeability is not the resident one: again, with it
                    del indptr, indices, data, nws
                    check.upload(check.flag)
                    indptr, indices, data, nws = _native_interpolate(g, method)
            g.permeability_edit_seen(edited)
            self._log(f"Interpolation done in {time.time() - t0:.2f} seconds")
            return _wrap_csr(data, indices, indptr, (P, E)), nws
        csr, nws = _run_weights(g, method, self.cells_data, self.points_data, self.variable_to_index, variable,
                                target_points, add_neumann=True)
        self._log(f"Interpolation done in {time.time() - t0:.2f} seconds")
        if full:
            W = sp.csr_matrix((csr, g.esup.astype(idx_t), g.esup_ptr.astype(idx_t)), shape=(P, E))
        else:
            # The reference only works for the full node set (its plugins write weights[point] into a
            # table sized by n_target).  Here a subset returns row i = node target_points[i].
            ptr = g.esup_ptr
            cnt = (ptr[1:] - ptr[:-1])[target_points]
            src = np.repeat(ptr[:-1][target_points], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
            indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(idx_t)
            W = sp.csr_matrix((csr[src], g.esup[src].astype(idx_t), indptr), shape=(len(target_points), E))
            nws = nws[target_points]
        W.eliminate_zeros()
        return W, nws

    def apply(self, variable, method, values=None):
        """Interpolate cell fields to the nodes on the device: `W.dot(u)` of the reference's callers
        (tests/utils/analytical.py:236) without bringing W to the host.  `values`: one cell array (n_elems,) -- default:
        the cell variable `variable` itself -- or k of them as (k, n_elems): the weights (which depend on `variable`
        only through its Neumann flags) are computed once and applied to every field.  Returns (node_values,
        neumann_ws), node_values shaped like `values` with n_points in place of n_elems; Dirichlet rows are 0."""
        self._check_call(method, variable)
        g = self.grid
        if g.device < 0:
            g.to_device(self.device)
        if values is None:
            values = np.asarray(self.cells_data[self.variable_to_index["cells"][variable]])[:g.n_elems]
        u = np.ascontiguousarray(values, dtype=DTYPE_F)
        if u.shape != (g.n_elems,) and not (u.ndim == 2 and u.shape[0] >= 1 and u.shape[1] == g.n_elems):
            raise ValueError(f"values must have shape ({g.n_elems},) or (k, {g.n_elems}), not {u.shape}.")
        _upload_fields(g, method, self.cells_data, self.points_data, self.variable_to_index, variable)
        k = 1 if u.ndim == 1 else u.shape[0]
        out = np.empty(g.n_points if u.ndim == 1 else (k, g.n_points), dtype=DTYPE_F)
        nws = np.empty(g.n_points, dtype=DTYPE_F)
        _lib.check(_lib.load().nin_apply_fields_host(g._h, _lib.METHOD_ID[method], _ptr(u), k, _ptr(out), _ptr(nws)))
        return out, nws

    def apply_transpose(self, variable, method, values):
        """The adjoint of `apply()`: node fields back to the cells, `W.T @ v` with the W that `apply()` uses and `interpolate()`
        returns (the `+ neumann_ws[row]` of interpolator.pyx:618 included), on the device.  `values`: one node array (n_points,)
        or k of them as (k, n_points); returns cell values shaped like `values` with n_elems in place of n_points.  Each cell
        sums its nodes' terms in ascending node id (scipy's order), without atomics: results are bitwise reproducible."""
        self._check_call(method, variable)
        g = self.grid
        v = np.ascontiguousarray(values, dtype=DTYPE_F)
        if v.shape != (g.n_points,) and not (v.ndim == 2 and v.shape[0] >= 1 and v.shape[1] == g.n_points):
            raise ValueError(f"values must have shape ({g.n_points},) or (k, {g.n_points}), not {v.shape}.")
        if g.device < 0:
            g.to_device(self.device)
        _upload_fields(g, method, self.cells_data, self.points_data, self.variable_to_index, variable)
        k = 1 if v.ndim == 1 else v.shape[0]
        out = np.empty(g.n_elems if v.ndim == 1 else (k, g.n_elems), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_apply_transpose_fields_host(g._h, _lib.METHOD_ID[method], _ptr(v), k, _ptr(out)))
        return out

    def _derivative_inputs(self, variable, lead_shape, cell_values, beside):
        """(u, k) of a derivative call: `cell_values` as a contiguous float64 array of shape lead_shape + (n_elems,) -- default: the cell
        variable `variable` itself, for each of the k = 1 or lead_shape[0] leading entries -- where lead_shape () or (k,) is that of the
        caller's own array, which `beside` names in the ValueError (None: there is none, and one field only)."""
        E = self.grid.n_elems
        k = lead_shape[0] if lead_shape else 1
        if cell_values is None:
            u = np.asarray(self.cells_data[self.variable_to_index["cells"][variable]])[:E]
            return np.ascontiguousarray(np.broadcast_to(u, (k, E)) if beside else u, dtype=DTYPE_F), k
        u = np.ascontiguousarray(cell_values, dtype=DTYPE_F)
        if u.shape != tuple(lead_shape) + (E,):
            raise ValueError(f"cell_values must have shape {tuple(lead_shape) + (E,)} beside {beside}, not {u.shape}." if beside else
                             f"cell_values must have shape ({E},), not {u.shape}.")
        return u, k

    def _gls_tables_to_device(self, variable):
        """the grid on the device with the GLS tables of `variable`: the last step before a derivative's native call"""
        if self.grid.device < 0:
            self.grid.to_device(self.device)
        _upload_fields(self.grid, "gls", self.cells_data, self.points_data, self.variable_to_index, variable)

    def permeability_gradient(self, variable, node_values, cell_values=None):
        """The derivative of `<v, W u>` with respect to the permeability, for the GLS matrix W that `apply(variable, "gls")` uses (the
        `+ neumann_ws[row]` included): `node_values` = v, one node array (n_points,) or k of them as (k, n_points); `cell_values` = u,
        shaped alike with n_elems (default: the cell variable `variable` itself, for every v).  Returns (n_elems, 3, 3): the gradient
        with respect to the resident permeability table, the chain through diff_mag = (1 - 3 / tr K)^2 folded in.  On the device, the
        sibling of apply_transpose(): host-synchronous, numpy in and out; deterministic.  Nodes whose row is zero (Dirichlet nodes)
        contribute nothing; the Neumann values are not differentiated (the node coordinates: points_gradient())."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        v = np.ascontiguousarray(node_values, dtype=DTYPE_F)
        if v.shape != (g.n_points,) and not (v.ndim == 2 and v.shape[0] >= 1 and v.shape[1] == g.n_points):
            raise ValueError(f"node_values must have shape ({g.n_points},) or (k, {g.n_points}), not {v.shape}.")
        u, k = self._derivative_inputs(variable, v.shape[:-1], cell_values, f"node_values of shape {v.shape}")
        self._gls_tables_to_device(variable)
        out = np.empty((g.n_elems, 3, 3), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_permeability_gradient_host(g._h, _ptr(v), _ptr(u), k, _ptr(out)))
        return out

    def points_gradient(self, variable, node_values, cell_values=None):
        """The derivative of `<v, W u>` with respect to the node coordinates, for the GLS matrix W that `apply(variable, "gls")` uses
        (the `+ neumann_ws[row]` included): `node_values` = v, one node array (n_points,) or k of them as (k, n_points);
        `cell_values` = u, shaped alike with n_elems (default: the cell variable `variable` itself, for every v).  Returns
        (n_points, 3): the gradient with respect to the grid's resident coordinates -- what update_points() rewrites -- at the
        resident permeability and flags; the float32 casts of the stored normals count as the identity.  On the device, the sibling
        of permeability_gradient(): host-synchronous, numpy in and out; deterministic.  Nodes whose row is zero (Dirichlet nodes)
        contribute nothing but receive gradient as vertices of their cells and faces.  3-D meshes, GLS only; the Neumann values are
        not differentiated."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        v = np.ascontiguousarray(node_values, dtype=DTYPE_F)
        if v.shape != (g.n_points,) and not (v.ndim == 2 and v.shape[0] >= 1 and v.shape[1] == g.n_points):
            raise ValueError(f"node_values must have shape ({g.n_points},) or (k, {g.n_points}), not {v.shape}.")
        u, k = self._derivative_inputs(variable, v.shape[:-1], cell_values, f"node_values of shape {v.shape}")
        self._gls_tables_to_device(variable)
        out = np.empty((g.n_points, 3), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_points_gradient_host(g._h, _ptr(v), _ptr(u), k, _ptr(out)))
        return out

    def permeability_tangent(self, variable, dK, cell_values=None):
        """The directional derivative of what `apply(variable, "gls")` returns, along a change `dK` of the permeability: `dK` one
        direction (n_elems, 3, 3) or k of them as (k, n_elems, 3, 3); `cell_values` = u, (n_elems,) or (k, n_elems) alike (default: the
        cell variable `variable` itself, for every direction).  Returns `(d_node_values, d_neumann_ws)`, each (n_points,) or
        (k, n_points): `dW_f . u_f` for the GLS matrix W that apply() uses (the `+ neumann_ws[row]` included) and the derivative of its
        neumann_ws, at the resident permeability table, the chain through diff_mag = (1 - 3 / tr K)^2 folded in.  On the device, the
        sibling of permeability_gradient(): host-synchronous, numpy in and out; deterministic.  It is what a Newton-Krylov solver with
        K(u) needs, `J . v` without differencing two weight launches.  Rows that are zero (Dirichlet nodes) have a zero derivative; the
        Neumann values are not differentiated (the node coordinates: points_tangent())."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        d = np.ascontiguousarray(dK, dtype=DTYPE_F)
        if d.shape != (g.n_elems, 3, 3) and not (d.ndim == 4 and d.shape[0] >= 1 and d.shape[1:] == (g.n_elems, 3, 3)):
            raise ValueError(f"dK must have shape ({g.n_elems}, 3, 3) or (k, {g.n_elems}, 3, 3), not {d.shape}.")
        lead = d.shape[:-3]
        u, k = self._derivative_inputs(variable, lead, cell_values, f"dK of shape {d.shape}")
        self._gls_tables_to_device(variable)
        out = np.empty(lead + (g.n_points,), dtype=DTYPE_F)
        nws = np.empty(lead + (g.n_points,), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_permeability_tangent_host(g._h, _ptr(d), _ptr(u), k, _ptr(out), _ptr(nws)))
        return out, nws

    def points_tangent(self, variable, dX, cell_values=None):
        """The directional derivative of what `apply(variable, "gls")` returns, along a change `dX` of the node coordinates: `dX` one
        direction (n_points, 3) or k of them as (k, n_points, 3); `cell_values` = u, (n_elems,) or (k, n_elems) alike (default: the
        cell variable `variable` itself, for every direction).  Returns `(d_node_values, d_neumann_ws)`, each (n_points,) or
        (k, n_points): `dW_f . u_f` for the GLS matrix W that apply() uses (the `+ neumann_ws[row]` included) and the derivative of its
        neumann_ws, at the grid's resident coordinates -- what update_points() rewrites -- permeability and flags; the float32 casts of
        the stored normals count as the identity.  On the device, the sibling of permeability_tangent() and the forward mode of
        points_gradient(): host-synchronous, numpy in and out; deterministic.  It is what a solver that moves the mesh needs, `J . dX`
        without differencing two update_points() + apply() pairs.  Rows that are zero (Dirichlet nodes) have a zero derivative, but
        moving a Dirichlet node moves the rows of its neighbours.  3-D meshes, GLS only; the Neumann values are not differentiated."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        d = np.ascontiguousarray(dX, dtype=DTYPE_F)
        if d.shape != (g.n_points, 3) and not (d.ndim == 3 and d.shape[0] >= 1 and d.shape[1:] == (g.n_points, 3)):
            raise ValueError(f"dX must have shape ({g.n_points}, 3) or (k, {g.n_points}, 3), not {d.shape}.")
        lead = d.shape[:-2]
        u, k = self._derivative_inputs(variable, lead, cell_values, f"dX of shape {d.shape}")
        self._gls_tables_to_device(variable)
        out = np.empty(lead + (g.n_points,), dtype=DTYPE_F)
        nws = np.empty(lead + (g.n_points,), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_points_tangent_host(g._h, _ptr(d), _ptr(u), k, _ptr(out), _ptr(nws)))
        return out, nws

    def _corner_gradient_inputs(self, variable, values):
        """(u, k, lead) of corner_gradients() / node_gradient(): `values` as apply() takes them, the GLS tables on the device"""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        if values is None:
            values = np.asarray(self.cells_data[self.variable_to_index["cells"][variable]])[:g.n_elems]
        u = np.ascontiguousarray(values, dtype=DTYPE_F)
        if u.shape != (g.n_elems,) and not (u.ndim == 2 and u.shape[0] >= 1 and u.shape[1] == g.n_elems):
            raise ValueError(f"values must have shape ({g.n_elems},) or (k, {g.n_elems}), not {u.shape}.")
        self._gls_tables_to_device(variable)
        return u, (1 if u.ndim == 1 else u.shape[0]), u.shape[:-1]

    def corner_gradients(self, variable, values=None, flux=False):
        """The gradients of the GLS reconstruction in the cells around every node: per node the least-squares system whose last
        unknown `apply(variable, "gls")` keeps as the node value has a gradient for each of the node's cells as its other unknowns,
        continuous in flux and in the tangential derivative across the faces.  `values` as in apply(): one cell array (n_elems,) --
        default: the cell variable `variable` itself -- or k of them as (k, n_elems).  Returns grad, (nnz_esup, 3) or (k, nnz_esup, 3) in
        esup order; with flux=True (grad, flux), flux = -K_e grad with the resident permeability, shaped alike.
        Indexing: grad[grid.esup_ptr[p]:grid.esup_ptr[p + 1]] are the gradients node p gives its cells grid.esup[that range].
        The face rows of the right-hand side are zero (Neumann rows too); rows that are zero in W (Dirichlet nodes) are zeros here.
        On the device, host-synchronous, numpy in and out; deterministic.  3-D meshes, GLS only."""
        u, k, lead = self._corner_gradient_inputs(variable, values)
        g = self.grid
        nnz = int(g.nnz_esup)
        grad = np.empty(lead + (nnz, 3), dtype=DTYPE_F)
        fl = np.empty(lead + (nnz, 3), dtype=DTYPE_F) if flux else None
        _lib.check(_lib.load().nin_gls_corner_gradients_host(g._h, _ptr(u), k, _ptr(grad), None, _ptr(fl), None))
        return (grad, fl) if flux else grad

    def node_gradient(self, variable, values=None):
        """One gradient per node: the mean of the node's corner gradients (corner_gradients()) in row order, zeros on zero rows --
        an average for visualisation, not a projection.  `values` as there; returns (n_points, 3) or (k, n_points, 3)."""
        u, k, lead = self._corner_gradient_inputs(variable, values)
        g = self.grid
        grad = np.empty(lead + (int(g.nnz_esup), 3), dtype=DTYPE_F)
        out = np.empty(lead + (g.n_points, 3), dtype=DTYPE_F)
        _lib.check(_lib.load().nin_gls_corner_gradients_host(g._h, _ptr(u), k, _ptr(grad), None, None, _ptr(out)))
        return out

    def gradient_operator(self, variable):
        """The map from a cell field to what `corner_gradients(variable, field)` returns, factorised ONCE at the grid's resident
        coordinates, permeability and flags and kept on the device: a scipy LinearOperator of shape (3 nnz_esup, n_elems), float64
        (GradientOperator: `matvec` = the corner gradients of a cell field, flattened (nnz_esup, 3); `rmatvec` = the transpose, which
        corner_gradients() does not have; `matmat` / `rmatmat` batched in one launch each; `to_scipy()` the explicit csr_matrix, the
        gradient stencil dg/du of an implicit flux scheme; `update()`; `release()`).  corner_gradients() assembles and factorises every
        node at every call; this does so once and every product afterwards streams the kept buffer (24 sum_p ne_p^2 bytes on the
        device, 15.4 GB at 216^3 hexahedra).  The operator depends on all three inputs: after a later update_permeability(),
        update_points() or update_neumann_flags() the products raise (NinpolError, a RuntimeError) until `update()` factorises again.
        The face rows of the right-hand side are zero, as in corner_gradients().  3-D meshes, GLS only.  Host-synchronous, numpy in
        and out."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        self._gls_tables_to_device(variable)
        op = GlsGradientOperator(self.grid)
        _lib.check(_lib.load().nin_gls_gradop_factorize_host(op._handle()))
        return GradientOperator(op, self, variable)

    def permeability_jacobian(self, variable, cell_values=None, neumann_values=None, basis=None):
        """The Jacobian of what `apply(variable, "gls")` returns, `W u` (+ `neumann_ws * neumann_values` when those are given), with
        respect to the permeability table, linearised ONCE at the resident table and kept on the device: a scipy LinearOperator of
        shape (n_points, 9 n_elems), float64 (PermeabilityJacobian: `matvec` = J . dK for a flattened (n_elems, 3, 3) direction,
        `rmatvec` = J^T . v, `matmat` / `rmatmat` batched in one launch each, `to_scipy()` the explicit csr_matrix, `release()`).
        `cell_values` = u (n_elems,), default the cell variable `variable` itself; `neumann_values` = b (n_points,) or None.  The chain
        through diff_mag = (1 - 3 / tr K)^2 is folded in.  The sibling of permeability_gradient() / permeability_tangent() for a Krylov
        solver: those factorise every node at every call, this does so once (the cost of one permeability_gradient) and every product
        afterwards streams the kept buffer (80 bytes per entry of esup, on the device).  Later update_*() calls do not change the
        operator; build a new one at the new point, or -- after local updates (`cells=`, `nodes=`, Grid.mark_dirty) -- call its
        `update()`, which recomputes only the rows of the grid's dirty nodes.  Host-synchronous, numpy in and out.

        `basis`: the permeability moves along M = 1, 3 or 6 parameters per cell, perm_e = sum_m theta_(e,m) B_(e,m), and
        the result is the Jacobian in theta instead: a ReducedPermeabilityJacobian of shape (n_points, M n_elems), column M e + m,
        kept in 8 M bytes per entry of esup (the 80-byte buffer is never made).  "scale": B = the resident permeability itself (M = 1,
        theta a log-multiplier); "diagonal": e_d e_d^T (M = 3); "symmetric": xx, yy, zz, xy, xz, yz with the off-diagonals e_i e_j^T +
        e_j e_i^T (M = 6); or a float64 ndarray (n_elems, M, 9), (n_elems, M, 3, 3) per cell, (M, 9) or (M, 3, 3) shared."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        if basis is not None:
            M, B, per_cell = reduced_basis(basis, g.n_elems)
        u, _ = self._derivative_inputs(variable, (), cell_values, None)
        b = None
        if neumann_values is not None:
            b = np.ascontiguousarray(neumann_values, dtype=DTYPE_F)
            if b.shape != (g.n_points,):
                raise ValueError(f"neumann_values must have shape ({g.n_points},), not {b.shape}.")
        self._gls_tables_to_device(variable)
        if basis is not None:
            rjac = GlsReducedJacobian(g, M)
            _lib.check(_lib.load().nin_gls_rjacobian_linearize_host(rjac._handle(), _ptr(u), _ptr(b), _ptr(B), int(per_cell)))
            return UpdatableReducedPermeabilityJacobian(rjac)._bind(self, variable, (B, per_cell))
        jac = GlsJacobian(g)
        _lib.check(_lib.load().nin_gls_jacobian_linearize_host(jac._handle(), _ptr(u), _ptr(b)))
        return UpdatablePermeabilityJacobian(jac)._bind(self, variable)

    def points_jacobian(self, variable, cell_values=None, neumann_values=None):
        """The Jacobian of what `apply(variable, "gls")` returns, `W u` (+ `neumann_ws * neumann_values` when those are given), with
        respect to the node coordinates, linearised ONCE at the grid's resident coordinates -- what update_points() rewrites --
        permeability and flags, and kept on the device: a scipy LinearOperator of shape (n_points, 3 n_points), float64
        (PointsJacobian: `matvec` = J . dX for a flattened (n_points, 3) direction, `rmatvec` = J^T . v, `matmat` / `rmatmat` batched in
        one launch each, `release()`).  `cell_values` = u (n_elems,), default the cell variable `variable` itself; `neumann_values` = b
        (n_points,) or None.  The sibling of points_gradient() / points_tangent() for a Krylov solver on a moving mesh: those factorise
        every node at every call, this does so once (the cost of one points_gradient) and every product afterwards streams the kept
        records (24 bytes per entry of esup, 48 per entry of fsup, 24 per node, on the device).  The Jacobian is kept factored through
        the mesh geometry; `assemble()` builds the explicit csr_matrix from it with kernels on the device -- not a
        `to_scipy()`, which elsewhere is a host-side reshape that cannot fail.  The products and `assemble()` read the resident
        coordinates, so after a later update_points() they raise (NinpolError, a RuntimeError): build a new operator at the new point, or after
        update_points(nodes=) call its `update()`, which recomputes only the moved neighbourhood; updates of the
        permeability or the flags do not change the operator.  3-D meshes, GLS only; the Neumann values are not differentiated.
        Host-synchronous, numpy in and out."""
        self._check_call(variable=variable)
        self._perm_rows()   # (ValueError without a permeability)
        g = self.grid
        u, _ = self._derivative_inputs(variable, (), cell_values, None)
        b = None
        if neumann_values is not None:
            b = np.ascontiguousarray(neumann_values, dtype=DTYPE_F)
            if b.shape != (g.n_points,):
                raise ValueError(f"neumann_values must have shape ({g.n_points},), not {b.shape}.")
        self._gls_tables_to_device(variable)
        jac = GlsShapeJacobian(g)
        _lib.check(_lib.load().nin_gls_xjacobian_linearize_host(jac._handle(), _ptr(u), _ptr(b)))
        return PointsJacobian(jac)._bind(self, variable)

    def release_scratch(self, pinned=True):
        """Give back what the object keeps between calls for speed: the grid's device scratch (weights, compacted
        triplets: ~2.3 GB of HBM at 10 M cells; the transpose index of apply_transpose(): 0.69 GB more) and, with pinned=True, the idle page-locked result buffers of the
        process-wide pool.  Results already returned stay valid."""
        if self.grid is not None:
            self.grid.release_scratch()
        if pinned:
            _pinned.trim(0)

    def device_plan(self, variable, method):
        """Upload the fields of (variable, method) and return a DevicePlan (kernel-only launches)."""
        return DevicePlan(self, variable, method)

    def prepare_interpolator(self, method, variable, target_points):
        """interpolator.pyx:631-670: dense (n_target, MX_ELEMENTS_PER_POINT) weights + neumann_ws."""
        target_points = np.asarray(target_points, dtype=DTYPE_I)
        weights = np.zeros((len(target_points), self.grid.MX_ELEMENTS_PER_POINT), dtype=DTYPE_F)
        neumann_ws = np.zeros(len(target_points), dtype=DTYPE_F)
        self.supported_methods[method](self.grid, self.cells_data, self.points_data, self.faces_data,
                                       self.variable_to_index, variable, target_points, weights, neumann_ws)
        return weights, neumann_ws


class DevicePlan:
    """Device-resident form of one `interpolate(variable, method)`: the field rows are uploaded by `refresh()` (once at
    construction) and every `launch` is just the kernel, asynchronous on the caller's HIP stream, writing into the
    caller's device buffers (e.g. torch tensors): csr_data [nnz_esup] float64, neumann_ws [n_points] float64.  This is
    what bench.py times and what the multi-GPU path feeds to its exchange.

    The Neumann flags and the permeability on the device belong to the grid, not to the plan: a launch first checks that
    the grid's resident flags are still this plan's variable (another plan, or interpolate() on another variable, may
    have replaced them) and re-uploads if not; `refresh()` re-reads the caller's tables unconditionally -- an in-place
    edit of a table is only seen there, exactly as Interpolator.interpolate() sees it on every call.

    The geometry belongs to the grid too: after Interpolator.update_points() the next `launch` computes the weights of the moved
    mesh (no refresh() is needed for that; what an earlier launch wrote into the caller's buffers stays what it was).

    So does a permeability that changes on the device: after Interpolator.update_permeability() with device tensors the next
    `launch` on the same stream computes with the new K -- `launch` never re-reads a table, so a time loop of update_permeability(K_dev)
    and launch(...) touches no host memory and never synchronises.  `refresh()` leaves that K resident as long as the contents of the
    host table are what they were (the precedence rule of update_permeability).

    And so do Neumann flags that change on the device: Interpolator.update_neumann_flags() with device tensors rewrites the grid's flags
    and marks the nodes whose bit changed; launch_dirty() recomputes those rows.  After a whole-array update for ANOTHER variable the
    grid holds that variable's flags: a plan of the first variable re-uploads its own at its next launch (ensure_current)."""

    def __init__(self, interp, variable, method):
        interp._check_call(method)
        self.interp = interp
        self.variable = variable
        self.grid = g = interp.grid
        # the tables of THIS mesh (advisor, round 3): a later load_mesh() on the Interpolator replaces interp.grid and its tables;
        # this plan goes on serving the grid it was made for, with the rows it was made from (in-place edits are still seen)
        self._cells_data, self._points_data, self._v2i = interp.cells_data, interp.points_data, interp.variable_to_index
        self._device = interp.device
        self.method = method
        self.method_id = _lib.METHOD_ID[method]
        L = _lib.load()
        self.refresh()
        P = g.n_points
        self.nnz = int(L.nin_grid_scalar(g._h, b"nnz_esup"))
        self.n_points = P
        self.n_elems = g.n_elems
        self.algorithmic_bytes = int(L.nin_algorithmic_bytes(g._h, self.method_id))
        self.kernel_name = L.nin_kernel_name(self.method_id).decode()

    def refresh(self):
        """Upload this plan's field rows from the Interpolator's tables as they are NOW (flags always; permeability and
        diff_mag when their contents changed: a hash of all their bytes)."""
        _upload_fields(self.grid, self.method, self._cells_data, self._points_data, self._v2i, self.variable,
                       device=self._device, always_perm=True)

    def ensure_current(self):
        if self.grid._fields_variable != self.variable:
            self.refresh()

    def any_neumann_flag(self):
        """Does any node carry neumann_flag_<variable>?  (neumann_ws is identically zero otherwise.)  It reads the HOST row: after
        Interpolator.update_neumann_flags() with device tensors it answers for the host row until fetch_neumann_flags()."""
        row = self._v2i["points"]["neumann_flag_" + self.variable]
        return bool(np.any(np.asarray(self._points_data)[row][:self.n_points].astype(np.int64) != 0))

    def launch(self, csr_data_ptr, neumann_ws_ptr, stream=0, add_neumann=True):
        self.ensure_current()
        _lib.check(_lib.load().nin_weights_device(self.grid._h, self.method_id, None, 0, int(bool(add_neumann)),
                                                  ctypes.c_void_p(csr_data_ptr), ctypes.c_void_p(neumann_ws_ptr),
                                                  ctypes.c_void_p(stream)))

    def launch_dirty(self, csr_data_ptr, neumann_ws_ptr, stream=0, add_neumann=True, clear=True):
        """Recompute, IN PLACE, the rows of the grid's dirty nodes only (nin_weights_dirty_device) -- after
        Interpolator.update_permeability(cells=...) the vertices of the rewritten cells -- and return how many that were.  If the
        buffers held a full result as of the last clear (Grid.clear_dirty() after a full launch(), or an earlier launch_dirty with
        clear=True), they hold afterwards what launch() would write now, bit for bit; no other row is touched.  The call reads 128
        bytes back (how many nodes each kernel gets) and so waits for `stream` once; everything else is asynchronous on it.
        clear=False keeps the set (a second buffer follows).  While every node is dirty (Grid.dirty_nodes == -1) this is launch().
        Raises if cell or node ids outside the mesh were scattered since the last call (update_permeability(cells=), update_points(nodes=),
        update_neumann_flags(nodes=)): nothing is launched, the set is kept, and the next call goes through."""
        self.ensure_current()
        n = ctypes.c_int64(0)
        _lib.check(_lib.load().nin_weights_dirty_device(self.grid._h, self.method_id, int(bool(add_neumann)), ctypes.c_void_p(csr_data_ptr),
                                                        ctypes.c_void_p(neumann_ws_ptr), ctypes.c_void_p(stream), int(bool(clear)),
                                                        ctypes.byref(n)))
        return int(n.value)

    def host_matrix(self, stream=0):
        """The matrix of Interpolator.interpolate(variable, method) on the host, kept current by this plan: a HostMatrix.  A full run
        now (host-synchronous on `stream`) into buffers the HostMatrix owns; its update() then recomputes, transfers and patches only
        the grid's dirty rows.  Clears the grid's dirty set -- one consumer per grid, the contract of launch_dirty(clear=True)."""
        return HostMatrix(self, stream)

    def launch_apply(self, u_cells_ptr, n_fields, node_values_ptr, neumann_ws_ptr, stream=0):
        """W . u on the device for n_fields cell fields (nin_apply_device): u [n_fields][n_elems] ->
        node_values [n_fields][n_points], weights computed once; asynchronous on `stream`."""
        self.ensure_current()
        _lib.check(_lib.load().nin_apply_device(self.grid._h, self.method_id, ctypes.c_void_p(u_cells_ptr), int(n_fields),
                                                ctypes.c_void_p(node_values_ptr), ctypes.c_void_p(neumann_ws_ptr),
                                                ctypes.c_void_p(stream)))

    def launch_spmv(self, weights_ptr, u_ptr, n_fields, values_ptr, stream=0):
        """W . u on weights the caller holds (nin_spmv_device): weights [nnz_esup] as `launch(..., add_neumann=True)` writes
        them, u [n_fields][n_elems] -> values [n_fields][n_points]; no weight kernel runs; asynchronous on `stream`."""
        _lib.check(_lib.load().nin_spmv_device(self.grid._h, ctypes.c_void_p(weights_ptr), ctypes.c_void_p(u_ptr), int(n_fields),
                                               ctypes.c_void_p(values_ptr), ctypes.c_void_p(stream)))

    def launch_spmv_transpose(self, weights_ptr, values_ptr, n_fields, cells_ptr, stream=0):
        """W^T . v on the same weights (nin_spmv_transpose_device): values [n_fields][n_points] -> cells [n_fields][n_elems];
        asynchronous on `stream` (the first call on a grid builds the transpose index and synchronises)."""
        _lib.check(_lib.load().nin_spmv_transpose_device(self.grid._h, ctypes.c_void_p(weights_ptr), ctypes.c_void_p(values_ptr),
                                                         int(n_fields), ctypes.c_void_p(cells_ptr), ctypes.c_void_p(stream)))


    def launch_sddmm(self, u_ptr, values_ptr, n_fields, grad_csr_ptr, stream=0):
        """The sampled product (nin_sddmm_device): grad_csr[pos] = sum_f values[f][p] * u[f][esup[pos]] over the entries of every row p
        -- the gradient of <values, W u> with respect to weights in esup position; u [n_fields][n_elems], values
        [n_fields][n_points], grad_csr [nnz_esup]; asynchronous on `stream`."""
        _lib.check(_lib.load().nin_sddmm_device(self.grid._h, ctypes.c_void_p(u_ptr), ctypes.c_void_p(values_ptr), int(n_fields),
                                                ctypes.c_void_p(grad_csr_ptr), ctypes.c_void_p(stream)))

    def _gls_derivative(self, name, why="do not depend on the permeability", current=True):
        """what the derivative launches begin with: GLS only -- a plan of another method raises, it does not return zeros -- and the
        tables current (a linearisation leaves that to the object's relinearize, after its own argument checks)"""
        if self.method != "gls":
            raise ValueError(f"the weights of '{self.method}' {why}: {name} is GLS only")
        if current:
            self.ensure_current()

    def launch_weights_backward(self, grad_csr_ptr, grad_perm_ptr, grad_diff_mag_ptr=0, grad_neumann_ws_ptr=0, stream=0, add_neumann=True):
        """The GLS weights differentiated with respect to the permeability (nin_gls_weights_backward_device): grad_csr [nnz_esup] =
        dL/d csr_data of a `launch(..., add_neumann)` (grad_neumann_ws [n_points] = dL/d neumann_ws, 0: none) -> grad_perm
        [n_elems][9] = dL/dK at what is resident now.  With grad_diff_mag [n_elems] the table's diff_mag counts as an independent
        input and gets its own gradient; with 0 its chain is folded into grad_perm.  Asynchronous on `stream` after the first call on
        a grid (which makes the bins and buffers -- 80 bytes per entry of esup -- and synchronises).  Only GLS depends on K."""
        self._gls_derivative("launch_weights_backward")
        _lib.check(_lib.load().nin_gls_weights_backward_device(self.grid._h, int(bool(add_neumann)), _vp(grad_csr_ptr), _vp(grad_neumann_ws_ptr),
                                                               _vp(grad_perm_ptr), _vp(grad_diff_mag_ptr), ctypes.c_void_p(stream)))

    def launch_weights_backward_points(self, grad_csr_ptr, grad_points_ptr, grad_neumann_ws_ptr=0, stream=0, add_neumann=True):
        """The GLS weights differentiated with respect to the node coordinates (nin_gls_weights_backward_points_device): grad_csr
        [nnz_esup] = dL/d csr_data of a `launch(..., add_neumann)` (grad_neumann_ws [n_points] = dL/d neumann_ws, 0: none) ->
        grad_points [n_points][3] = dL/d point_coords at what is resident now (geometry, flags, K): a shape adjoint, the sibling of
        launch_weights_backward.  Every node gets its gradient, Dirichlet nodes too (as vertices of their cells and faces).
        Asynchronous on `stream` after the first call on a grid (which makes the bins and buffers -- 24 bytes per entry of esup, 48 per
        entry of fsup, 96 per face -- and synchronises); deterministic.  3-D grids.  GLS only: the IDW and LS weights depend on the
        coordinates too, but their derivative is not provided -- a plan of those methods raises instead of returning zeros."""
        self._gls_derivative("launch_weights_backward_points", "do depend on the node coordinates, but they are not differentiated here")
        _lib.check(_lib.load().nin_gls_weights_backward_points_device(self.grid._h, int(bool(add_neumann)), _vp(grad_csr_ptr),
                                                                      _vp(grad_neumann_ws_ptr), _vp(grad_points_ptr), ctypes.c_void_p(stream)))

    def launch_weights_tangent(self, tangent_perm_ptr, tangent_csr_ptr, n_tangents=1, tangent_diff_mag_ptr=0, tangent_neumann_ws_ptr=0, stream=0,
                               add_neumann=True):
        """The directional derivative of the GLS weights in the permeability (nin_gls_weights_tangent_device): tangent_perm
        [n_tangents][n_elems][9] = the directions dK -> tangent_csr [n_tangents][nnz_esup] = (d csr_data / dK) . dK for the csr_data of a
        `launch(..., add_neumann)` at what is resident now, and tangent_neumann_ws [n_tangents][n_points] (0: not wanted) the same for
        neumann_ws.  With tangent_diff_mag [n_tangents][n_elems] the table's diff_mag counts as an independent input with its own
        direction; with 0 its chain is folded from the resident K.  All directions share one factorisation per node.  Every entry of
        the outputs is written.  Asynchronous on `stream` after the first call on a grid (which makes the bins and synchronises); no
        contribution buffer is allocated.  Only GLS depends on K."""
        self._gls_derivative("launch_weights_tangent")
        _lib.check(_lib.load().nin_gls_weights_tangent_device(self.grid._h, int(bool(add_neumann)), int(n_tangents), _vp(tangent_perm_ptr),
                                                              _vp(tangent_diff_mag_ptr), _vp(tangent_csr_ptr), _vp(tangent_neumann_ws_ptr),
                                                              ctypes.c_void_p(stream)))

    def launch_weights_tangent_points(self, tangent_points_ptr, tangent_csr_ptr, n_tangents=1, tangent_neumann_ws_ptr=0, stream=0, add_neumann=True):
        """The directional derivative of the GLS weights in the node coordinates (nin_gls_weights_tangent_points_device):
        tangent_points [n_tangents][n_points][3] = the directions dX -> tangent_csr [n_tangents][nnz_esup] = (d csr_data / dX) . dX for the
        csr_data of a `launch(..., add_neumann)` at what is resident now (geometry, flags, K), and tangent_neumann_ws
        [n_tangents][n_points] (0: not wanted) the same for neumann_ws: a shape tangent, the sibling of launch_weights_tangent and the
        forward mode of launch_weights_backward_points.  All directions share one factorisation per node.  Every entry of the outputs
        is written.  Asynchronous on `stream` after the first call on a grid (which makes the bins and synchronises); the grid keeps
        24 bytes per cell and 48 per face, per direction, grown to the largest n_tangents seen -- none of the adjoints' buffers.  3-D
        grids.  GLS only: a plan of IDW or LS raises instead of returning zeros."""
        self._gls_derivative("launch_weights_tangent_points", "do depend on the node coordinates, but they are not differentiated here")
        _lib.check(_lib.load().nin_gls_weights_tangent_points_device(self.grid._h, int(bool(add_neumann)), int(n_tangents), _vp(tangent_points_ptr),
                                                                     _vp(tangent_csr_ptr), _vp(tangent_neumann_ws_ptr), ctypes.c_void_p(stream)))

    def launch_corner_gradients(self, u_ptr, grad_ptr, n_fields=1, node_values_ptr=0, flux_ptr=0, node_gradient_ptr=0, stream=0):
        """The corner gradients of the GLS reconstruction (nin_gls_corner_gradients_device): u [n_fields][n_elems] -> grad
        [n_fields][nnz_esup][3], the gradient in cell esup[pos] as the node whose row holds pos reconstructs it -- the other 3 ne
        unknowns of the least-squares system whose last unknown the weights keep -- at what is resident now (geometry, flags, K).
        Optional (0: not wanted): node_values [n_fields][n_points] = sum_i w_i u_i with the weights of add_neumann=False; flux
        [n_fields][nnz_esup][3] = -K_e grad; node_gradient [n_fields][n_points][3] = the mean of a node's corner gradients in row
        order (an average for visualisation, not a projection).  The face rows of the right-hand side are zero, Neumann rows too.
        All fields share one factorisation per node; every entry of every output is written, zeros where the row is zero.
        Asynchronous on `stream` after the first call on a grid (which makes the adjoint's bins and synchronises); deterministic.
        3-D grids.  GLS only: IDW and LS solve no such system -- a plan of those methods raises instead of returning zeros."""
        self._gls_derivative("launch_corner_gradients", "are not the solution of a system that has cell gradients")
        _lib.check(_lib.load().nin_gls_corner_gradients_device(self.grid._h, int(n_fields), _vp(u_ptr), _vp(grad_ptr), _vp(node_values_ptr),
                                                               _vp(flux_ptr), _vp(node_gradient_ptr), ctypes.c_void_p(stream)))

    def gradient_operator(self, stream=0):
        """The map u -> launch_corner_gradients(u), kept on the device: a GlsGradientOperator factorised at what is resident now
        (geometry, flags, K).  One launch of the adjoint kernel's gradient mode with the unit columns of every node as its fields;
        its launch_apply / launch_apply_transpose then stream 24 sum_p ne_p^2 bytes instead of factorising every node again, and the
        second is the transpose launch_corner_gradients does not have.  The object owns its buffers.  Its launches answer until the
        next update of the permeability, the points or the flags (then: its factorize()).  3-D grids.  GLS only: a plan of IDW or LS
        raises instead of returning zeros."""
        self._gls_derivative("gradient_operator", "are not the solution of a system that has cell gradients")
        op = GlsGradientOperator(self.grid, plan=self)
        op.factorize(stream)
        return op

    def linearize(self, u_ptr, neumann_values_ptr=0, stream=0):
        """The Jacobian of the node values `W u + neumann_ws * b` in the permeability, kept on the device: a GlsJacobian linearised at
        what is resident now, for the cell field u [n_elems] (and node values b [n_points], 0: none), both device pointers.  One launch
        of the adjoint kernel (the cost of one launch_weights_backward); its launch_jvp / launch_vjp then stream 80 bytes per entry of
        esup instead of factorising every node again.  The object owns its buffers (80 bytes per entry of esup).  Only GLS depends on K."""
        self._gls_derivative("linearize", current=False)
        if not u_ptr:
            raise ValueError("u_ptr must be a device pointer to n_elems float64 values, not 0")
        J = GlsDirtyJacobian(self.grid, plan=self)
        J.relinearize(u_ptr, neumann_values_ptr, stream)
        return J

    def linearize_points(self, u_ptr, neumann_values_ptr=0, stream=0):
        """The Jacobian of the node values `W u + neumann_ws * b` in the node coordinates, kept on the device: a GlsShapeJacobian
        linearised at what is resident now (geometry, flags, K), for the cell field u [n_elems] (and node values b [n_points], 0:
        none), both device pointers.  One launch of the adjoint kernel's coordinate mode (the factorisations of one
        launch_weights_backward_points); its launch_jvp / launch_vjp then stream the kept records through the mesh geometry instead of
        factorising every node again.  The object owns its buffers (24 bytes per entry of esup, 48 per entry of fsup, 24 per node,
        plus the scratch of its launches); none of the grid's buffers of launch_weights_backward_points / launch_weights_tangent_points
        is made.  Its launches answer until the next update of the points.  3-D grids.  GLS only: a plan of IDW or LS raises instead
        of returning zeros."""
        self._gls_derivative("linearize_points", "do depend on the node coordinates, but they are not differentiated here", current=False)
        if not u_ptr:
            raise ValueError("u_ptr must be a device pointer to n_elems float64 values, not 0")
        J = GlsShapeJacobian(self.grid, plan=self)
        J.relinearize(u_ptr, neumann_values_ptr, stream)
        return J

    def linearize_reduced(self, u_ptr, n_params=1, basis_ptr=0, basis_per_cell=True, neumann_values_ptr=0, stream=0):
        """linearize() for a permeability that moves along n_params = 1, 3 or 6 parameters per cell, perm_e = sum_m theta_(e,m)
        B_(e,m): a GlsReducedJacobian, 8 n_params bytes per entry of esup, linearised at what is resident now.
        basis_ptr: device pointer to B [n_elems][n_params][9] (basis_per_cell) or [n_params][9] shared by every cell, read by this call
        only; 0 with n_params = 1: the resident permeability itself (theta a log-multiplier).  The adjoint kernel contracts with the
        basis where it has the ten values of a (node, cell) pair: the 80-byte buffer of linearize() is never written or allocated."""
        self._gls_derivative("linearize_reduced", current=False)
        if not u_ptr:
            raise ValueError("u_ptr must be a device pointer to n_elems float64 values, not 0")
        _check_n_params(n_params, basis_ptr)
        J = GlsDirtyReducedJacobian(self.grid, n_params, plan=self)
        J.relinearize(u_ptr, basis_ptr, basis_per_cell, neumann_values_ptr, stream)
        return J


class HostMatrix:
    """`W, neumann = Interpolator.interpolate(variable, method)` as an object that stays current: `M.W` (scipy csr_matrix, n_points x
    n_elems, int32 indices) and `M.neumann` (n_points,) in page-locked host memory.  After Interpolator.update_permeability(cells=),
    update_points(nodes=) or update_neumann_flags(nodes=) -- numpy or device arguments -- `M.update()` recomputes the grid's dirty rows on
    the device, brings only those rows over PCIe and patches them in; afterwards indptr, indices, data and neumann are bit for bit what
    interpolate() of a fresh load_mesh() of the mesh as it is now returns.

    Like DevicePlan.launch_dirty it computes from what is resident on the device (plan.refresh() re-reads the tables and makes every node
    dirty), and the dirty set is the grid's: one HostMatrix (or one launch_dirty consumer) per grid.  Its device buffers -- weights, neumann_ws
    and row counts -- are its own: interpolate() / apply() calls in between do not disturb it.  Made by DevicePlan.host_matrix()."""

    def __init__(self, plan, stream=0):
        g = plan.grid
        if max(g.nnz_esup, g.n_elems, g.n_points) >= np.iinfo(np.int32).max:
            raise ValueError("this mesh needs int64 indices: a HostMatrix holds int32 ones (use interpolate())")
        if plan.method == "gls" and g.dim == 2:
            import warnings
            warnings.warn("GLS on a 2-D mesh: the reference's result there is undefined (rank-deficient system); "
                          "values will not match ninpol's", RuntimeWarning, stacklevel=3)
        self.plan = plan
        self.W = self.neumann = None
        self.structure_changed = False
        self._h = None
        self._full(stream)
        self.structure_changed = False

    @staticmethod
    def _empty(n, dtype):
        return (np.empty if os.environ.get("NINPOL_AMD_NO_PINNED") else _pinned.empty)(n, dtype=dtype)

    def _full(self, stream):
        """every row: the full launch (unless update() has just run it) and the ordinary count / scan / compaction"""
        L = _lib.load()
        g = self.plan.grid
        P, E = g.n_points, g.n_elems
        self.plan.ensure_current()
        moved = self._h is None          # new buffers: whoever holds the old arrays keeps the old matrix
        if moved:
            h = ctypes.c_void_p()
            _lib.check(L.nin_hostmatrix_create(g._h, self.plan.method_id, ctypes.byref(h)))
            self._h = h
            self._indices, self._data = self._empty(g.nnz_esup, np.int32), self._empty(g.nnz_esup, DTYPE_F)
            self.neumann = self._empty(P, DTYPE_F)
        indptr = self._empty(P + 1, np.int32)
        nnz = ctypes.c_int64(0)
        _lib.check(L.nin_hostmatrix_full(self._h, _ptr(indptr), _ptr(self._indices), _ptr(self._data), _ptr(self.neumann),
                                         ctypes.byref(nnz), ctypes.c_void_p(stream)))
        if not moved and np.array_equal(indptr, self.W.indptr):
            self.structure_changed = False      # same row lengths: the arrays of M.W were rewritten where they are
        else:
            self.W = _wrap_csr(self._data[:nnz.value], self._indices[:nnz.value], indptr, (P, E))
            self.structure_changed = True

    def update(self, clear=True, stream=0):
        """Bring M.W and M.neumann up to date with the grid's dirty rows and return how many rows that were (0: nothing was touched).
        `structure_changed` says what happened to the objects: False -- no dirty row's count of surviving entries changed, and indptr,
        indices, data were patched in place (the same arrays: references to M.W stay valid; indices are rewritten too, equal counts do not
        imply an equal pattern); True -- M.W is a new matrix over new arrays (a flag flipped to Dirichlet empties a row, for example); after a
        patch, arrays handed out before keep the old matrix (after a full run they share M's buffers and hold the new entries).  An entry survives when it is `!= 0.0` (NaNs stay, +-0 go), as in interpolate().
        While every node is dirty (Grid.dirty_nodes == -1: a whole-array update, plan.refresh() after an edit, the first call after
        release()) this is the full run, rewritten in place when the row lengths allow.  Host-synchronous on `stream`; `clear` as
        launch_dirty's.  Raises what launch_dirty raises if ids outside the mesh were scattered since the last call: M and the dirty set
        stay as they are, and the next update() goes through."""
        L = _lib.load()
        g = self.plan.grid
        if self._h is None:
            self._full(stream)
            return int(g.n_points)
        self.plan.ensure_current()
        n, changed, entries = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(L.nin_hostmatrix_update(self._h, int(bool(clear)), ctypes.c_void_p(stream), ctypes.byref(n), ctypes.byref(changed),
                                           ctypes.byref(entries)))
        if entries.value < 0:            # every node was dirty
            self._full(stream)
            return int(n.value)
        self.structure_changed = False
        if n.value == 0:
            return 0
        W = self.W
        if changed.value == 0:
            _lib.check(L.nin_hostmatrix_patch(self._h, _ptr(W.indptr), _ptr(self._indices), _ptr(self._data), _ptr(self.neumann),
                                              None, None, None))
            return int(n.value)
        P = g.n_points
        indptr = self._empty(P + 1, np.int32)
        indices, data = self._empty(g.nnz_esup, np.int32), self._empty(g.nnz_esup, DTYPE_F)
        _lib.check(L.nin_hostmatrix_patch(self._h, _ptr(W.indptr), _ptr(self._indices), _ptr(self._data), _ptr(self.neumann),
                                          _ptr(indptr), _ptr(indices), _ptr(data)))
        nnz = int(indptr[P])
        self._indices, self._data = indices, data
        self.W = _wrap_csr(data[:nnz], indices[:nnz], indptr, (P, g.n_elems))
        self.structure_changed = True
        return int(n.value)

    def release(self):
        """Give the device buffers and the page-locked staging back.  M.W and M.neumann stay valid as they are; the next update() allocates
        again and is a full run."""
        if self._h is not None:
            _lib.load().nin_hostmatrix_destroy(self._h)
            self._h = None
        self._indices = self._data = None

    def __del__(self):
        try:
            self.release()
        except Exception:       # interpreter shutdown
            pass
