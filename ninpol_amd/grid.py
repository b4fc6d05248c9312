"""`Grid`: host mirror of the reference's `ninpol.Grid` (ninpol/_interpolator/grid.pyx, grid.pxd:128-187)
over the native builder in csrc/grid_host.cpp.  Same constructor arguments, same readonly attribute
names, same dtypes on the Python side (int64 / float64); the arrays themselves live in the C++
object as int32 and are converted on first access.
"""
import ctypes
import warnings

import numpy as np

from . import _lib
from . import topology as T
from ._args import is_torch, on_gpu

_SCALARS = ("dim", "n_elems", "n_points", "n_faces", "n_edges", "MX_ELEMENTS_PER_POINT",
            "MX_POINTS_PER_POINT", "MX_ELEMENTS_PER_FACE", "MX_FACES_PER_POINT")
_SHAPES = {"esuel": T.MAX_FACES_PER_ELEMENT, "infael": T.MAX_FACES_PER_ELEMENT, "inpofa": T.MAX_POINTS_PER_FACE,
           "inpoel": T.MAX_POINTS_PER_ELEMENT, "inedel": T.MAX_EDGES_PER_ELEMENT, "inpoed": 2,
           "centroids": 3, "faces_centers": 3, "normal_faces": 3, "point_coords": 3}
_ARRAYS = ("esup", "esup_ptr", "psup", "psup_ptr", "fsup", "fsup_ptr", "esuf", "esuf_ptr", "esuel", "infael",
           "inpofa", "inpoel", "inpoed", "inedel", "boundary_faces", "boundary_points", "point_coords",
           "centroids", "faces_centers", "normal_faces", "faces_areas", "element_types")


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev_ptr(t):
    """the address of a torch tensor's data (None stays None: an optional argument of the C entry point)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev_ids(t):
    """the three arguments of a C entry point that reads ids (int32 / int64) from the device: address, 64-bit?, how many"""
    return ctypes.c_void_p(t.data_ptr()), int(t.element_size() == 8), int(t.numel())


def _stream_of(t):
    """torch's current stream on the tensor's device: where the *_device methods of Grid launch"""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _PlanCounts(dict):
    """Nodes per kernel of the GLS launch plan; `plan["mfx"]` = the wide multifrontal kernel's five size classes together (interior
    nodes; its boundary nodes' list is `mfx_boundary`)."""

    def __missing__(self, key):
        if key == "mfx":
            return sum(v for k, v in self.items() if k.startswith("mfx_") and k != "mfx_boundary")
        raise KeyError(key)


class Grid:
    """Grid(dim, n_elems, n_points, npoel, nfael, lnofa, lpofa, nedel, lpoed, connectivity,
    element_types, logging=False, build_edges=False)  -- grid.pyx:47-53.

    Unlike the reference, the point coordinates are part of construction (`coords=`) and everything
    -- connectivity, centroids, normals -- is built in one native call; `build()`, `calculate_centroids()`,
    `calculate_normal_faces()` and `load_point_coords()` without an argument are therefore no-ops kept for
    call-compatibility.  `load_point_coords(coords)` moves the points of the built grid (a deforming mesh).
    """

    def __init__(self, dim, n_elems, n_points, npoel, nfael, lnofa, lpofa, nedel, lpoed, connectivity,
                 element_types, logging=False, build_edges=False, coords=None, num_threads=0, build_device=None):
        # grid.pyx:55-60
        if dim < 1:
            raise ValueError("The number of dimensions must be greater than 0.")
        if n_elems < 1:
            raise ValueError("The number of elements must be greater than 0.")
        if n_points < 1:
            raise ValueError("The number of points must be greater than 0.")
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        tabs = [i64(npoel), i64(nfael), i64(lnofa), i64(lpofa), i64(nedel), i64(lpoed)]
        expected = [(T.NUM_ELEMENT_TYPES,), (T.NUM_ELEMENT_TYPES,),
                    (T.NUM_ELEMENT_TYPES, T.MAX_FACES_PER_ELEMENT),
                    (T.NUM_ELEMENT_TYPES, T.MAX_FACES_PER_ELEMENT, T.MAX_POINTS_PER_FACE),
                    (T.NUM_ELEMENT_TYPES,), (T.NUM_ELEMENT_TYPES, T.MAX_EDGES_PER_ELEMENT, T.MAX_POINTS_PER_EDGE)]
        for a, shp in zip(tabs, expected):  # grid.pyx:80-101 _validate_shape
            if a.shape != shp:
                raise ValueError(f"The array must have shape {shp}, not {a.shape}.")
        conn = i64(connectivity)
        if conn.shape != (n_elems, T.MAX_POINTS_PER_ELEMENT):
            raise ValueError(f"The array must have shape {(n_elems, T.MAX_POINTS_PER_ELEMENT)}, not {conn.shape}.")
        etypes = i64(element_types)
        if coords is None:
            raise ValueError("The point coordinates have not been set.")
        xyz = np.ascontiguousarray(coords, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[0] != n_points or not 1 <= xyz.shape[1] <= 3:
            raise ValueError(f"coords must have shape ({n_points}, 1..3), not {xyz.shape}.")
        self.logging = bool(logging)
        self.build_edges = bool(build_edges)
        self._cache = {}
        self._no_fields_resident()
        self._h = ctypes.c_void_p()
        L = _lib.load()
        if build_device is None:   # the native OpenMP builder (csrc/grid_host.cpp)
            rc = L.nin_grid_create(int(dim), int(n_elems), int(n_points), *[_ptr(a) for a in tabs], _ptr(conn),
                                   _ptr(etypes), _ptr(xyz), int(xyz.shape[1]), int(bool(build_edges)),
                                   int(num_threads), ctypes.byref(self._h))
        else:                      # the same arrays built by HIP kernels on that GPU (csrc/grid_device.hip)
            rc = L.nin_grid_create_on_device(int(dim), int(n_elems), int(n_points), *[_ptr(a) for a in tabs], _ptr(conn),
                                             _ptr(etypes), _ptr(xyz), int(xyz.shape[1]), int(bool(build_edges)),
                                             int(build_device), ctypes.byref(self._h))
        if rc == _lib.NIN_EINVAL:
            raise ValueError(L.nin_last_error().decode())
        _lib.check(rc)
        self._coords_dim = int(xyz.shape[1])
        self.are_elements_loaded = True
        self.are_coords_loaded = True
        self.are_structures_built = True
        self.are_centroids_calculated = True
        self.are_normals_calculated = True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.load().nin_grid_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- reference method names, kept so reference-style call sequences run unchanged -------------
    def build(self):
        return None

    def load_point_coords(self, coords=None):
        """With coordinates: move the mesh (Interpolator.update_points does this).  `coords` has the shape the constructor saw,
        (n_points, coords_dim): a host array, or a torch tensor on the grid's device.  The connectivity, the GLS launch plan and
        everything else resident on the device stay; point_coords, centroids, faces_centers, normal_faces and faces_areas become
        what a fresh Grid of the moved mesh holds, bit for bit (nin_grid_update_points / nin_grid_update_points_device).  A host
        array is synchronous; a device tensor is asynchronous on torch's current stream and is not copied to the host.

        Without coordinates: a no-op, like build() (reference-style call sequences load the coordinates at construction here)."""
        if coords is None:
            return None
        L = _lib.load()
        shape = (int(self.n_points), self._coords_dim)
        if on_gpu(coords):
            import torch
            if tuple(coords.shape) != shape:
                raise ValueError(f"points must have shape {shape}, not {tuple(coords.shape)}.")
            if coords.dtype != torch.float64:
                raise ValueError(f"points on the device must be float64, not {coords.dtype}.")
            if self.device < 0 or coords.device.index != self.device:
                raise ValueError(f"points are on {coords.device}, the grid is on " +
                                 (f"cuda:{self.device}" if self.device >= 0 else "no device (call to_device first)") + ".")
            t = coords.detach().contiguous()
            rc = L.nin_grid_update_points_device(self._h, _dev_ptr(t), self._coords_dim, _stream_of(t))
        else:
            if is_torch(coords):
                coords = coords.detach().numpy()
            try:
                xyz = np.ascontiguousarray(coords, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"points cannot be converted to float64: {e}") from e
            if xyz.shape != shape:
                raise ValueError(f"points must have shape {shape}, not {xyz.shape}.")
            rc = L.nin_grid_update_points(self._h, _ptr(xyz), self._coords_dim)
        self._points_moved(rc)
        return None

    def _points_moved(self, rc):
        """behind a native call that moved points: the cached geometry goes, its return code is raised"""
        for name in ("point_coords", "centroids", "faces_centers", "normal_faces", "faces_areas"):
            self._cache.pop(name, None)   # also after a failure: the native arrays may be half way
        if rc == _lib.NIN_EINVAL:
            raise ValueError(_lib.load().nin_last_error().decode())
        _lib.check(rc)

    def scatter_point_coords(self, nodes, rows):
        """Move a subset of the nodes (nin_grid_scatter_points_device / nin_grid_scatter_points): row i of `rows` (m, coords_dim) float64 is
        the new position of node nodes[i].  torch tensors on the grid's device (nodes int32 / int64): asynchronous on torch's current
        stream, ids checked on the device.  numpy arrays (nodes int64, contiguous): synchronous, ids checked here (ValueError); on a grid
        without a device copy the host builder's geometry code runs.  On a device the geometry around the nodes is made again and the
        vertices of the cells around them join the dirty set.  The arguments are checked by Interpolator.update_points, which is the
        public way in."""
        L = _lib.load()
        if is_torch(rows):
            rc = L.nin_grid_scatter_points_device(self._h, *_dev_ids(nodes), _dev_ptr(rows), self._coords_dim, _stream_of(rows))
        else:
            rc = L.nin_grid_scatter_points(self._h, _ptr(nodes), int(len(nodes)), _ptr(rows), self._coords_dim)
        self._points_moved(rc)

    def calculate_centroids(self):
        return None

    def calculate_normal_faces(self):
        return None

    # -- attributes --------------------------------------------------------------------------------
    def _scalar(self, name):
        return int(_lib.load().nin_grid_scalar(self._h, name.encode()))

    def _array(self, name):
        if name in self._cache:
            return self._cache[name]
        L = _lib.load()
        n, dt = ctypes.c_int64(), ctypes.c_int()
        _lib.check(L.nin_grid_array_info(self._h, name.encode(), ctypes.byref(n), ctypes.byref(dt)))
        a = np.empty(n.value, dtype=np.float64 if dt.value == 1 else np.int64)
        _lib.check(L.nin_grid_array_copy(self._h, name.encode(), _ptr(a), n.value))
        if name in _SHAPES:
            a = a.reshape(-1, _SHAPES[name])
            if name == "point_coords" and self._coords_dim != 3:
                a = np.ascontiguousarray(a[:, :self._coords_dim])   # grid.pyx:666 keeps the caller's width
        self._cache[name] = a
        return a

    @property
    def nnz_esup(self):
        """len(esup) without bringing the array to the host (a device-built grid mirrors arrays lazily)."""
        return self._scalar("nnz_esup")

    def __getattr__(self, name):
        if name in _SCALARS:
            return self._scalar(name)
        if name in _ARRAYS:
            return self._array(name)
        raise AttributeError(name)

    def get_data(self):
        """grid.pyx:583-658, including its quirk: with build_edges=False the reference dies on
        `self.inpoed.copy()` of an empty (0, 0) view with this ValueError."""
        if not self.build_edges:
            raise ValueError("Invalid shape in axis 0: 0.")
        data = {k: getattr(self, k) for k in ("n_elems", "n_points", "n_faces", "n_edges", "MX_ELEMENTS_PER_POINT",
                                              "MX_POINTS_PER_POINT", "MX_ELEMENTS_PER_FACE", "MX_FACES_PER_POINT")}
        for k in ("point_coords", "centroids", "normal_faces", "faces_centers", "faces_areas", "boundary_faces",
                  "boundary_points", "inpoel", "element_types", "inpofa", "infael", "inpoed", "inedel"):
            data[k] = getattr(self, k).copy()

        def dense(ptr, idx, n_rows, width):
            out = -np.ones((n_rows, width), dtype=np.int64)
            cnt = np.diff(ptr)
            rows = np.repeat(np.arange(n_rows), cnt)
            cols = np.arange(len(idx)) - np.repeat(ptr[:-1], cnt)
            out[rows, cols] = idx
            return out
        data["esup"] = dense(self.esup_ptr, self.esup, self.n_points, self.MX_ELEMENTS_PER_POINT)
        data["psup"] = dense(self.psup_ptr, self.psup, self.n_points, self.MX_POINTS_PER_POINT)
        data["esuf"] = dense(self.esuf_ptr, self.esuf, self.n_faces, self.MX_ELEMENTS_PER_FACE)
        data["fsup"] = dense(self.fsup_ptr, self.fsup, self.n_points, self.MX_FACES_PER_POINT)
        return data

    # -- device ------------------------------------------------------------------------------------
    def to_device(self, device=0):
        self._no_fields_resident()
        _lib.check(_lib.load().nin_grid_to_device(self._h, int(device)))
        return self

    # -- whose are the fields resident on the device? ------------------------------------------------------------------------------------
    # The record is six fields.  Only the methods below assign them, each named for the event it records; the Interpolator reads them.
    #   _perm_key               fingerprint (interpolator.py: _perm_keys) of the host permeability / diff_mag rows as they were when the
    #                           resident table was last theirs, or was written over them; None: no permeability on this device copy yet
    #   _perm_from_device       the resident table was written from device memory and is newer than the host rows
    #                           (Interpolator.permeability_on_device)
    #   _perm_edited_last_call  interpolate() found the host table edited at its last call: the next one hashes before it launches
    #   _fields_variable        the variable whose Neumann flags are resident (DevicePlan.ensure_current); None: nobody's
    #   _flags_from_device      the resident flags were written from device memory and are newer than that variable's host row
    #                           (Interpolator.neumann_flags_on_device)
    #   _flags_key              only while _flags_from_device: the fingerprint of that host row at the first device update behind a host upload
    # The rule: a device copy stays until the CONTENTS of the host rows change; an in-place edit of the host rows wins at the next call
    # that reads the tables -- it is found there, by its fingerprint, and is then a host upload; another variable's flags make every node
    # dirty.  What each event does ("-": stays as it is):
    #
    #   permeability                                      method                       _perm_key        _perm_from_device
    #   new Grid, to_device()                             _no_fields_resident          None             False    (_perm_edited_last_call too)
    #   host upload                                       host_permeability_resident   the rows'        False
    #   whole-table device update, device scatter         permeability_from_device     - (the rows'     True
    #                                                                                    if it was None)
    #   host rows patched in step (the device followed)   host_permeability_resident   the rows'        False (it was)
    #   host rows edited (the device did not follow)      host_permeability_edited     -                False
    #   fetch                                             host_permeability_resident   the rows'        False
    #   interpolate() compared the fingerprints           permeability_edit_seen       -                -        (_perm_edited_last_call)
    #
    #   Neumann flags                                     method                       _fields_variable _flags_from_device  _flags_key
    #   new Grid, to_device()                             _no_fields_resident          None             False               None
    #   host upload: every call that reads the tables,    host_flags_uploaded          the variable     False               None
    #     unless a device copy is still current                                        (every node dirty if a device copy or another variable's flags went)
    #   whole-array device update (another variable's     flags_from_device            the variable     True                the row's, unless kept from
    #     too: the differing nodes are dirty), scatter                                                                      an earlier device update
    #   host row patched in step (the device followed)    (nothing to record: the row still is what is resident)
    #   host row edited (the device did not follow)       (nothing to record: found by its fingerprint, or uploaded anyway)
    #   fetch                                             flags_fetched                -                False               None
    #
    # Who records: the *_device methods further down only launch.  Their caller knows which event the launch was -- a device update, or
    # host values sent through the device path -- and records it afterwards, so a launch that raises records nothing.
    def _no_fields_resident(self):
        """a fresh device copy holds no fields and nobody's Neumann flags: every DevicePlan re-uploads at its next launch"""
        self._perm_key = self._fields_variable = self._flags_key = None
        self._perm_from_device = self._flags_from_device = self._perm_edited_last_call = False

    def host_permeability_resident(self, key):
        """the resident table IS the host rows (fingerprint `key`): they were uploaded, followed row by row, or fetched into"""
        self._perm_key, self._perm_from_device = key, False

    def host_permeability_edited(self):
        """the host rows are the newer ones now: the next call that reads the tables uploads them"""
        self._perm_from_device = False

    def permeability_from_device(self, fingerprint, *host_rows):
        """the resident table was written from device memory.  fingerprint(*host_rows) is only asked for when no permeability went to this
        device copy before: the host table then counts as seen from here on, or the next call would upload it over the device's K (its
        first hash finds nothing to compare with)"""
        if self._perm_key is None:
            self._perm_key = fingerprint(*host_rows)
        self._perm_from_device = True

    def permeability_edit_seen(self, edited):
        """interpolate() found the host table edited at this call (True) or still the resident one (False)"""
        self._perm_edited_last_call = edited

    def host_flags_uploaded(self, variable):
        """`variable`'s host row went over whatever flags were resident"""
        if self._flags_from_device or self._fields_variable not in (None, variable):
            self.mark_all_dirty()   # other flags: any row may differ from what a caller's buffers hold (DevicePlan.launch_dirty)
        self._fields_variable, self._flags_from_device, self._flags_key = variable, False, None

    def flags_from_device(self, variable, fingerprint, host_row):
        """the resident flags, now `variable`'s, were written from device memory.  fingerprint(host_row), of the variable's host row, is
        asked for at the FIRST device update behind a host upload, not at every step of a time loop: an in-place edit of the row made
        between two device updates is still found by the next call that reads the tables"""
        if not (self._flags_from_device and self._fields_variable == variable and self._flags_key is not None):
            self._flags_key = fingerprint(host_row)
        self._fields_variable, self._flags_from_device = variable, True

    def flags_fetched(self):
        """the resident flags were read back into the host row: the row IS what is resident"""
        self._flags_from_device, self._flags_key = False, None

    def load_permeability_device(self, K, scale=None):
        """The resident permeability from torch tensors on the grid's device (nin_fields_set_permeability_device): K float64,
        contiguous, n_elems * 9 values; scale None or float64 contiguous (n_elems,).  Asynchronous on torch's current stream; the
        arguments are checked by Interpolator.update_permeability, which is the public way in."""
        _lib.check(_lib.load().nin_fields_set_permeability_device(self._h, _dev_ptr(K), _dev_ptr(scale), _stream_of(K)))

    def scatter_permeability_device(self, cells, K, scale=None):
        """Rows of the resident permeability from torch tensors on the grid's device (nin_fields_scatter_permeability_device):
        cells int32 / int64 (m,), K float64 contiguous m * 9 values, scale None or float64 (m,).  The vertices of the cells join the
        dirty set.  Asynchronous on torch's current stream; the arguments are checked by Interpolator.update_permeability, which is
        the public way in."""
        _lib.check(_lib.load().nin_fields_scatter_permeability_device(self._h, *_dev_ids(cells), _dev_ptr(K), _dev_ptr(scale), _stream_of(K)))

    def load_flags_device(self, flags):
        """The resident Neumann flags from a torch tensor on the grid's device (nin_fields_set_flags_device): float64, bool or uint8,
        contiguous, (n_points,).  The nodes whose bit changes join the dirty set (none while every node is dirty).  Asynchronous on torch's
        current stream; the arguments are checked by Interpolator.update_neumann_flags, which is the public way in."""
        _lib.check(_lib.load().nin_fields_set_flags_device(self._h, _dev_ptr(flags), int(flags.element_size() == 1), _stream_of(flags)))

    def scatter_flags_device(self, nodes, flags):
        """Neumann flags of a subset of the nodes from torch tensors on the grid's device (nin_fields_scatter_flags_device): nodes int32 /
        int64 (m,), flags float64, bool or uint8 (m,), value i for node nodes[i].  Ids are checked on the device; the nodes whose bit changes
        join the dirty set.  Asynchronous on torch's current stream; the arguments are checked by Interpolator.update_neumann_flags, which
        is the public way in."""
        _lib.check(_lib.load().nin_fields_scatter_flags_device(self._h, *_dev_ids(nodes), _dev_ptr(flags), int(flags.element_size() == 1), _stream_of(flags)))

    def fetch_flags(self):
        """The Neumann bits resident on the device as a uint8 array (n_points,) of 0 / 1 (nin_fields_get_flags: waits for the device); None
        when the grid is on no device or holds no flags there."""
        if self.device < 0:
            return None
        out = np.empty(int(self.n_points), dtype=np.uint8)
        rc = _lib.load().nin_fields_get_flags(self._h, _ptr(out))
        if rc == _lib.NIN_ESTATE:
            return None
        _lib.check(rc)
        return out

    @property
    def flag_updates(self):
        """How many times the Neumann flags of this grid's device copy were rewritten from device memory (0: never, or host-only)."""
        return int(_lib.load().nin_grid_flag_updates(self._h))

    @property
    def dirty_nodes(self):
        """How many nodes' weights may have moved since the last clear (nin_grid_dirty_nodes: waits for the device): the vertices of
        the cells that update_permeability(cells=...) rewrote and of the cells around the nodes that update_points(nodes=...) moved, and the
        nodes whose Neumann bit update_neumann_flags() changed.
        -1: every node -- after the grid went to the device, a full permeability update, a whole-mesh update_points(), or the Neumann
        flags of another variable uploaded from the host.  0 for a grid on no device.  A diagnostic: it
        waits for the whole device and so stalls every stream -- not for a time loop (launch_dirty returns its count)."""
        n = int(_lib.load().nin_grid_dirty_nodes(self._h))
        if n < -1:
            _lib.check(_lib.NIN_EHIP)
        return n

    def clear_dirty(self, stream=0):
        """Empty the dirty set: the caller's weight buffers hold a full result as of now (nin_grid_dirty_reset; asynchronous on
        `stream`).  DevicePlan.launch_dirty(clear=True) does the same behind its launch."""
        _lib.check(_lib.load().nin_grid_dirty_reset(self._h, 0, ctypes.c_void_p(stream)))

    def mark_all_dirty(self, stream=0):
        """Every node is dirty: the next DevicePlan.launch_dirty is a full launch."""
        _lib.check(_lib.load().nin_grid_dirty_reset(self._h, 1, ctypes.c_void_p(stream)))

    def mark_dirty(self, cells=None, nodes=None, stream=0):
        """Nodes join the dirty set without an update (nin_grid_mark_dirty_device): `nodes`, or the vertices of `cells` -- exactly one
        of the two -- for a cell field u (resp. node values b) that changed there while K, the points and the flags did not, so that a
        kept Jacobian's relinearize_dirty() recomputes those rows.  1-D integer ids.  A torch tensor (int32 / int64) on
        the grid's device: asynchronous on `stream` (0: torch's current stream), no host copy; ids are checked on the device -- one
        outside the mesh marks nothing, and the next dirty launch raises with the count.  A numpy array, a list or a CPU tensor: checked
        here (ValueError for an id outside the mesh), copied up and marked before the call returns (needs torch).  Counts in none of
        the update counters: `is_current()` of a kept Jacobian does not see it."""
        from . import _args
        if (cells is None) == (nodes is None):
            raise ValueError("mark_dirty takes exactly one of cells= and nodes=")
        ids, name, n = (cells, "cells", self.n_elems) if nodes is None else (nodes, "nodes", self.n_points)
        L = _lib.load()
        if self.device < 0:
            _lib.check(L.nin_grid_mark_dirty_device(self._h, None, 0, 0, int(nodes is None), None))     # (NIN_ENODEVICE, in the library's words)
        import torch
        on_host = not on_gpu(ids)
        if on_host:
            ids = torch.from_numpy(_args.host_ids(_args.to_host(ids), name, int(n))).to(torch.device("cuda", self.device))
        else:
            _args.device_ids(ids, name, self.device)
            ids = ids.detach().contiguous()
        s = ctypes.c_void_p(stream) if stream and not on_host else _stream_of(ids)     # (host ids: behind their copy, on torch's stream)
        _lib.check(L.nin_grid_mark_dirty_device(self._h, *_dev_ids(ids), int(nodes is None), s))
        if on_host:
            torch.cuda.current_stream(ids.device).synchronize()

    def fetch_permeability(self):
        """(permeability (n_elems, 9), diff_mag (n_elems,)) as resident on the device (nin_fields_get_permeability: waits for the
        device); None when the grid is on no device or holds no permeability there."""
        if self.device < 0:
            return None
        E = int(self.n_elems)
        perm, dmag = np.empty((E, 9), dtype=np.float64), np.empty(E, dtype=np.float64)
        rc = _lib.load().nin_fields_get_permeability(self._h, _ptr(perm), _ptr(dmag))
        if rc == _lib.NIN_ESTATE:
            return None
        _lib.check(rc)
        return perm, dmag

    @property
    def field_updates(self):
        """How many times the permeability of this grid's device copy was replaced from device memory (0: never, or host-only)."""
        return int(_lib.load().nin_grid_field_updates(self._h))

    @property
    def device(self):
        return int(_lib.load().nin_grid_device(self._h))

    @property
    def geometry_updates(self):
        """How many times load_point_coords() or scatter_point_coords() moved the device copy of this grid (0: never, or the grid is
        host-only)."""
        return int(_lib.load().nin_grid_geometry_updates(self._h))

    @property
    def has_transpose_index(self):
        """Is the cell-major index of apply_transpose() resident on the device?  (It survives a move of the points.)"""
        return bool(_lib.load().nin_grid_has_transpose_index(self._h))

    def release_scratch(self):
        """Free the device buffers interpolate() / apply() keep between calls (nin_grid_release_scratch: ~2.3 GB of HBM
        at 10 M cells; the connectivity copies of load_point_coords(): ~1 GB more); the next call allocates them again."""
        _lib.check(_lib.load().nin_grid_release_scratch(self._h))

    ADJOINT_BINS = ("lds1", "lds2", "lds4", "global")

    def gls_adjoint_plan(self):
        """Nodes per bin of the GLS adjoint kernel on the device copy (nin_gls_adjoint_plan): the LDS classes of one, two and four
        wavefronts per node, then the systems kept in global-memory scratch.  Makes the bins if they are not there yet."""
        counts = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.load().nin_gls_adjoint_plan(self._h, counts.ctypes.data_as(ctypes.c_void_p)))
        return dict(zip(self.ADJOINT_BINS, counts.tolist()))

    PLAN_KERNELS = ("block1", "block2", "block4", "block8", "scratch", "hex8", "mfw_large", "mfw_small", "mfw_general", "small4", "small8",
                    "small12", "quad4", "mfx_6x10", "mfx_7x11", "mfx_8x13", "mfx_9x15", "mfx_10x16", "mfx_boundary", "mfg_tiles", "mfx_4x7", "mfx_7x12")

    def gls_plan_flops(self):
        """Per kernel of the GLS launch plan (nin_gls_plan_flops): {kernel: (algorithmic flops, reference-equivalent dgels flops,
        nodes computed)} for one launch over all nodes; needs the fields on the device (a DevicePlan or an interpolate() first)."""
        alg, ref, comp = np.zeros(22), np.zeros(22), np.zeros(22, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _lib.check(_lib.load().nin_gls_plan_flops(self._h, p(alg), p(ref), p(comp)))
        return {k: (float(alg[i]), float(ref[i]), int(comp[i])) for i, k in enumerate(self.PLAN_KERNELS)}

    def gls_plan(self):
        """Nodes per GLS kernel of the device copy (nin_gls_plan): block kernel classes 1 / 2 / 4 / 8 wavefronts per
        node and global scratch, the cube-node kernel, the one-wavefront multifrontal kernel (two-coloured nodes large / small, general kind), the one-wavefront dense
        kernel for small nodes (at most 4 / 8 / 12 cells), the two-lanes-per-node kernel for the nodes inside a boundary
        face of a hexahedron mesh, the wide one-wavefront multifrontal kernel (interior nodes of unstructured meshes)."""
        counts = np.zeros(22, dtype=np.int64)
        _lib.check(_lib.load().nin_gls_plan(self._h, counts.ctypes.data_as(ctypes.c_void_p)))
        return _PlanCounts(zip(self.PLAN_KERNELS, counts.tolist()))
