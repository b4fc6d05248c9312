"""torch autograd for the interpolation operator: `CellToNode(interp, variable, method)(u)` is `W . u` on the device, and its
backward pass is `W^T . grad` (nin_spmv_device / nin_spmv_transpose_device), both on torch's current stream.

Not imported by `ninpol_amd/__init__.py`: importing the package loads nothing native and does not import torch.  This module
imports torch, and opens its device, before the native library loads ("A process that also uses a PyTorch-ROCm
wheel")."""
import torch

if torch.cuda.is_available():
    torch.cuda.init()

from .interpolator import DevicePlan  # noqa: E402  (after torch has the device)


class _CellToNodeFn(torch.autograd.Function):
    """u [k][n_elems] -> W u [k][n_points]; backward W^T g.  The weights travel with the graph: a later refresh() of the module
    does not change the gradient of an output computed before it."""

    @staticmethod
    def forward(ctx, u, op, weights):
        ctx.op, ctx.weights = op, weights
        return op._spmv(weights, u)

    @staticmethod
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ctx.op._spmv_transpose(ctx.weights, grad.contiguous()), None, None


class CellToNode(torch.nn.Module):
    """Cell fields -> node values through the nodal interpolation matrix W of `interp.interpolate(variable, method)` (with the
    `+ neumann_ws[row]` of the Neumann rows), differentiable in the cell values.

    The weights are computed once, at construction, into `weights` (float64 [nnz_esup], esup / CSR position) with `neumann_ws`
    (float64 [n_points]) beside them; `refresh()` re-reads the Interpolator's tables and computes them again -- an in-place edit of
    the permeability is seen there and only there (the contract of DevicePlan.refresh()).  The same holds for a moved mesh: after
    `interp.update_points(...)` the module goes on applying the weights of the old geometry until `refresh()`; nothing is
    recomputed behind the caller's back.  A permeability that lives on the device reaches the module through
    `interp.update_permeability(K_dev)` followed by `recompute_weights()`: the weight kernels run again on torch's current stream
    from whatever is resident -- geometry and permeability -- with no table re-read, no hash and no synchronisation.  Derivatives
    with respect to the permeability, the Neumann values or the node coordinates are not provided."""

    def __init__(self, interp, variable, method):
        super().__init__()
        self.device = torch.device("cuda", int(interp.device))
        torch.cuda.init()
        torch.empty(1, device=self.device)       # torch holds the device before the native library opens it
        self.plan = DevicePlan(interp, variable, method)
        self.n_points, self.n_elems = self.plan.n_points, self.plan.n_elems
        self.weights = self.neumann_ws = None
        self._compute_weights()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _compute_weights(self):
        w = torch.empty(self.plan.nnz, dtype=torch.float64, device=self.device)
        nws = torch.empty(self.n_points, dtype=torch.float64, device=self.device)
        self.plan.launch(w.data_ptr(), nws.data_ptr(), self._stream(), add_neumann=True)
        # new tensors, not an in-place update: outputs computed before a refresh() keep the weights of their forward pass
        self.weights, self.neumann_ws = w, nws

    def refresh(self):
        """Upload the Interpolator's field tables as they are now and recompute the weights, from the grid's geometry as it is now
        (on torch's current stream: behind an update_points() from a device tensor on the same stream)."""
        self.plan.refresh()
        self._compute_weights()

    def recompute_weights(self, dirty_only=False):
        """Compute the weights again from what is resident on the device NOW -- after interp.update_permeability() or
        update_points() with device tensors on the same stream -- without reading the Interpolator's tables (refresh() does that).
        Asynchronous on torch's current stream; outputs computed before keep the weights of their forward pass in backward.

        dirty_only=True: only the rows of the grid's dirty nodes (after interp.update_permeability(cells=...): the vertices of those
        cells; after interp.update_points(rows, nodes=...): the vertices of the cells around the moved nodes -- the same set serves
        both, and nothing here had to change for local mesh motion) are computed, into CLONES of `weights` / `neumann_ws` that then replace them (DevicePlan.launch_dirty: reads the sizes
        of its lists back, so it waits for the stream once), and the set is cleared.  While every node is dirty -- as it is until
        the first clear after the grid went to the device -- the call is a full launch; from then on only the marked rows run.  The
        set belongs to the grid: one module (or one DevicePlan buffer) per grid can be kept current this way."""
        if not dirty_only:
            return self._compute_weights()
        w, nws = self.weights.clone(), self.neumann_ws.clone()
        self.plan.launch_dirty(w.data_ptr(), nws.data_ptr(), self._stream(), add_neumann=True, clear=True)
        self.weights, self.neumann_ws = w, nws

    def _spmv(self, weights, u):
        k = 1 if u.dim() == 1 else u.shape[0]
        out = torch.empty((self.n_points,) if u.dim() == 1 else (k, self.n_points), dtype=torch.float64, device=self.device)
        self.plan.launch_spmv(weights.data_ptr(), u.data_ptr(), k, out.data_ptr(), self._stream())
        return out

    def _spmv_transpose(self, weights, v):
        k = 1 if v.dim() == 1 else v.shape[0]
        out = torch.empty((self.n_elems,) if v.dim() == 1 else (k, self.n_elems), dtype=torch.float64, device=self.device)
        self.plan.launch_spmv_transpose(weights.data_ptr(), v.data_ptr(), k, out.data_ptr(), self._stream())
        return out

    def forward(self, u):
        """u: float64 (n_elems,) or (k, n_elems) on the plan's device -> node values (n_points,) or (k, n_points)."""
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"u must be a torch.Tensor, not {type(u).__name__}")
        if u.dtype != torch.float64:
            raise TypeError(f"u must be float64, not {u.dtype} (no silent cast)")
        if u.device != self.device:
            raise ValueError(f"u must be on {self.device}, not {u.device}")
        if tuple(u.shape) != (self.n_elems,) and not (u.dim() == 2 and u.shape[0] >= 1 and u.shape[1] == self.n_elems):
            raise ValueError(f"u must have shape ({self.n_elems},) or (k, {self.n_elems}), not {tuple(u.shape)}")
        return _CellToNodeFn.apply(u.contiguous(), self, self.weights)
