"""torch autograd for the interpolation operator: `CellToNode(interp, variable, method)(u)` is `W . u` on the device, and its
backward pass is `W^T . grad` (nin_spmv_device / nin_spmv_transpose_device), both on torch's current stream.  `CellToNode(...)(u, K)`
also makes the GLS weights a function of the permeability tensor K: its backward pass returns dL/dK through the sampled product
(nin_sddmm_device) and the adjoint of the weight kernels (nin_gls_weights_backward_device).  Under torch.autograd.forward_ad (dual
tensors) the same call gives the forward derivative, W du + dW u, with dW from the tangent of the weight kernels
(nin_gls_weights_tangent_device); torch.func.jvp, which needs setup_context-style Functions, is not supported.
`CellToNode(...)(u, points=X)` makes the GLS weights a function of the node coordinates as well: the mesh moves to X
(Interpolator.update_points) and the backward pass returns dL/dX (nin_gls_weights_backward_points_device); under forward_ad a dual X
gives dW u along dX (nin_gls_weights_tangent_points_device).
`CellToNode.linearize(u, K, scale)` is for a caller that needs many such products at one point (a Krylov solver): it keeps the
Jacobian of W u in the permeability on the device (nin_gls_jacobian) and returns a Linearization whose jvp / vjp are plain tensor
methods, one streaming pass each instead of a factorisation of every node; with wrt="points" it keeps the Jacobian in the node
coordinates instead (nin_gls_xjacobian).

Not imported by `ninpol_amd/__init__.py`: importing the package loads nothing native and does not import torch.  This module
imports torch, and opens its device, before the native library loads ("A process that also uses a PyTorch-ROCm
wheel")."""
import numpy as np
import torch

if torch.cuda.is_available():
    torch.cuda.init()

from .interpolator import DevicePlan  # noqa: E402  (after torch has the device)


class _CellToNodeFn(torch.autograd.Function):
    """u [k][n_elems] -> W u [k][n_points]; backward W^T g for u and, when the weights themselves require a gradient (they are the
    output of _GlsWeightsFn), the sampled product g u^T on W's pattern for them.  The weights travel with the graph: a later
    refresh() of the module does not change the gradient of an output computed before it."""

    @staticmethod
    def forward(ctx, u, op, weights):
        ctx.op, ctx.weights = op, weights
        ctx.u = u if ctx.needs_input_grad[2] else None
        ctx.save_for_forward(u, weights)
        return op._spmv(weights, u)

    @staticmethod
    def jvp(ctx, du, _, dweights):
        """forward mode: d(W u) = W du + dW u, the second term when the weights carry a tangent (they are _GlsWeightsFn's output)"""
        u, weights = ctx.saved_tensors
        op = ctx.op
        out = None
        if du is not None:
            out = op._spmv(weights, du.contiguous())
        if dweights is not None:
            t = op._spmv(dweights.contiguous(), u)
            out = t if out is None else out + t
        return out

    @staticmethod
    def backward(ctx, grad):
        gu = gw = None
        if ctx.needs_input_grad[0]:
            gu = ctx.op._spmv_transpose(ctx.weights, grad.contiguous())
        if ctx.needs_input_grad[2]:
            gw = ctx.op._sddmm(ctx.u, grad.contiguous())
        return gu, None, gw


class _GlsWeightsFn(torch.autograd.Function):
    """K [n_elems][3][3] (or [n_elems][9]) or None, scale [n_elems] or None, points [n_points][3] or None -> the stored GLS weights
    [nnz_esup] and neumann_ws [n_points] of the permeability scale * K on the mesh moved to `points`: the points become the grid's
    resident coordinates (Interpolator.update_points), scale * K its resident table (Interpolator.update_permeability); None leaves
    what is resident.  Backward reads what is resident -- geometry, flags, permeability -- so it refuses to run once any of them was
    updated after the forward pass: it would differentiate at another point."""

    @staticmethod
    def forward(ctx, K, scale, op, points=None):
        if points is not None:
            op.plan.interp.update_points(points.detach())
        if K is not None:
            op.plan.interp.update_permeability(K.detach(), None if scale is None else scale.detach())
        w, nws = op._launch_weights()
        ctx.op, ctx.stamp = op, op._stamp()
        ctx.save_for_backward(K, scale)
        ctx.save_for_forward(K, scale)
        ctx.set_materialize_grads(False)
        return w, nws

    @staticmethod
    def _check_stamp(ctx, what, call):
        now = ctx.op._stamp()
        if now != ctx.stamp:
            names = ("field_updates", "geometry_updates", "flag_updates")
            moved = ", ".join(f"{n} {a} -> {b}" for n, a, b in zip(names, ctx.stamp, now) if a != b)
            raise RuntimeError("the grid's resident permeability, geometry or Neumann flags were updated after the forward pass "
                               f"({moved}): the {what} with respect to K would be taken at another point.  Run {call} before "
                               "the next update, or the forward pass again.")

    @staticmethod
    def jvp(ctx, dK, dscale, _=None, dpoints=None):
        """forward mode (torch.autograd.forward_ad): the tangent of perm = scale * K is scale * dK + dscale * K, a missing tangent
        counts as zero; one DevicePlan.launch_weights_tangent call gives (dW, dneumann_ws).  A tangent of the node coordinates adds
        one DevicePlan.launch_weights_tangent_points call; the two results are summed.  Autograd calls this right behind forward();
        like backward() it reads what is resident and refuses once that was updated."""
        K, scale = ctx.saved_tensors
        op = ctx.op
        _GlsWeightsFn._check_stamp(ctx, "tangent", "jvp()")
        E = op.n_elems
        tperm = None
        if dK is not None:
            tperm = dK.reshape(E, 9) if scale is None else dK.reshape(E, 9) * scale[:, None]
        if dscale is not None and scale is not None:
            t = K.reshape(E, 9) * dscale[:, None]
            tperm = t if tperm is None else tperm + t
        dw = torch.empty(op.plan.nnz, dtype=torch.float64, device=op.device)
        dnws = torch.empty(op.n_points, dtype=torch.float64, device=op.device)
        if tperm is None and dpoints is None:
            return dw.zero_(), dnws.zero_()
        if tperm is not None:
            tperm = tperm.contiguous()
            op.plan.launch_weights_tangent(tperm.data_ptr(), dw.data_ptr(), 1, 0, dnws.data_ptr(), op._stream(), add_neumann=True)
            if dpoints is None:
                return dw, dnws
        if tperm is None:
            dwx, dnx = dw, dnws
        else:
            dwx, dnx = torch.empty_like(dw), torch.empty_like(dnws)
        dx = dpoints.contiguous()
        op.plan.launch_weights_tangent_points(dx.data_ptr(), dwx.data_ptr(), 1, dnx.data_ptr(), op._stream(), add_neumann=True)
        return (dw, dnws) if tperm is None else (dw + dwx, dnws + dnx)

    @staticmethod
    def backward(ctx, gw, gnws):
        K, scale = ctx.saved_tensors
        op = ctx.op
        want_perm, want_points = ctx.needs_input_grad[0] or ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if not (want_perm or want_points):
            return None, None, None, None
        _GlsWeightsFn._check_stamp(ctx, "gradient", "backward()")
        E = op.n_elems
        if gw is None:
            gw = torch.zeros(op.plan.nnz, dtype=torch.float64, device=op.device)
        gw = gw.contiguous()
        gnws = None if gnws is None else gnws.contiguous()
        gK = gscale = gpoints = None
        if want_perm:
            gperm = torch.empty((E, 9), dtype=torch.float64, device=op.device)
            op.plan.launch_weights_backward(gw.data_ptr(), gperm.data_ptr(), 0, 0 if gnws is None else gnws.data_ptr(), op._stream(),
                                            add_neumann=True)
            # perm = scale * K, entry by entry
            if ctx.needs_input_grad[0]:
                gK = (gperm if scale is None else gperm * scale[:, None]).reshape(K.shape)
            if scale is not None and ctx.needs_input_grad[1]:
                gscale = (K.reshape(E, 9) * gperm).sum(dim=1)
        if want_points:
            gpoints = torch.empty((op.n_points, 3), dtype=torch.float64, device=op.device)
            op.plan.launch_weights_backward_points(gw.data_ptr(), gpoints.data_ptr(), 0 if gnws is None else gnws.data_ptr(), op._stream(),
                                                   add_neumann=True)
        return gK, gscale, None, gpoints


class _ConstantWeightsFn(torch.autograd.Function):
    """IDW / LS: the weights do not depend on the permeability -- K and scale get zeros"""

    @staticmethod
    def forward(ctx, K, scale, weights):
        ctx.save_for_backward(K, scale)
        ctx.save_for_forward(weights)
        return weights.detach().clone()

    @staticmethod
    def jvp(ctx, dK, dscale, _):
        return torch.zeros_like(ctx.saved_tensors[0])

    @staticmethod
    def backward(ctx, gw):
        K, scale = ctx.saved_tensors
        return (torch.zeros_like(K) if ctx.needs_input_grad[0] else None,
                torch.zeros_like(scale) if scale is not None and ctx.needs_input_grad[1] else None, None)


class _GradientOperatorFn(torch.autograd.Function):
    """u [k][n_elems] -> G u [k][nnz_esup][3] (and the flux -K G u beside it) through a kept gradient operator; backward G^T of the
    cotangent, the flux's folded in first; linear in u, so the forward derivative is the function itself on du."""

    @staticmethod
    def forward(ctx, u, op, want_flux):
        ctx.op, ctx.want_flux = op, want_flux
        grad, flux = op._apply(u, want_flux)
        return (grad, flux) if want_flux else grad

    @staticmethod
    def jvp(ctx, du, _, __):
        grad, flux = ctx.op._apply(du.contiguous(), ctx.want_flux)
        return (grad, flux) if ctx.want_flux else grad

    @staticmethod
    def backward(ctx, ggrad, gflux=None):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ctx.op._apply_transpose(ctx.op.fold(ggrad, gflux)), None, None


class KeptGradients:
    """What CellToNode.gradient_operator() returns: `op(u, flux=False)` is the corner gradients of u -- float64 (nnz_esup, 3) or
    (k, nnz_esup, 3) in esup position, what CellToNode.corner_gradients(u) returns up to the rounding of another summation order -- from
    a GlsGradientOperator (`operator`) factorised once, and, unlike corner_gradients(), differentiable in u: backward() is the
    transposed product, and under torch.autograd.forward_ad the call is linear.  With flux=True it returns (grad, flux), flux = -K_e grad
    with the permeability resident at the factorisation; a cotangent fbar of the flux reaches u through
    `gbar[..., d] += -((K[0][d] fbar[0] + K[1][d] fbar[1]) + K[2][d] fbar[2])` (torch arithmetic, one rounding per operation) before the
    one transposed product.  Everything runs on torch's current stream.  After an update of the permeability, the points or the flags
    the call raises (NinpolError) until `factorize()`."""

    def __init__(self, module):
        self.module = module
        self.operator = module.plan.gradient_operator(module._stream())
        self._read_permeability()

    def _read_permeability(self):
        m = self.module
        g = m.plan.grid
        got = g.fetch_permeability()                    # (waits for the device: the factorisation is behind it)
        K = torch.from_numpy(got[0]).to(m.device)       # [E][9]
        self.K = K[torch.from_numpy(np.asarray(g.esup).astype(np.int64)).to(m.device)].reshape(-1, 3, 3)      # [nnz][3][3], row-major K_e per entry

    def factorize(self):
        """Factorise again at what is resident now (GlsGradientOperator.factorize) and read the permeability of the flux fold again."""
        self.operator.factorize(self.module._stream())
        self._read_permeability()

    def fold(self, ggrad, gflux):
        """the cotangent of G u from those of (grad, flux): ggrad + (-K^T gflux) per entry of esup, either may be None"""
        if gflux is None:
            return ggrad.contiguous()
        K, f = self.K, gflux
        back = torch.stack([-((K[:, 0, d] * f[..., 0] + K[:, 1, d] * f[..., 1]) + K[:, 2, d] * f[..., 2]) for d in range(3)], dim=-1)
        return (back if ggrad is None else ggrad + back).contiguous()

    def _apply(self, u, want_flux):
        m = self.module
        k = 1 if u.dim() == 1 else u.shape[0]
        shape = tuple(u.shape[:-1]) + (m.plan.nnz, 3)
        grad = torch.empty(shape, dtype=torch.float64, device=m.device)
        flux = torch.empty(shape, dtype=torch.float64, device=m.device) if want_flux else None
        self.operator.launch_apply(u.data_ptr(), grad.data_ptr(), k, flux.data_ptr() if want_flux else 0, 0, m._stream())
        return grad, flux

    def _apply_transpose(self, gbar):
        m = self.module
        k = 1 if gbar.dim() == 2 else gbar.shape[0]
        out = torch.empty(tuple(gbar.shape[:-2]) + (m.n_elems,), dtype=torch.float64, device=m.device)
        self.operator.launch_apply_transpose(gbar.data_ptr(), out.data_ptr(), k, m._stream())
        return out

    def __call__(self, u, flux=False):
        m = self.module
        m._check_cell_field(u)
        return _GradientOperatorFn.apply(u.contiguous(), self, bool(flux))


class Linearization:
    """CellToNode.linearize's result: `value` = W u at one permeability, with the weights (`weights`, `neumann_ws`), the resident
    Jacobian of W u (+ neumann_ws * neumann_values) in the permeability (`jacobian`: a GlsJacobian; None for IDW / LS, whose J is 0)
    and the K / scale it was taken at.  jvp() and vjp() are plain tensor methods on torch's current stream -- no autograd graph -- and
    cost one streaming pass each instead of a factorisation of every node: what a Krylov solver calls once per iteration.
    wrt="points": `jacobian` is a GlsShapeJacobian, the derivative in the node coordinates; jvp(du, dpoints=...) is
    W du + J dX and vjp(g) is (W^T g, J^T g).  Its products read the resident coordinates and raise (RuntimeError) once
    Interpolator.update_points() ran after the linearisation."""

    def __init__(self, op, u, weights, neumann_ws, jacobian, K, scale, wrt="K"):
        self.op, self.u, self.weights, self.neumann_ws, self.jacobian, self.K, self.scale = op, u, weights, neumann_ws, jacobian, K, scale
        # "scale": `jacobian` is a GlsReducedJacobian in the one parameter per cell, basis K; "points": a GlsShapeJacobian
        self.wrt = wrt
        self.value = op._spmv(weights, u)

    def _batch(self, t, name, shapes):
        """t as (k, ...) with its batch flag: one of `shapes` as it is, or with one leading batch dimension"""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.op.device:
            raise TypeError(f"{name} must be a float64 torch.Tensor on {self.op.device}")
        if tuple(t.shape) in shapes:
            return t.unsqueeze(0), False
        if t.dim() >= 2 and t.shape[0] >= 1 and tuple(t.shape[1:]) in shapes:
            return t, True
        raise ValueError(f"{name} must have shape {' or '.join(map(str, shapes))}, optionally with a leading batch dimension, "
                         f"not {tuple(t.shape)}")

    def jvp(self, du=None, dK=None, dscale=None, dpoints=None):
        """W du + J (scale * dK + dscale * K): the change of `value` along du (n_elems,), dK shaped like K and dscale (n_elems,), each
        optional, all with the same optional leading batch dimension.  Returns (n_points,) or (k, n_points).  A linearisation taken
        with wrt="scale" gives W du + R dscale from its (nnz_esup,) Jacobian, with no (n_elems, 9) temporary, and takes no dK.  One
        taken with wrt="points" gives W du + J dX for dpoints (n_points, 3) and takes neither dK nor dscale; the others take no
        dpoints."""
        op = self.op
        E, P = op.n_elems, op.n_points
        if self.wrt == "scale" and dK is not None:
            raise ValueError('a linearisation taken with wrt="scale" holds no derivative in K: dK must be None (take one with wrt="K")')
        if self.wrt == "points":
            for t, name in ((dK, "dK"), (dscale, "dscale")):
                if t is not None:
                    raise ValueError(f'a linearisation taken with wrt="points" holds no derivative in K: {name} must be None (take one with '
                                     'wrt="K")')
        elif dpoints is not None:
            raise ValueError(f'a linearisation taken with wrt="{self.wrt}" holds no derivative in the node coordinates: dpoints must be None '
                             '(take one with wrt="points")')
        if dscale is not None and (self.scale is None or self.K is None):
            raise ValueError("dscale needs a linearisation taken with K and scale")
        given = [(t, name, shapes) for t, name, shapes in ((du, "du", ((E,),)), (dK, "dK", ((E, 3, 3), (E, 9))), (dscale, "dscale", ((E,),)),
                                                           (dpoints, "dpoints", ((P, 3),)))
                 if t is not None]
        parts = {name: self._batch(t, name, shapes) for t, name, shapes in given}
        flags = {b for _, b in parts.values()}
        ks = {int(t.shape[0]) for t, _ in parts.values()}
        if len(flags) > 1 or len(ks) > 1:
            raise ValueError("du, dK, dscale and dpoints must share their leading batch dimension")
        batched, k = (flags.pop(), ks.pop()) if parts else (False, 1)
        out = None
        if du is not None:
            out = op._spmv(self.weights, parts["du"][0].contiguous())
        if self.wrt == "points":
            if dpoints is not None:
                dx = parts["dpoints"][0].contiguous()
                jv = torch.empty((k, P), dtype=torch.float64, device=op.device)
                self.jacobian.launch_jvp(dx.data_ptr(), jv.data_ptr(), k, op._stream())
                out = jv if out is None else out + jv
            if out is None:
                out = torch.zeros((k, P), dtype=torch.float64, device=op.device)
            return out if batched else out[0]
        if self.wrt == "scale":
            if dscale is not None and self.jacobian is not None:
                ds = parts["dscale"][0].contiguous()
                jv = torch.empty((k, P), dtype=torch.float64, device=op.device)
                self.jacobian.launch_jvp(ds.data_ptr(), jv.data_ptr(), k, op._stream())
                out = jv if out is None else out + jv
            if out is None:
                out = torch.zeros((k, P), dtype=torch.float64, device=op.device)
            return out if batched else out[0]
        tperm = None
        if dK is not None:
            tperm = parts["dK"][0].reshape(k, E, 9)
            if self.scale is not None:
                tperm = tperm * self.scale[None, :, None]
        if dscale is not None:
            t = self.K.reshape(1, E, 9) * parts["dscale"][0][:, :, None]
            tperm = t if tperm is None else tperm + t
        if tperm is not None and self.jacobian is not None:
            tperm = tperm.contiguous()
            jv = torch.empty((k, P), dtype=torch.float64, device=op.device)
            self.jacobian.launch_jvp(tperm.data_ptr(), jv.data_ptr(), k, 0, op._stream())
            out = jv if out is None else out + jv
        if out is None:
            out = torch.zeros((k, P), dtype=torch.float64, device=op.device)
        return out if batched else out[0]

    def vjp(self, g):
        """g (n_points,) or (k, n_points) -> (W^T g, scale * J^T g shaped like K, sum_k K * J^T g or None without a scale): the
        gradients of <g, value> in u, K and scale, what backward() of CellToNode(u, K, scale) returns.  A linearisation taken with
        wrt="points" returns (W^T g, J^T g shaped (n_points, 3)): the gradients in u and in the node coordinates, what backward() of
        CellToNode(u, points=X) returns."""
        op = self.op
        E = op.n_elems
        g, batched = self._batch(g, "g", ((op.n_points,),))
        g = g.contiguous()
        k = int(g.shape[0])
        gu = op._spmv_transpose(self.weights, g)
        if self.wrt == "points":
            gx = torch.empty((k, op.n_points, 3), dtype=torch.float64, device=op.device)
            self.jacobian.launch_vjp(g.data_ptr(), gx.data_ptr(), k, op._stream())
            return (gu, gx) if batched else (gu[0], gx[0])
        if self.wrt == "scale":      # (W^T g, None, R^T g): the gradient in scale straight from the reduced Jacobian
            if self.jacobian is not None:
                gscale = torch.empty((k, E), dtype=torch.float64, device=op.device)
                self.jacobian.launch_vjp(g.data_ptr(), gscale.data_ptr(), k, op._stream())
            else:
                gscale = torch.zeros((k, E), dtype=torch.float64, device=op.device)
            return (gu, None, gscale) if batched else (gu[0], None, gscale[0])
        if self.jacobian is not None:
            gperm = torch.empty((k, E, 9), dtype=torch.float64, device=op.device)
            self.jacobian.launch_vjp(g.data_ptr(), gperm.data_ptr(), k, 0, op._stream())
        else:
            gperm = torch.zeros((k, E, 9), dtype=torch.float64, device=op.device)
        kshape = (E, 3, 3) if self.K is None else tuple(self.K.shape)
        gK = (gperm if self.scale is None else gperm * self.scale[None, :, None]).reshape((k,) + kshape)
        gscale = None
        if self.scale is not None and self.K is not None:
            gscale = (self.K.reshape(1, E, 9) * gperm).sum(dim=2)
        if batched:
            return gu, gK, gscale
        return gu[0], gK[0], None if gscale is None else gscale[0]

    def assemble(self):
        """The Jacobian of a linearisation taken with wrt="points" as an explicit matrix: a torch.sparse_csr_tensor (n_points, 3
        n_points) on the plan's device, column 3 q + c = coordinate c of node q, sorted columns, explicit zeros kept.
        The pattern and the values go straight into tensors torch allocates, on torch's current stream; the pattern is made once per
        linearisation object and does not depend on the point.  Like jvp() it reads the resident coordinates and raises
        (RuntimeError) once Interpolator.update_points() ran after the linearisation.  Any other wrt: ValueError (K has to_scipy() on
        Interpolator.permeability_jacobian)."""
        if self.wrt != "points":
            raise ValueError(f'assemble() is for a linearisation taken with wrt="points", not wrt="{self.wrt}"')
        op = self.op
        P = op.n_points
        n_blocks = self.jacobian.pattern(op._stream())[0]
        block_ptr = torch.empty(P + 1, dtype=torch.int64, device=op.device)
        block_col = torch.empty(n_blocks, dtype=torch.int32, device=op.device)
        values = torch.empty((n_blocks, 3), dtype=torch.float64, device=op.device)
        self.jacobian.launch_pattern_copy(block_ptr.data_ptr(), block_col.data_ptr(), op._stream())
        self.jacobian.launch_assemble(values.data_ptr(), op._stream())
        col = (3 * block_col.to(torch.int64)[:, None] + torch.arange(3, dtype=torch.int64, device=op.device)).reshape(-1)
        return torch.sparse_csr_tensor(3 * block_ptr, col, values.reshape(-1), size=(P, 3 * P))

    def release(self):
        """give the Jacobian's device buffers back: jvp() / vjp() with a permeability direction raise afterwards"""
        if self.jacobian is not None:
            self.jacobian.release()


class CellToNode(torch.nn.Module):
    """Cell fields -> node values through the nodal interpolation matrix W of `interp.interpolate(variable, method)` (with the
    `+ neumann_ws[row]` of the Neumann rows), differentiable in the cell values.

    The weights are computed once, at construction, into `weights` (float64 [nnz_esup], esup / CSR position) with `neumann_ws`
    (float64 [n_points]) beside them; `refresh()` re-reads the Interpolator's tables and computes them again -- an in-place edit of
    the permeability is seen there and only there (the contract of DevicePlan.refresh()).  The same holds for a moved mesh: after
    `interp.update_points(...)` the module goes on applying the weights of the old geometry until `refresh()`; nothing is
    recomputed behind the caller's back.  A permeability that lives on the device reaches the module through
    `interp.update_permeability(K_dev)` followed by `recompute_weights()`: the weight kernels run again on torch's current stream
    from whatever is resident -- geometry and permeability -- with no table re-read, no hash and no synchronisation.

    The derivative with respect to the permeability comes through `forward(u, K, scale)` (GLS; see there) or `weights_of(K, scale)`,
    backwards (backward()) and forwards (torch.autograd.forward_ad: dual u, K, scale in any combination).  The derivative with
    respect to the node coordinates comes through `forward(u, points=...)` / `weights_of(points=...)`, backwards and forwards alike
    (GLS, 3-D; dual points beside dual u, K, scale in any combination).
    Derivatives with respect to the Neumann values are not provided, nor are those of the sharded (multi-GPU) path; the tangent is
    that of a full launch (recompute_weights(dirty_only=True) carries none)."""

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

    def _launch_weights(self):
        w = torch.empty(self.plan.nnz, dtype=torch.float64, device=self.device)
        nws = torch.empty(self.n_points, dtype=torch.float64, device=self.device)
        self.plan.launch(w.data_ptr(), nws.data_ptr(), self._stream(), add_neumann=True)
        return w, nws

    def _compute_weights(self):
        # new tensors, not an in-place update: outputs computed before a refresh() keep the weights of their forward pass
        self.weights, self.neumann_ws = self._launch_weights()

    def _stamp(self):
        g = self.plan.grid
        return (g.field_updates, g.geometry_updates, g.flag_updates)

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

    def _sddmm(self, u, v):
        k = 1 if u.dim() == 1 else u.shape[0]
        out = torch.empty(self.plan.nnz, dtype=torch.float64, device=self.device)
        self.plan.launch_sddmm(u.data_ptr(), v.data_ptr(), k, out.data_ptr(), self._stream())
        return out

    def weights_of(self, K=None, scale=None, points=None):
        """The stored weights [nnz_esup] (esup / CSR position, `+ neumann_ws[row]` included) and neumann_ws [n_points] as differentiable
        functions of the permeability: K float64 (n_elems, 3, 3) or (n_elems, 9) on the plan's device, optionally times the per-cell
        factor `scale` (n_elems,) -- the arguments, and the checks, of Interpolator.update_permeability with device tensors, which is
        what runs first: scale * K becomes the grid's resident permeability (the module's own `weights` stay what they were).  Fresh
        tensors on torch's current stream.  GLS: backward gives dL/dK = scale * dL/dperm and dL/dscale = sum(K * dL/dperm) through
        DevicePlan.launch_weights_backward, which reads the resident geometry, flags and permeability -- so backward raises
        RuntimeError if Grid.field_updates, geometry_updates or flag_updates moved after this call (another weights_of /
        forward(u, K) included): run each backward before the next update.  Under forward_ad.dual_level() dual K / scale give the
        weights' tangent along scale * dK + dscale * K through DevicePlan.launch_weights_tangent.  IDW / LS: the module's weights, and
        zeros for K.

        points: float64 (n_points, 3) on the plan's device, alone or beside K (3-D meshes, GLS) -- the weights as a differentiable
        function of the node coordinates.  It is given to Interpolator.update_points() first, as K is to update_permeability(): the
        mesh moves there.  Backward gives dL/dpoints through DevicePlan.launch_weights_backward_points, under the same rule about
        later updates; under forward_ad.dual_level() dual points give the weights' tangent along dX through
        DevicePlan.launch_weights_tangent_points, added to that of dual K / scale.  IDW / LS depend on the coordinates too, but that derivative is
        not provided: ValueError, never zeros."""
        if points is not None:
            if self.plan.method != "gls":
                raise ValueError(f"the weights of '{self.plan.method}' do depend on the node coordinates, but they are not differentiated "
                                 "here: points= is GLS only")
            if not isinstance(points, torch.Tensor) or points.dtype != torch.float64:
                raise TypeError(f"points must be a float64 torch.Tensor on {self.device} (no silent cast)")
            if points.device != self.device or tuple(points.shape) != (self.n_points, 3):
                raise ValueError(f"points must be on {self.device} with shape ({self.n_points}, 3), not {tuple(points.shape)} on {points.device}")
        if K is None:
            if scale is not None:
                raise ValueError("scale needs K")
            if points is None:
                raise ValueError("weights_of needs K or points")
            return _GlsWeightsFn.apply(None, None, self, points)
        if not isinstance(K, torch.Tensor):
            raise TypeError(f"K must be a torch.Tensor on {self.device}, not {type(K).__name__}")
        if K.device != self.device:
            raise ValueError(f"K must be on {self.device}, not {K.device}")
        if self.plan.method != "gls":
            for t, name, shapes in ((K, "K", ((self.n_elems, 3, 3), (self.n_elems, 9))), (scale, "scale", ((self.n_elems,),))):
                if t is None:
                    continue
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                    raise TypeError(f"{name} must be a float64 torch.Tensor (no silent cast)")
                if t.device != self.device or tuple(t.shape) not in shapes:
                    raise ValueError(f"{name} must be on {self.device} with shape {' or '.join(map(str, shapes))}")
            return _ConstantWeightsFn.apply(K, scale, self.weights), self.neumann_ws
        return _GlsWeightsFn.apply(K, scale, self, points)

    def linearize(self, u, K=None, scale=None, points=None, neumann_values=None, wrt="K"):
        """Linearise `forward(u, K, scale)` once, for many jvp / vjp products at that point: u float64 (n_elems,) on the plan's device
        (one field).  With K (and scale) it first does what weights_of does -- scale * K becomes the grid's resident permeability --
        and computes fresh weights; without, the weights of what is resident now.  Returns a Linearization: `value` = W u, `jvp(du, dK,
        dscale)`, `vjp(g)`, the weights and -- GLS -- the GlsJacobian of W u + neumann_ws * neumann_values ((n_points,) or None) in the
        permeability, resident on the device (80 bytes per entry of esup; the cost of one backward pass, once).  IDW / LS do not
        depend on K: no buffer is allocated and J counts as 0.  No autograd Function is involved: the methods are plain tensor calls
        on torch's current stream.

        wrt="scale" (needs K and scale): the permeability scale * K moves along the one parameter per cell only, d perm / d scale = K,
        and the Jacobian kept is the reduced one with the per-cell basis K (a GlsReducedJacobian, 8 bytes per entry of esup instead of
        80).  `jvp(du, dscale=...)` is then W du + R dscale with no (n_elems, 9) temporary and takes no dK; `vjp(g)` returns (W^T g,
        None, R^T g).

        points: float64 (n_points, 3) on the plan's device (3-D meshes, GLS) -- given to Interpolator.update_points() first, as in
        forward(): the mesh moves there and `value` is bit for bit what forward(u, K, scale, points) returns.  wrt="points": the
        Jacobian kept is the one in the node coordinates (a GlsShapeJacobian, DESIGN.md 4.18: 24 bytes per entry of esup, 48 per entry
        of fsup, 24 per node), `jvp(du, dpoints=...)` is W du + J dX and takes neither dK nor dscale, `vjp(g)` returns (W^T g, J^T g).
        Its products read the resident coordinates: after a later update_points() they raise RuntimeError -- linearise again.  IDW /
        LS depend on the coordinates too, but that derivative is not provided: ValueError, never zeros."""
        if wrt not in ("K", "scale", "points"):
            raise ValueError(f'wrt must be "K", "scale" or "points", not {wrt!r}')
        if wrt == "scale" and (K is None or scale is None):
            raise ValueError('wrt="scale" needs K and scale: the derivative is taken along scale at the permeability scale * K')
        if wrt == "points" and self.plan.method != "gls":
            raise ValueError(f"the weights of '{self.plan.method}' do depend on the node coordinates, but they are not differentiated "
                             'here: wrt="points" is GLS only')
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"u must be a torch.Tensor, not {type(u).__name__}")
        if u.dtype != torch.float64:
            raise TypeError(f"u must be float64, not {u.dtype} (no silent cast)")
        if tuple(u.shape) != (self.n_elems,):
            raise ValueError(f"u must have shape ({self.n_elems},): one field per linearisation, not {tuple(u.shape)}")
        if u.device != self.device:
            raise ValueError(f"u must be on {self.device}, not {u.device}")
        if neumann_values is not None:
            if not isinstance(neumann_values, torch.Tensor) or neumann_values.dtype != torch.float64:
                raise TypeError("neumann_values must be a float64 torch.Tensor (no silent cast)")
            if tuple(neumann_values.shape) != (self.n_points,) or neumann_values.device != self.device:
                raise ValueError(f"neumann_values must have shape ({self.n_points},) on {self.device}")
        if K is None and scale is not None:
            raise ValueError("scale needs K")
        u = u.detach().contiguous()
        if K is not None or points is not None:
            with torch.no_grad():      # (weights_of checks points, moves the mesh there and makes scale * K resident)
                weights, neumann_ws = self.weights_of(None if K is None else K.detach(), None if scale is None else scale.detach(),
                                                      None if points is None else points.detach())
            K, scale = None if K is None else K.detach(), None if scale is None else scale.detach()
        elif self.plan.method == "gls":
            weights, neumann_ws = self._launch_weights()
        else:
            weights, neumann_ws = self.weights, self.neumann_ws
        jac = None
        if self.plan.method == "gls":
            b = None if neumann_values is None else neumann_values.detach().contiguous()
            if wrt == "scale":
                basis = K.reshape(self.n_elems, 9).contiguous()       # read by the launch below only (stream-ordered)
                jac = self.plan.linearize_reduced(u.data_ptr(), 1, basis.data_ptr(), True, 0 if b is None else b.data_ptr(), self._stream())
            elif wrt == "points":
                jac = self.plan.linearize_points(u.data_ptr(), 0 if b is None else b.data_ptr(), self._stream())
            else:
                jac = self.plan.linearize(u.data_ptr(), 0 if b is None else b.data_ptr(), self._stream())
        return Linearization(self, u, weights, neumann_ws, jac, K, scale, wrt)

    def forward(self, u, K=None, scale=None, points=None):
        """u: float64 (n_elems,) or (k, n_elems) on the plan's device -> node values (n_points,) or (k, n_points).

        With K (and optionally scale; see weights_of): the weights are first computed from the permeability scale * K, and the
        result is differentiable in u, K and scale.  With points (see weights_of): the mesh is first moved there, and the result is
        differentiable in the node coordinates too.  Without either nothing changes: the module's weights are applied."""
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"u must be a torch.Tensor, not {type(u).__name__}")
        if u.dtype != torch.float64:
            raise TypeError(f"u must be float64, not {u.dtype} (no silent cast)")
        if u.device != self.device:
            raise ValueError(f"u must be on {self.device}, not {u.device}")
        if tuple(u.shape) != (self.n_elems,) and not (u.dim() == 2 and u.shape[0] >= 1 and u.shape[1] == self.n_elems):
            raise ValueError(f"u must have shape ({self.n_elems},) or (k, {self.n_elems}), not {tuple(u.shape)}")
        if K is None and points is None:
            if scale is not None:
                raise ValueError("scale needs K")
            return _CellToNodeFn.apply(u.contiguous(), self, self.weights)
        weights, _ = self.weights_of(K, scale, points)
        return _CellToNodeFn.apply(u.contiguous(), self, weights)

    def _check_cell_field(self, u):
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"u must be a torch.Tensor, not {type(u).__name__}")
        if u.dtype != torch.float64:
            raise TypeError(f"u must be float64, not {u.dtype} (no silent cast)")
        if u.device != self.device:
            raise ValueError(f"u must be on {self.device}, not {u.device}")
        if tuple(u.shape) != (self.n_elems,) and not (u.dim() == 2 and u.shape[0] >= 1 and u.shape[1] == self.n_elems):
            raise ValueError(f"u must have shape ({self.n_elems},) or (k, {self.n_elems}), not {tuple(u.shape)}")

    def gradient_operator(self):
        """The corner gradients as a kept, differentiable operator: a KeptGradients `op`, `op(u, flux=False)`,
        factorised once from what is resident on the device NOW.  Where corner_gradients(u) factorises every node at every call and
        carries no graph, `op(u)` streams the kept operator, its backward pass is the transposed product (the flux's cotangent
        folded in) and it works under torch.autograd.forward_ad.  GLS, 3-D; corner_gradients() itself is unchanged."""
        return KeptGradients(self)

    def corner_gradients(self, u):
        """u as in forward() -> the corner gradients of the GLS reconstruction (DevicePlan.launch_corner_gradients): float64
        (nnz_esup, 3) or (k, nnz_esup, 3) in esup position, from what is resident on the device NOW.  A plain tensor call on torch's
        current stream: NO autograd -- the result carries no graph even when u requires grad; differentiating through the gradients
        is not provided.  GLS, 3-D."""
        if not isinstance(u, torch.Tensor):
            raise TypeError(f"u must be a torch.Tensor, not {type(u).__name__}")
        if u.dtype != torch.float64:
            raise TypeError(f"u must be float64, not {u.dtype} (no silent cast)")
        if u.device != self.device:
            raise ValueError(f"u must be on {self.device}, not {u.device}")
        if tuple(u.shape) != (self.n_elems,) and not (u.dim() == 2 and u.shape[0] >= 1 and u.shape[1] == self.n_elems):
            raise ValueError(f"u must have shape ({self.n_elems},) or (k, {self.n_elems}), not {tuple(u.shape)}")
        u = u.detach().contiguous()
        k = 1 if u.dim() == 1 else u.shape[0]
        grad = torch.empty(tuple(u.shape[:-1]) + (self.plan.nnz, 3), dtype=torch.float64, device=self.device)
        self.plan.launch_corner_gradients(u.data_ptr(), grad.data_ptr(), k, stream=self._stream())
        return grad
