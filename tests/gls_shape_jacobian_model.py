"""A numpy model of the GLS Jacobian in the node coordinates: the two products of the kept object, as glue over the
models of the shape tangent (tests/gls_shape_tangent_model.py) and the shape adjoint (tests/gls_shape_model.py).

For a fixed cell field u and optional node values b the node values are  F_p(X) = sum_i d_i(X) u[c_i] + nws_p(X) b_p  with d the stored
weights of a launch with add_neumann = 1 (the W of apply()).  Then

  J . dX     = the row sums of dW . u plus dnws . b,   (dW, dnws) = shape_tangent(dX) with add_neumann = True
  J^T . v    = shape_adjoint(ghat, ghat_nws) with ghat[pos] = v_p u[esup[pos]], ghat_nws = v_p b_p, add_neumann = True

in a number format of the caller's choice (numpy.longdouble is the 80-bit model the device is held to, numpy.float64 the restatement).
The scales are the models' own: per row, the tangent's row scale times sum |u| + |b| (D.jvp_of); per coordinate, the sum of the absolute
contributions carried through the geometry chain, |v| included (SM.shape_adjoints).

Not a test module (no test_ prefix).  Plain numpy."""
import gls_derivative_exact as D
import gls_shape_model as SM
import gls_shape_tangent_model as STM
from gls_exact import LD


def jvp_models(grid, perm, diff_mag, flag, inpoel, inpofa, u, bs, directions, dtype=LD):
    """J . dX for every b of bs (an array [P] or None each) and every direction dX [P][3]: out[i][j] for bs[i] and directions[j], a dict
    with `value` [P], `scale` [P] and `computed` [P]; one factorisation per node for all of them"""
    tans = STM.shape_tangents(grid, perm, diff_mag, flag, inpoel, inpofa, directions, True, dtype)
    return [[dict(D.jvp_of(grid, t, u, b, dtype), computed=t["computed"]) for t in tans] for b in bs]


def vjp_models(grid, perm, diff_mag, flag, inpoel, inpofa, u, bs, fields, dtype=LD):
    """J^T . v for every b of bs and every node field v [P]: out[i][j] for bs[i] and fields[j], a dict with `grad_points` [P][3], `scale`
    [P][3] and `computed` [P]; one factorisation per node for all of them"""
    cots = [D.cotangent(grid, u, v, b, dtype) + (True,) for b in bs for v in fields]
    out = SM.shape_adjoints(grid, perm, diff_mag, flag, inpoel, inpofa, cots, dtype)
    return [out[i * len(fields):(i + 1) * len(fields)] for i in range(len(bs))]
