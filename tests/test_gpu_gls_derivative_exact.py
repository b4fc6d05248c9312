"""Every GLS derivative kernel held to the 80-bit model of tests/gls_derivative_exact.py: the adjoint in K
(DevicePlan.launch_weights_backward), the tangent (launch_weights_tangent), the kept Jacobian (linearize, launch_jvp / launch_vjp) and
the reduced Jacobian (linearize_reduced, M = 1 / 3 / 6) -- on the ALH, FAN and LIN tensors, on seven transforms of the mesh off the unit
box and past eta = 1, and on the Delaunay mesh that populates every bin (the table: gls_derivative_exact.CASES; the two cases left out
and why: LEFT_OUT there).  The paths that exist in the derivative alone see inputs the older files never gave them: -log|U| tau on
both sides of |U| = 1, glsmath::face_tau past eta = 1, the pick rule at ties (FAN, lin_x*) and where eta is nobody's (LIN), the fold
factor at other traces than ALH's.

The bar, per (case, surface, output), on the scale of the 80-bit model:

    dist(device, exact) <= max(SLACK x dist(float64 restatement, exact), the surface's existing bar)

The restatement is the same algorithm in plain float64 on the CPU (its distance is computed in the test); SLACK =
util.GLS_EXACT_SLACK_CAP: four times worse than that has lost accuracy somewhere.  The floor is the bar the surface's own file holds
it to against its lstsq model, imported: on the well-conditioned cases a numpy QR is 5e-14 from exact and a correct kernel a few 1e-13,
so the ratio alone would fail a correct kernel by a factor of ten.  Nothing in the bar is measured on the code under test, and it can
never exceed SLACK x CASE_CAP (a case whose restatement is further than CASE_CAP from exact is not in the set).

Every output buffer is NaN-filled before its launch and must come back finite.  One line per test with the figures (profiles/r17/
derivative_exact.txt keeps those of an MI355X run; the worst are in DESIGN.md 4.11 to 4.14)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # the child process of test_forced_global_class: the paths tests/conftest.py sets up
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import gls_adjoint_model as GM  # noqa: E402
import gls_derivative_exact as D  # noqa: E402
import util  # noqa: E402
from test_gpu_gls_jacobian import JVP_RTOL, VJP_RTOL  # noqa: E402
from test_gpu_gls_reduced_jacobian import RJVP_RTOL, RVJP_RTOL  # noqa: E402
from test_gpu_gls_tangent import ADJOINT_RTOL, TANGENT_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

SLACK = util.GLS_EXACT_SLACK_CAP
FLOOR = {"backward": ADJOINT_RTOL, "tangent": TANGENT_RTOL, "tangent_explicit": TANGENT_RTOL, "jvp": JVP_RTOL, "jvp_explicit": JVP_RTOL,
         "vjp": VJP_RTOL, "rjvp": RJVP_RTOL, "rvjp": RVJP_RTOL}
assert max(FLOOR.values()) <= SLACK * D.CASE_CAP


def _torch():
    import torch
    return torch


class Device:
    """one Problem on the device: the launches of every surface into NaN-filled buffers"""

    def __init__(self, name):
        from ninpol_amd.interpolator import DevicePlan
        torch = _torch()
        self.pb = pb = D.Problem(name)
        self.dev = torch.device("cuda", int(pb.I.device))
        self.plan = DevicePlan(pb.I, "u", "gls")
        self._jac = None
        self._red = {}

    def stream(self):
        return _torch().cuda.current_stream(self.dev).cuda_stream

    def to_dev(self, a):
        return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def nan(self, *shape):
        torch = _torch()
        return torch.full(shape, float("nan"), dtype=torch.float64, device=self.dev)

    def host(self, *tensors):
        _torch().cuda.synchronize(self.dev)
        out = [t.cpu().numpy() for t in tensors]
        assert all(np.all(np.isfinite(a)) for a in out), "a device result is not finite (or was not written)"
        return out

    def backward(self, unfolded):
        pb = self.pb
        g, gn = self.to_dev(pb.ghat), self.to_dev(pb.gnws)
        gp, gd = self.nan(pb.E, 9), self.nan(pb.E)
        self.plan.launch_weights_backward(g.data_ptr(), gp.data_ptr(), gd.data_ptr() if unfolded else 0, gn.data_ptr(), self.stream(),
                                          add_neumann=True)
        return self.host(gp, gd) if unfolded else self.host(gp) + [None]

    def tangent(self, ddm=None):
        """k = 1; ddm None: folded"""
        pb = self.pb
        d, dm = self.to_dev(pb.dK.reshape(1, pb.E, 9)), None if ddm is None else self.to_dev(np.reshape(ddm, (1, pb.E)))
        out, nws = self.nan(1, pb.nnz), self.nan(1, pb.P)
        self.plan.launch_weights_tangent(d.data_ptr(), out.data_ptr(), 1, 0 if dm is None else dm.data_ptr(), nws.data_ptr(), self.stream(),
                                         add_neumann=True)
        out, nws = self.host(out, nws)
        return out[0], nws[0]

    def jac(self):
        if self._jac is None:
            ud, bd = self.to_dev(self.pb.u), self.to_dev(self.pb.b)
            self._jac = self.plan.linearize(ud.data_ptr(), bd.data_ptr(), self.stream())
            _torch().cuda.synchronize(self.dev)
        return self._jac

    def jvp(self, explicit):
        pb = self.pb
        d, dm = self.to_dev(pb.dK.reshape(1, pb.E, 9)), self.to_dev(pb.ddm.reshape(1, pb.E))
        out = self.nan(1, pb.P)
        self.jac().launch_jvp(d.data_ptr(), out.data_ptr(), 1, dm.data_ptr() if explicit else 0, self.stream())
        return self.host(out)[0][0]

    def vjp(self, unfolded):
        pb = self.pb
        vd = self.to_dev(pb.v.reshape(1, pb.P))
        gp, gd = self.nan(1, pb.E, 9), self.nan(1, pb.E)
        self.jac().launch_vjp(vd.data_ptr(), gp.data_ptr(), 1, gd.data_ptr() if unfolded else 0, self.stream())
        if unfolded:
            gp, gd = self.host(gp, gd)
            return gp[0], gd[0]
        return self.host(gp)[0][0], None

    def red(self, M):
        if M not in self._red:
            pb = self.pb
            _, arr, per_cell = pb.reduced.bases[D.REDUCED_BASES[M]]
            ud, bd = self.to_dev(pb.u), self.to_dev(pb.b)
            Bd = None if arr is None else self.to_dev(arr)
            self._red[M] = self.plan.linearize_reduced(ud.data_ptr(), M, 0 if Bd is None else Bd.data_ptr(), per_cell, bd.data_ptr(),
                                                       self.stream())
            _torch().cuda.synchronize(self.dev)
        return self._red[M]

    def rjvp(self, M):
        pb = self.pb
        d, out = self.to_dev(pb.dtheta(M).reshape(1, pb.E, M)), self.nan(1, pb.P)
        self.red(M).launch_jvp(d.data_ptr(), out.data_ptr(), 1, self.stream())
        return self.host(out)[0][0]

    def rvjp(self, M):
        pb = self.pb
        vd, out = self.to_dev(pb.v.reshape(1, pb.P)), self.nan(1, pb.E, M)
        self.red(M).launch_vjp(vd.data_ptr(), out.data_ptr(), 1, self.stream())
        return self.host(out)[0][0]


_DEVICES = {}


def get(name):
    if name not in _DEVICES:
        _DEVICES[name] = Device(name)
    return _DEVICES[name]


def bar_of(pb, surface, output):
    """(the float64 restatement's distance from the 80-bit model, the bar of the module's docstring, the term of it that applies) for
    one output of one surface; the reduced surfaces carry their M behind the name"""
    d_ref = pb.distances({surface: pb.run(np.float64)[surface]})[(surface, output)]
    floor = FLOOR[surface.rstrip("136")]
    return d_ref, max(SLACK * d_ref, floor), "ratio" if SLACK * d_ref > floor else "floor"


def hold(pb, surface, output, d_dev, tag=""):
    """prints the line of record of one output and returns whether the device is inside the bar (the callers assert once all their
    lines are out)"""
    d_ref, bar, term = bar_of(pb, surface, output)
    assert d_ref <= D.CASE_CAP, (pb.name, surface, output, d_ref)
    ratio = d_dev / d_ref if d_ref > 0 else (0.0 if d_dev == 0 else float("inf"))
    print(f"{pb.name} {surface}{tag} {output}: restatement {d_ref:.2e}, device {d_dev:.2e}, ratio {ratio:.2f}, "
          f"bar {bar:.2e} ({term}){'' if d_dev <= bar else '  MISSED'}")
    return d_dev <= bar


def check_backward(dv, tag=""):
    pb, ex = dv.pb, dv.pb.run(D.LD)["backward"]
    gp, gd = dv.backward(True)
    fo, _ = dv.backward(False)
    ok = [hold(pb, "backward", "grad_perm", D.dist(gp, ex["grad_perm"], ex["scale_perm"]), tag),
          hold(pb, "backward", "grad_diff_mag", D.dist(gd, ex["grad_diff_mag"], ex["scale_diff_mag"]), tag),
          hold(pb, "backward", "folded", D.dist(fo, ex["folded"], ex["scale_folded"]), tag)]
    assert all(ok), (pb.name, "backward" + tag)


def check_tangent(dv, tag=""):
    pb, ex = dv.pb, dv.pb.run(D.LD)
    t, n = dv.tangent()
    assert not n[pb.flag == 0].any()
    ok = [hold(pb, "tangent", "tangent", D.tangent_dist(pb.grid, t, n, ex["tangent"]), tag)]
    t, n = dv.tangent(pb.ddm)
    ok.append(hold(pb, "tangent_explicit", "tangent", D.tangent_dist(pb.grid, t, n, ex["tangent_explicit"]), tag))
    assert all(ok), (pb.name, "tangent" + tag)


@pytest.fixture(params=list(D.CASES))
def dv(request):
    return get(request.param)


def test_backward(dv):
    """launch_weights_backward, unfolded and folded, with grad_neumann_ws"""
    ex = dv.pb.run(D.LD)["backward"]
    assert np.count_nonzero(ex["grad_perm"]) > 0 and np.count_nonzero(ex["neumann_ws"]) > 0 and not ex["computed"].all()
    check_backward(dv)


def test_tangent(dv):
    """launch_weights_tangent, k = 1, folded and with an explicit d diff_mag, with tangent_neumann_ws"""
    check_tangent(dv)


def test_jacobian(dv):
    """linearize + launch_jvp (folded, explicit) / launch_vjp (folded, unfolded), n = 1, neumann_values given"""
    pb, ex = dv.pb, dv.pb.run(D.LD)
    ok = []
    for surface, explicit in (("jvp", False), ("jvp_explicit", True)):
        e = ex[surface]
        ok.append(hold(pb, surface, "value", D.dist(dv.jvp(explicit), e["value"], e["scale"])))
    e = ex["vjp"]
    gp, gd = dv.vjp(True)
    ok.append(hold(pb, "vjp", "grad_perm", D.dist(gp, e["grad_perm"], e["scale_perm"])))
    ok.append(hold(pb, "vjp", "grad_diff_mag", D.dist(gd, e["grad_diff_mag"], e["scale_diff_mag"])))
    fo, _ = dv.vjp(False)
    ok.append(hold(pb, "vjp", "folded", D.dist(fo, e["folded"], e["scale_folded"])))
    assert all(ok), (pb.name, "jacobian")


def _reduced(dv, M):
    pb, ex = dv.pb, dv.pb.run(D.LD)
    e = ex[f"rjvp{M}"]
    ok = [hold(pb, f"rjvp{M}", "value", D.dist(dv.rjvp(M), e["value"], e["scale"]))]
    e = ex[f"rvjp{M}"]
    ok.append(hold(pb, f"rvjp{M}", "grad_theta", D.dist(dv.rvjp(M), e["grad_theta"], e["scale"])))
    assert all(ok), (pb.name, f"reduced, M = {M}")


def test_reduced_jacobian_three_parameters(dv):
    """linearize_reduced with a random per-cell basis of three parameters + its launch_jvp / launch_vjp, n = 1"""
    _reduced(dv, 3)


@pytest.mark.parametrize("M", (1, 6))
@pytest.mark.parametrize("name", D.REDUCED_ALL_M)
def test_reduced_jacobian_one_and_six_parameters(name, M):
    """M = 1: the resident permeability as the basis (a NULL pointer); M = 6: the built-in symmetric basis, shared"""
    _reduced(get(name), M)


@pytest.mark.parametrize("name", [k for k in D.CASES if k.endswith("/LIN")])
def test_lin_eta_is_nobodys(name):
    """diff_mag == 0 on every cell: max() takes eta from nobody, so grad_diff_mag is exactly 0 and d diff_mag never enters"""
    dv = get(name)
    pb = dv.pb
    assert not pb.dmag.any()
    _, gd = dv.backward(True)
    assert not gd.any()
    _, gd = dv.vjp(True)
    assert not gd.any()
    with_ddm, zero = dv.tangent(pb.ddm), dv.tangent(np.zeros(pb.E))
    assert with_ddm[0].tobytes() == zero[0].tobytes() and with_ddm[1].tobytes() == zero[1].tobytes() and with_ddm[0].any()
    assert dv.jvp(True).tobytes() == dv.jvp(False).tobytes()          # (the fold factor is 0 at tr K = 3 as well)


@pytest.mark.parametrize("name", [k for k in D.CASES if k.endswith("/lin_x0.45_eta1.49")])
def test_a_tie_is_charged_to_the_first_cell(name):
    """every face a tie at diff_mag > 0: the forward's max() keeps cell a, so only first cells of internal faces carry grad_diff_mag"""
    dv = get(name)
    pb = dv.pb
    assert pb.dmag.min() > 0 and np.all(pb.dmag == pb.dmag[0])
    fc = GM.face_cells(pb.grid)
    first = np.zeros(pb.E, dtype=bool)
    first[fc[fc[:, 1] >= 0, 0]] = True
    assert first.any() and not first.all()
    _, gd = dv.backward(True)
    assert gd[first].any() and not gd[~first].any()


CHILD_CASES = ("hex/FAN", "hex/lin_x0.36_eta3.16")


def _child():
    _torch().cuda.init()                    # torch opens the device before the native library does (tests/conftest.py does it for pytest)
    for name in CHILD_CASES:
        dv = get(name)
        check_tangent(dv, " forced global")     # (the tangent call makes the bins itself)
        plan = dv.pb.grid.gls_adjoint_plan()
        assert plan == {"lds1": 0, "lds2": 0, "lds4": 0, "global": dv.pb.P}, plan
        check_backward(dv, " forced global")
    print("CHILD OK")


def test_forced_global_class():
    """backward and tangent on hex / FAN and hex / lin_x0.36_eta3.16 with every system in global-memory scratch, in a fresh process (the
    switch is read when the bins are made), under the same bar"""
    env = dict(os.environ, NIN_GLS_ADJ_FORCE_GLOBAL="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


if __name__ == "__main__":
    _child()
