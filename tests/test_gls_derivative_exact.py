"""The yardstick of tests/test_gpu_gls_derivative_exact.py validated on its own (CPU): tests/gls_derivative_exact.py restates the adjoint
and the tangent of the GLS weights through one Householder QR, in 80-bit arithmetic (the model every derivative kernel is held to) and
in float64 (the restatement whose distance from the model sets the kernels' bar).  Before a kernel is held to it:
  * on the four ALH unit-box cases the lstsq models of the older device tests -- pinned to central differences of the oracle -- are
    within those tests' own bars of the 80-bit model: the new yardstick and the old ones say the same thing where both can speak;
  * on every case the 80-bit adjoint and the 80-bit tangent, two derivations that share nothing behind the assembly, agree through
    the duality <ghat, dd> + <gnws, dnws> = <Kbar, dK> + <etabar, ddm> to DUALITY_RTOL of the sum of the absolute terms: that is the
    evidence that the formulas hold on FAN, off the unit box and at ties, where central differences are too noisy to pin them;
  * on every case and output the float64 restatement is within CASE_CAP of the 80-bit model (printed: `pytest -s`), and the two
    cases left out are measured too;
  * the cases have teeth: four one-line mutations of the restatement -- the places where a derivative kernel can be wrong while every
    forward kernel is right -- each exceed the GPU bar on a named case, and a wrong tie rule passes every ALH case;
  * on LIN, where eta is nobody's, grad_diff_mag is exactly zero and the tangent does not depend on d diff_mag.
No kernel is touched here."""
import numpy as np
import pytest

import gls_adjoint_model as GM
import gls_derivative_exact as D
import gls_jacobian_model as JM
import gls_reduced_jacobian_model as RM
import gls_tangent_model as TM
from gls_derivative_exact import LD
from test_gpu_gls_derivative_exact import bar_of
from test_gpu_gls_jacobian import JVP_RTOL, VJP_RTOL
from test_gpu_gls_reduced_jacobian import RJVP_RTOL, RVJP_RTOL
from test_gpu_gls_tangent import ADJOINT_RTOL, TANGENT_RTOL

# the 80-bit duality gap over the sum of the absolute terms: measured 0 to MEASURED_DUALITY over all cases; ten times the worst figure,
# never above 1e-15
MEASURED_DUALITY = 1.31e-18     # tet / FAN, unfolded; 0 to 1e-19 on ALH and LIN, 1e-19 to 1e-18 on FAN
DUALITY_RTOL = min(10 * MEASURED_DUALITY, 1e-15)

_PROBLEMS = {}


def problem(name, spec=None):
    from ninpol_amd import build as nbuild
    if name not in _PROBLEMS:
        nbuild.build()                      # the grid tables come from the native library's host side (no device is touched)
        _PROBLEMS[name] = D.Problem(name, spec)
    return _PROBLEMS[name]


def test_the_qr_agrees_with_an_independent_solver():
    """random full-rank 40 x 25 systems: the three solves in 80 bits against numpy's SVD-based lstsq / pinv (nothing shared)"""
    rng = np.random.default_rng(0)
    for _ in range(4):
        A, b, z = rng.standard_normal((40, 25)), rng.standard_normal(40), rng.standard_normal(25)
        for dtype, tol in ((LD, 1e-12), (np.float64, 1e-12)):
            F = D.qr(A, dtype)
            x = np.linalg.lstsq(A, b, rcond=None)[0]
            assert not F.singular and F.solve(b).dtype == dtype
            assert np.abs(F.solve(b) - x).max() <= tol * np.abs(x).max()
            assert np.abs(F.residual(b) - (b - A @ x)).max() <= tol * np.abs(b).max()
            want = np.linalg.pinv(A).T @ z
            assert np.abs(F.pinv_t(z) - want).max() <= tol * np.abs(want).max()
            blk = F.residual(np.stack([b, 2 * b], axis=1))                     # a block is its columns (another order of the sums)
            assert np.abs(blk[:, 0] - F.residual(b)).max() <= 1e-14 * np.abs(b).max()
    A[:, 3] = 0.0
    assert D.qr(A, LD).singular


def test_the_table_is_the_issues():
    assert len(D.CASES) == 9 + 21 + 1 and "delaunay/ALH" in D.CASES and "hex/lin_x0.36_eta3.16" in D.CASES
    assert not any("scale_1e-3" in k or k == "delaunay/FAN" for k in D.CASES)
    assert len(D.REDUCED_ALL_M) == 4


@pytest.mark.parametrize("name", D.UNIT_ALH)
def test_lstsq_models_against_the_80_bit_model(name):
    """the four lstsq models on the ALH unit box, each at the bar of the kernel that is held to it"""
    pb = problem(name)
    ex = pb.run(LD)
    a = GM.gls_adjoint_model(pb.grid, pb.perm, pb.dmag, pb.flag, pb.ghat, add_neumann=True, grad_neumann_ws=pb.gnws)
    a["folded"] = GM.fold(a["grad_perm"], a["grad_diff_mag"], pb.perm)
    d = D.adjoint_dist(a, ex["backward"])
    print(f"{name}: gls_adjoint_model vs exact: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= ADJOINT_RTOL
    assert np.array_equal(a["computed"], ex["backward"]["computed"])
    tans = {}
    for key, ddm in (("tangent", None), ("tangent_explicit", pb.ddm)):
        t = tans[key] = TM.gls_tangent_model(pb.grid, pb.perm, pb.dmag, pb.flag, pb.dK, ddm=ddm)
        dt = D.tangent_dist(pb.grid, t["tangent"], t["tangent_neumann_ws"], ex[key])
        print(f"{name}: gls_tangent_model vs exact, {key}: {dt:.2e}")
        assert dt <= TANGENT_RTOL
    for key in ("jvp", "jvp_explicit"):
        j = JM.jvp_model(pb.grid, pb.perm, pb.dmag, pb.flag, pb.u, pb.dK, b=pb.b, tangent=tans["tangent" + key[3:]])
        dj = D.dist(j["value"], ex[key]["value"], ex[key]["scale"])
        print(f"{name}: gls_jacobian_model.jvp_model vs exact, {key}: {dj:.2e}")
        assert dj <= JVP_RTOL
    full = JM.vjp_model(pb.grid, pb.perm, pb.dmag, pb.flag, pb.u, pb.v, b=pb.b)
    d = D.adjoint_dist(full, ex["vjp"])
    print(f"{name}: gls_jacobian_model.vjp_model vs exact: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= VJP_RTOL
    for M in (3,):                          # (the reduced model is glue over `full`: one basis, the per-cell one of three)
        B = pb.B(M)
        rj = RM.jvp_model(pb.grid, pb.perm, pb.dmag, pb.flag, pb.u, B, pb.dtheta(M), b=pb.b)
        rv = RM.vjp_model(pb.grid, pb.perm, pb.dmag, pb.flag, pb.u, B, pb.v, b=pb.b, full=full)
        dj = D.dist(rj["value"], ex[f"rjvp{M}"]["value"], ex[f"rjvp{M}"]["scale"])
        dv = D.dist(rv["grad_theta"], ex[f"rvjp{M}"]["grad_theta"], ex[f"rvjp{M}"]["scale"])
        print(f"{name}: gls_reduced_jacobian_model vs exact, M = {M}: jvp {dj:.2e}, vjp {dv:.2e}")
        assert dj <= RJVP_RTOL and dv <= RVJP_RTOL


@pytest.mark.parametrize("name", list(D.CASES))
def test_duality_in_80_bits(name):
    pb = problem(name)
    ex = pb.run(LD)
    b = ex["backward"]
    for tag, tan, rhs_terms in (("folded", ex["tangent"], [b["folded"] * pb.dK]),
                                ("unfolded", ex["tangent_explicit"], [b["grad_perm"] * pb.dK, b["grad_diff_mag"] * pb.ddm])):
        assert tan["tangent"].dtype == LD and b["grad_perm"].dtype == LD
        lhs_terms = [pb.ghat * tan["tangent"], pb.gnws * tan["tangent_neumann_ws"]]
        lhs, rhs = sum(t.sum() for t in lhs_terms), sum(t.sum() for t in rhs_terms)
        S = sum(np.abs(t).sum() for t in lhs_terms + rhs_terms)
        print(f"{name} {tag}: duality gap {float(abs(lhs - rhs) / S):.2e} of the sum of the absolute terms ({float(S):.3e})")
        assert S > 0 and abs(lhs - rhs) <= DUALITY_RTOL * S


@pytest.mark.parametrize("name", list(D.CASES))
def test_the_restatement_is_within_the_cap(name):
    """every output of every surface: the float64 restatement's distance from the 80-bit model, printed and held to CASE_CAP"""
    pb = problem(name)
    d = pb.distances(pb.run(np.float64))
    assert {s for s, _ in d} >= {"backward", "vjp", "tangent", "tangent_explicit", "jvp", "jvp_explicit", "rjvp3", "rvjp3"}
    for (s, o), v in d.items():
        print(f"{name} {s} {o}: restatement {v:.2e}")
    assert max(d.values()) <= D.CASE_CAP, max(d.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("spec", [s for s in D.LEFT_OUT if s[2] is not None], ids=lambda s: "/".join(str(x) for x in s if x))
def test_the_cases_left_out(spec):
    """scale_1e-3: the restatement's own distance from the 80-bit model, every surface, printed (the figures of LEFT_OUT's comment;
    delaunay / FAN, ten seconds of 80-bit arithmetic, is measured by `python tests/gls_derivative_exact.py` instead).  The cases are out
    of the set whatever this prints, so nothing but finiteness is asserted -- and that they are out."""
    name = "left out: " + "/".join(str(x) for x in spec if x)
    assert spec not in D.CASES.values()
    pb = problem(name, spec)
    d = pb.distances(pb.run(np.float64))
    print(f"{name}: restatement vs exact: " + ", ".join(f"{s}.{o} {v:.2e}" for (s, o), v in d.items()))
    assert all(np.isfinite(v) for v in d.values())


# ---- teeth: a mutant is the float64 restatement with one rule changed; it must exceed the bar a kernel is held to ------------------

def mutant_excess(pb, mutant):
    """{(surface, output): the mutant's distance / the bar tests/test_gpu_gls_derivative_exact.py holds a kernel to} over backward and
    tangent"""
    got = pb.run(np.float64, D.MUTANTS[mutant], reduced=False)
    d = pb.distances({s: got[s] for s in ("backward", "tangent", "tangent_explicit")})
    return {k: v / bar_of(pb, *k)[1] for k, v in d.items()}


@pytest.mark.parametrize("name", ("hex/scale_1e3", "hex/ALH", "tet/FAN"))
def test_teeth_the_sign_of_the_logarithm(name):
    """+log|U| for -log|U|: |U| >> 1 on scale_1e3, |U| < 1 on the unit box -- both signs of the factor are seen"""
    x = mutant_excess(problem(name), "log_sign")
    print(f"{name}: log_sign mutant / bar: " + ", ".join(f"{s}.{o} {v:.1e}" for (s, o), v in x.items()))
    assert x[("backward", "grad_diff_mag")] > 1 and x[("backward", "folded")] > 1 and x[("tangent", "tangent")] > 1


@pytest.mark.parametrize("name", [k for k in D.CASES if D.CASES[k][1] == "ALH" or (D.CASES[k][2] and "lin" not in D.CASES[k][2])])
def test_teeth_a_wrong_tie_passes_every_alh_case(name):
    """pick = Ib at a tie: ALH gives every cell its own diff_mag, so no ALH case -- on or off the unit box -- can see it"""
    x = mutant_excess(problem(name), "tie_to_b")
    assert max(x.values()) <= 1, (name, x)


@pytest.mark.parametrize("name", ("hex/lin_x0.45_eta1.49", "tet/lin_x0.45_eta1.49", "mixed/lin_x0.45_eta1.49", "hex/FAN"))
def test_teeth_a_wrong_tie_fails_where_every_face_is_one(name):
    x = mutant_excess(problem(name), "tie_to_b")
    print(f"{name}: tie_to_b mutant / bar: " + ", ".join(f"{s}.{o} {v:.1e}" for (s, o), v in x.items()))
    assert x[("backward", "grad_diff_mag")] > 1 and x[("backward", "folded")] > 1 and x[("tangent_explicit", "tangent")] > 1


@pytest.mark.parametrize("name", ("hex/LIN", "tet/LIN", "mixed/LIN"))
def test_teeth_eta_from_nobody(name):
    """pick = Ia where diff_mag == 0: a gradient and a tangent term where there is none"""
    x = mutant_excess(problem(name), "zero_to_a")
    print(f"{name}: zero_to_a mutant / bar: " + ", ".join(f"{s}.{o} {v:.1e}" for (s, o), v in x.items()))
    assert x[("backward", "grad_diff_mag")] > 1 and x[("tangent_explicit", "tangent")] > 1


@pytest.mark.parametrize("name", ("hex/FAN", "hex/ALH", "hex/lin_x0.36_eta3.16"))
def test_teeth_the_fold_factor(name):
    """2 (1 - 3 / tr) 3 / tr^2 with tr - 3 for tr: only the folded forms change, at every trace but LIN's own (tr = 3: a factor of 0)"""
    x = mutant_excess(problem(name), "fold_tr_shift")
    print(f"{name}: fold_tr_shift mutant / bar: " + ", ".join(f"{s}.{o} {v:.1e}" for (s, o), v in x.items()))
    assert x[("backward", "folded")] > 1 and x[("tangent", "tangent")] > 1
    assert x[("backward", "grad_perm")] <= 1 and x[("tangent_explicit", "tangent")] <= 1


@pytest.mark.parametrize("name", [k for k in D.CASES if k.endswith("/LIN")])
def test_lin_eta_is_nobodys(name):
    pb = problem(name)
    assert not pb.dmag.any()
    for dtype in (LD, np.float64):
        r = pb.run(dtype)
        assert not r["backward"]["grad_diff_mag"].any() and not r["vjp"]["grad_diff_mag"].any()
        assert not r["backward"]["scale_diff_mag"].any()
        for k in ("tangent", "tangent_neumann_ws"):
            assert np.array_equal(r["tangent"][k], r["tangent_explicit"][k]) and r["tangent"]["tangent"].any()
