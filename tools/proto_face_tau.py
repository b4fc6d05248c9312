#!/usr/bin/env python3
"""tau = u^(-eta) by tables: the numpy / exact-arithmetic model of glsmath::face_tau_tab_t (csrc/gls_device_math.hpp),
operation for operation, and the generator of its constants (csrc/gls_tau_table.hpp).

    python tools/proto_face_tau.py            measure the model against numpy's pow on the grid below
    python tools/proto_face_tau.py --emit     print csrc/gls_tau_table.hpp

The scheme.  u = 2^e m, m in [1/2, 1); i = the top 7 mantissa bits of m; c_i the midpoint of interval i.
  log:  the table holds rc_i = fl(1 / c_i) and lc_i = -log(rc_i) (of the ROUNDED reciprocal, so that m rc_i - 1 is f with
        log m = lc_i + log1p(f) exactly) as lh_i + ll_i, lh_i a multiple of 2^-40.  f = fma(m, rc_i, -1), |f| <= 2^-8;
        log1p(f) = f + f^2 g(f), g of degree 3 (economised: 8e-17 on the logarithm).  s = e LN2_HI + lh_i is EXACT
        (LN2_HI has 31 bits), everything else of the logarithm is the small word w = f + (e LN2_LO + ll_i + f^2 g).
  pow:  eta log u = yh + yl with yh = fl(eta s), yl = fma(eta, s, -yh) + eta w: the product is carried in two words,
        because one rounding of y = 55 (u = 1e-6, eta = 4) would already be 6e-15 on tau.
  exp:  c = -1 (or -1/2: the argument is u^2) is folded into the constants.  k = rint(yh c 32 / ln2), rho = c (yh + yl) -
        k ln2 / 32, |rho| <= ln2 / 64 + |c| eta 2^-8 (k ignores yl: 0.0265 at |c| eta = 4);
        exp(rho) = 1 + rho Q(rho), Q of degree 5 (economised over |rho| <= 0.0275: 3e-17);
        tau = 2^(k >> 5) T_j (1 + rho Q), T_j = fl(2^(j / 32)), j = k & 31.
The model does every fma exactly (fractions.Fraction, one rounding), so it is the device's arithmetic bit for bit.
"""
import decimal
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ninpol_amd", "csrc", "gls_tau_table.hpp")
LOG_N, EXP_N = 128, 32
LN2_HI = float.fromhex("0x1.62e42feep-1")       # 31 bits: e * LN2_HI is exact
RHO_MAX = 0.0275
DOCUMENTED_SERIES_ERROR = 1.8e-15                 # face_tau_t, gls_device_math.hpp


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def generate():
    """The constants, from 60-digit arithmetic: {name: list of floats}."""
    decimal.getcontext().prec = 60
    D = decimal.Decimal
    ln2 = D(2).ln()
    rc, lh, ll = [], [], []
    for i in range(LOG_N):
        r = 1.0 / (0.5 + (i + 0.5) / (2 * LOG_N))
        lc = -D(r).ln()
        h = float(round(lc * 2 ** 40)) / 2.0 ** 40
        rc.append(r); lh.append(h); ll.append(float(lc - D(h)))
    ex = [float(D(2) ** (D(j) / EXP_N)) for j in range(EXP_N)]
    from numpy.polynomial import chebyshev as C, polynomial as P

    def g(f):      # (log1p(f) - f) / f^2
        return sum((-1.0) ** (n + 1) * f ** (n - 2) / n for n in range(14, 1, -1))

    def q(r):      # (exp(r) - 1) / r
        return np.expm1(r) / r
    fmax = 2.0 ** -8 * (1 + 2.0 ** -20)
    lg = P.Polynomial(C.cheb2poly(C.chebinterpolate(lambda t: g(fmax * t), 3)))
    eq = P.Polynomial(C.cheb2poly(C.chebinterpolate(lambda t: q(RHO_MAX * t), 5)))
    return {"kTauTab": rc + lh + ll + ex,
            "TAU_LG": [float(c / fmax ** n) for n, c in enumerate(lg.coef)],
            "TAU_EX": [float(c / RHO_MAX ** n) for n, c in enumerate(eq.coef)],
            "TAU_LN2_LO": [float(ln2 - D(LN2_HI))],
            "TAU_INV_L": [float(D(EXP_N) / ln2)]}


def emit():
    k = generate()

    def arr(v):
        return ",\n".join("    " + ", ".join(x.hex() for x in v[i:i + 4]) for i in range(0, len(v), 4))
    print("// gls_tau_table.hpp -- constants of glsmath::face_tau_tab_t: written by tools/proto_face_tau.py --emit, which explains them")
    print("#pragma once")
    print("#include <hip/hip_runtime.h>")
    print("\nnamespace nin {\nnamespace glsmath {\n")
    print(f"constexpr int TAU_LOG_N = {LOG_N}, TAU_EXP_N = {EXP_N}, TAU_TAB_DOUBLES = {3 * LOG_N + EXP_N};")
    print("// [0, 128): rc_i;  [128, 256): lh_i;  [256, 384): ll_i;  [384, 416): 2^(j / 32)")
    print(f"__device__ const double kTauTab[TAU_TAB_DOUBLES] = {{\n{arr(k['kTauTab'])}}};")
    print(f"constexpr double TAU_LG[4] = {{{', '.join(x.hex() for x in k['TAU_LG'])}}};   // g(f) = (log1p(f) - f) / f^2")
    print(f"constexpr double TAU_EX[6] = {{{', '.join(x.hex() for x in k['TAU_EX'])}}};   // Q(rho) = (exp(rho) - 1) / rho")
    print(f"constexpr double TAU_LN2_HI = {LN2_HI.hex()}, TAU_LN2_LO = {k['TAU_LN2_LO'][0].hex()}, TAU_INV_L = {k['TAU_INV_L'][0].hex()};   // ln 2 in two words; 32 / ln 2")
    print("\n}  // namespace glsmath\n}  // namespace nin")


def read_header(path=HEADER):
    """The constants as the device compiles them."""
    text = open(path).read()
    out = {}
    for name in ("kTauTab", "TAU_LG", "TAU_EX"):
        body = re.search(name + r"\[\w+\] = \{(.*?)\};", text, re.S).group(1)
        out[name] = [float.fromhex(x) for x in re.findall(r"-?0x[0-9a-f.]+p[-+]\d+", body)]
    for name in ("TAU_LN2_HI", "TAU_LN2_LO", "TAU_INV_L"):
        out[name] = [float.fromhex(re.search(name + r" = (-?0x[0-9a-f.]+p[-+]\d+)", text).group(1))]
    return out


def face_tau_tab(un, eta, squared, K):
    """One call of face_tau_tab_t<SQUARED>, in the device's order of operations."""
    if eta == 0.0:
        return 1.0
    tab, G, E = K["kTauTab"], K["TAU_LG"], K["TAU_EX"]
    c = -0.5 if squared else -1.0
    m, e = math.frexp(un)
    ef = float(e)
    i = (np.float64(m).view(np.uint64) >> np.uint64(45)) & np.uint64(127)    # (hi word >> 13) & 127
    i = int(i)
    f = fma(m, tab[i], -1.0)
    f2 = f * f
    g = fma(G[3], f, G[2]); g = fma(g, f, G[1]); g = fma(g, f, G[0])
    s = fma(ef, K["TAU_LN2_HI"][0], tab[LOG_N + i])
    t = fma(ef, K["TAU_LN2_LO"][0], tab[2 * LOG_N + i])
    t = fma(f2, g, t)
    w = f + t
    yh = eta * s
    yl = fma(eta, w, fma(eta, s, -yh))
    k = float(round(yh * (c * K["TAU_INV_L"][0])))           # round half to even, as v_rndne_f64
    r = fma(k, -(K["TAU_LN2_HI"][0] / EXP_N) / c, yh)
    r = fma(k, -(K["TAU_LN2_LO"][0] / EXP_N) / c, r)
    r = r + yl                                                # rho = c r
    cn = [E[n] * c ** (n + 1) for n in range(6)]              # (powers of two: exact)
    q = fma(cn[5], r, cn[4])
    for n in (3, 2, 1, 0):
        q = fma(q, r, cn[n])
    ki = int(k)
    T = tab[3 * LOG_N + (ki & (EXP_N - 1))]
    return math.ldexp(fma(T * r, q, T), ki >> 5)


def grid(n_u=240, n_eta=48):
    """u in [1e-6, 1e2] (log-spaced, and the same jittered), eta in (0, 4] -- (0, 1] is the range the series was documented on."""
    rng = np.random.default_rng(7)
    u = np.concatenate([np.logspace(-6, 2, n_u), 10.0 ** rng.uniform(-6, 2, n_u)])
    eta = np.concatenate([np.linspace(0, 1, n_eta // 2 + 1)[1:], np.linspace(1, 4, n_eta // 2 + 1)[1:]])
    return u, eta


def measure(K=None, n_u=240, n_eta=48):
    """Max and mean relative error of both forms against numpy's pow, (0, 1] and (0, 4] apart."""
    K = K or read_header()
    u, eta = grid(n_u, n_eta)
    res = {}
    for squared in (False, True):
        arg = u * u if squared else u
        ref = np.power(arg[:, None], (-0.5 if squared else -1.0) * eta[None, :])
        got = np.array([[face_tau_tab(float(a), float(h), squared, K) for h in eta] for a in arg])
        rel = np.abs(got - ref) / ref
        low = eta <= 1.0
        res[squared] = (rel[:, low].max(), rel.max(), rel.mean())
    return res


if __name__ == "__main__":
    if "--emit" in sys.argv:
        emit()
    else:
        for squared, (e1, e4, mean) in measure().items():
            print(f"face_tau_tab_t<{str(squared).lower()}>: max relative error {e1:.2e} on eta in (0, 1], {e4:.2e} on (0, 4], mean {mean:.2e}")
