"""tools/proto_face_tau.py: the exact-arithmetic model of the table-driven tau (glsmath::face_tau_tab_t) against numpy's pow,
and the constants the device compiles (csrc/gls_tau_table.hpp) against their 60-digit values."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import proto_face_tau as T  # noqa: E402


def test_table_header_is_what_the_generator_writes():
    have, want = T.read_header(), T.generate()
    assert len(have["kTauTab"]) == 3 * T.LOG_N + T.EXP_N
    # the tables bit for bit (decimal arithmetic); the fitted polynomials to what numpy's Chebyshev fit reproduces
    assert have["kTauTab"] == want["kTauTab"]
    assert have["TAU_LN2_LO"] == want["TAU_LN2_LO"] and have["TAU_INV_L"] == want["TAU_INV_L"] and have["TAU_LN2_HI"] == [T.LN2_HI]
    for name in ("TAU_LG", "TAU_EX"):
        np.testing.assert_allclose(have[name], want[name], rtol=1e-9, atol=0)
    # s = e LN2_HI + lh_i is exact: both are multiples of 2^-40 and the sum stays below 2^10
    for v in [T.LN2_HI] + have["kTauTab"][T.LOG_N:2 * T.LOG_N]:
        assert (v * 2.0 ** 40).is_integer()


def test_model_against_numpy_pow():
    """No worse than the 1.8e-15 documented for the series (eta in (0, 1]), on that range and on eta in (0, 4]."""
    for squared, (e1, e4, mean) in T.measure().items():
        print(f"face_tau_tab_t<{str(squared).lower()}>: max relative error {e1:.3e} on eta in (0, 1], {e4:.3e} on (0, 4], mean {mean:.3e}")
        assert e1 <= T.DOCUMENTED_SERIES_ERROR and e4 <= T.DOCUMENTED_SERIES_ERROR


def test_model_edges():
    K = T.read_header()
    assert T.face_tau_tab(3.7, 0.0, True, K) == 1.0
    for u in (0.5, 1.0, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -52, 2.0, np.nextafter(0.75, 1), 1e-300, 1e300):
        for eta in (1e-3, 1.0, 4.0):
            ref = float(np.power(np.float64(u), -eta))
            if np.isfinite(ref) and ref > 1e-300:
                assert abs(T.face_tau_tab(float(u), eta, False, K) - ref) <= T.DOCUMENTED_SERIES_ERROR * ref, (u, eta)
