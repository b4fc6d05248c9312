"""Both device forms of tau = u^(-eta) -- the series (glsmath::face_tau_t) and the tables (glsmath::face_tau_tab_t, read from LDS
as the cube-node kernel reads them) -- through tools/test_face_tau.hip on the model's grid, against numpy's pow."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import proto_face_tau as T  # noqa: E402


@pytest.mark.gpu
def test_gpu_face_tau_against_numpy_pow(tmp_path):
    exe = os.path.join(ROOT, "tools", "_bin", "test_face_tau")
    assert os.path.exists(exe), "python -c 'import __graft_entry__ as g; g.build()' builds it"
    u, eta = T.grid(n_u=600, n_eta=80)
    uu, ee = [a.ravel() for a in np.meshgrid(u, eta, indexing="ij")]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int64(uu.size).tobytes())
        f.write(np.stack([uu, ee], axis=1).astype(np.float64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all ok" in r.stdout, r.stdout[-1000:] + r.stderr[-1000:]
    out = np.fromfile(fout, dtype=np.float64).reshape(-1, 4)
    ref = np.power(uu, -ee)
    ref_sq = np.power(uu * uu, -0.5 * ee)
    low = ee <= 1.0
    err = {}
    for name, col, rf in (("series", 0, ref), ("tab", 1, ref), ("series_sq", 2, ref_sq), ("tab_sq", 3, ref_sq)):
        rel = np.abs(out[:, col] - rf) / rf
        err[name] = (rel[low].max(), rel.max())
        print(f"{name}: max relative error {rel[low].max():.3e} on eta in (0, 1], {rel.max():.3e} on (0, 4], mean {rel.mean():.3e}")
    # the series where it was documented; the tables there and on (0, 4]
    assert err["series"][0] <= T.DOCUMENTED_SERIES_ERROR and err["series_sq"][0] <= T.DOCUMENTED_SERIES_ERROR
    for name in ("tab", "tab_sq"):
        assert err[name][0] <= T.DOCUMENTED_SERIES_ERROR and err[name][1] <= T.DOCUMENTED_SERIES_ERROR, err
    # the device runs the model's arithmetic: a sample of the grid bit for bit
    K = T.read_header()
    for i in np.random.default_rng(3).choice(uu.size, 300, replace=False):
        assert out[i, 1] == T.face_tau_tab(float(uu[i]), float(ee[i]), False, K), (uu[i], ee[i])
        assert out[i, 3] == T.face_tau_tab(float(uu[i] * uu[i]), float(ee[i]), True, K), (uu[i], ee[i])
