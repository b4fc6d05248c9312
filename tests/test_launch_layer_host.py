"""The host side of the launch layer (csrc/launch.hpp) on a CPU: tools/launch_layer_driver.hip, a stand-alone program, checks the chunk
walk (for_each_chunk<4> and <2>, n = 0 .. 9: the partition, the sizes, the early stop), launch_status (0 for hipSuccess; NIN_EHIP and
HIP's words in nin_last_error() for an error it is handed) and blocks_for (n = 0, 1, 256, 257, 2^31 + 1 at 16 and 256 per block).  It
launches nothing and opens no device.  Built here with hipcc and linked with the objects the library's build left."""
import glob
import os
import shutil
import subprocess

import pytest

from ninpol_amd import build as nin_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_launch_layer_driver_answers_as_expected(tmp_path):
    hipcc = shutil.which("hipcc") or os.path.join(nin_build.ROCM, "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    nin_build.build()
    objs = sorted(glob.glob(os.path.join(nin_build.OBJ, "*.o")))
    if len(objs) != len(nin_build.UNITS):      # (a tree that came with the library but without its objects)
        nin_build.build(force=True)
        objs = sorted(glob.glob(os.path.join(nin_build.OBJ, "*.o")))
    exe = str(tmp_path / "launch_layer_driver")
    rocm_lib = os.path.join(nin_build.ROCM, "lib")
    subprocess.check_call([hipcc, f"--offload-arch={nin_build.ARCH}", "-O1", "-std=c++17", "-c", os.path.join(ROOT, "tools", "launch_layer_driver.hip"),
                           "-o", exe + ".o"])
    subprocess.check_call([hipcc, f"--offload-arch={nin_build.ARCH}", exe + ".o"] + objs +
                          ["-L", rocm_lib, "-lamdhip64", "-lgomp", "-Wl,-rpath," + rocm_lib, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
    lines = run.stdout.splitlines()
    assert lines[0] == "for_each_chunk<4>: ok"
    assert lines[1] == "for_each_chunk<2>: ok"
    assert lines[2].startswith("launch_status: ok (\"launch failed: ") and "invalid configuration argument" in lines[2]
    assert lines[3] == "blocks_for: ok"
    assert lines[4] == "launch_layer_driver: all answers as expected"
    assert run.stderr == ""
