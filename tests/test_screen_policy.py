"""The guard of the screened encode without a device: tools/screen_policy_check.cpp feeds csrc/glc_resources.hpp's
ScreenPolicy the counts a repair launch would leave and checks the decisions include/glc_debug.h documents (32 launches
held off after a bad count, one probe, the fresh context's probe, mode 2, what a mode change clears, the repair's
crossover at 128 failed rows).  Built here with AddressSanitizer and UBSan and run: it is plain host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_screen_policy_takes_the_documented_decisions(tmp_path):
    gxx = shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.fail("g++ and the HIP headers are needed to build tools/screen_policy_check.cpp")
    exe = str(tmp_path / "screen_policy_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tools", "screen_policy_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "screen policy ok" in run.stdout
