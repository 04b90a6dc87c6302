"""The thread protocol of the pipelined host calls without a device: tools/stage_check.cpp includes csrc/glc_stages.hpp
alone and holds Worker, StageGate and run_stages to their properties with fake stages - a consumer sees a round only
after its producer advanced past it, a failure in any stage at any round stops the others within the round they are in
and the FIRST error comes back, stop() releases a blocked helper, a job that throws comes back as GLC_ENOMEM, a Worker
runs its jobs on one thread and one without a job destroys cleanly, and the runner never returns while a helper runs.
Built here twice and run: with AddressSanitizer + UBSan, and with ThreadSanitizer.  It is plain host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fno-sanitize-recover=all"]


def gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.fail("g++ is needed to build tools/stage_check.cpp")
    return exe


def build_and_run(tmp_path, sanitize):
    exe = str(tmp_path / "stage_check")
    subprocess.check_call([gxx(), *FLAGS, "-fsanitize=" + sanitize, os.path.join(ROOT, "tools", "stage_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "stages ok" in run.stdout


def test_stages_hold_their_properties_under_asan_and_ubsan(tmp_path):
    build_and_run(tmp_path, "address,undefined")


def test_stages_hold_their_properties_under_tsan(tmp_path):
    # a host on which the thread sanitizer's run-time cannot start at all (it maps fixed address ranges) shows that
    # with an empty program built the same way: only there is this half skipped
    src, probe = tmp_path / "empty.cpp", str(tmp_path / "empty")
    src.write_text("int main() { return 0; }\n")
    subprocess.check_call([gxx(), *FLAGS, "-fsanitize=thread", str(src), "-o", probe])
    if subprocess.run([probe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("the thread sanitizer's run-time does not start on this host")
    build_and_run(tmp_path, "thread")
