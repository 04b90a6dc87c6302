"""The round rule of the batch, store and stream drivers without a device: tools/round_plan_check.cpp includes
csrc/glc_rounds.hpp alone and holds pack_rounds to the properties DESIGN.md section 3 states (every item in one round,
in order, none empty, the sums, `lng` exactly for an item that fits no round, the budget, greediness) over the budgets
and fronts the drivers use and a few tiny ones, and TableOffsets to 256-byte tables that do not overlap.  With
csrc/glc_common.h it holds the rounds of ONE stream to theirs: encode_stream_rounds tiles the stream with four opening
rounds, whole chunks and no short last round; the upload marks of its rounds never decrease, cover each round's halo and
end at the stream's length; the output spans of the decode rounds tile what the trim keeps.  Built here
with AddressSanitizer and UBSan and run: it is plain host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_plan_holds_its_properties(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tools/round_plan_check.cpp")
    exe = str(tmp_path / "round_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "round_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "round plan ok" in run.stdout
