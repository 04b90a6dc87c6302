"""The argument rules of the device batch, store and stream calls without a device: tools/arg_rules_check.cpp includes
csrc/glc_args.hpp alone and holds the rules to the properties DESIGN.md section 3 states - a layout that passes the
stride rule gives every sample an element of its own inside its clip's slot and below the extent, one that fails it
fails by exactly the stated inequality; the frames rule at 512 / 513 samples per channel and at 2^32 rows; overlap of
byte spans, the pairwise list, the in-place exception; alignment and the formats at every boundary; the message texts
the refusal tests of the suite assert.  Built here with AddressSanitizer and UBSan and run: it is plain host code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arg_rules_hold_their_properties(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tools/arg_rules_check.cpp")
    exe = str(tmp_path / "arg_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "arg_rules_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "arg rules ok" in run.stdout
