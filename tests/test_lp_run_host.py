"""The host arithmetic of tw_lp_run (csrc/lp_run_plan.hpp), CPU only: a
stand-alone program built with ASan + UBSan runs the block-size rule against
the loop tw_lp_run used to hold inline (every demand 0 .. 70,000 plus -1 and
the two ends of int64, eight strides, every power-of-two block), the cases
that follow from the rule, the even node boundaries and the gathered ones
(contiguous, a gap, an overlap, an empty rank in the middle), the severity
table with "the worst of", and the parsers of TW_LP_XCAP and
TW_TEST_FAIL_TICK."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("lp_run") / "lp_run_plan"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "lp_run_plan_main.cpp")], check=True)
    return str(exe)


def test_lp_run_plan_under_sanitizers(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 200
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
