"""The host logic of tw_lp_read_trace / tw_lp_measure (csrc/lp_trace_plan.hpp),
CPU only: a stand-alone program built with ASan + UBSan runs the canonical
order, the merge of 1 to 4 record lists (empty ones and equal keys included),
the shard counts -> E / truncated / kept / gather offsets rule at E == cap,
E == cap + 1 and a cap between the largest shard count and E, and the clipping
to a smaller caller buffer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("lp_trace") / "lp_trace_plan"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "lp_trace_plan_main.cpp")], check=True)
    return str(exe)


def test_plan_merge_and_clip_under_sanitizers(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 200
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
