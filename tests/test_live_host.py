"""The host logic of tw_set_live_delays (csrc/live_plan.hpp), CPU only: a
stand-alone program built with ASan + UBSan runs every refusal, the per-link
descriptors (a reversed range, k = 1, k at the one-draw bound), draws against
the oracle's randomR, and the exactness of the reciprocal the event kernels
use for `mod k`: every k the plan admits, at 0, k - 1, k, 2147483561 and 2,048
random arguments each.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def live_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("live") / "live_plan"
    # (-O2: the reciprocal sweep is 4.4e9 arguments; the runtimes linked
    # statically, as in test_load_host.py)
    subprocess.run([cxx, "-std=c++17", "-g", "-O2", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "live_plan_main.cpp")], check=True)
    return str(exe)


def test_checks_descriptors_and_draws_under_sanitizers(live_exe):
    r = subprocess.run([live_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "live plan ok" in r.stdout


def test_reciprocal_is_exact_for_every_admitted_k(live_exe):
    r = subprocess.run([live_exe, "recip"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"recip ok: {2147483 * (2048 + 10)} arguments over k = 1 .. 2147483" in r.stdout
