"""tw_measure_quantiles' host side, CPU only: the HIP-free select logic
(csrc/measure_select.hpp) in a stand-alone program built with ASan + UBSan,
timewarp.measures.quantile_reference (the yardstick of the GPU tests) against
hand-computed cases, and the ctypes mirror of tw_quantile against the header."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from timewarp import abi, engine
from timewarp.measures import quantile_of_sorted, quantile_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
A, B = 21, 22  # hand-made tags
QS = (0, 1, 499999, 500000, 500001, 999999, 1000000)


def test_select_logic_under_sanitizers(tmp_path):
    """The argument checks, the index arithmetic up to n = 2^64 - 1, the digit
    step and the whole select loop over 1, 2 and 3 shards against
    std::nth_element and a sort, compiled without HIP with ASan + UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "select"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "measure_select_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "select ok" in r.stdout


def test_quantile_of_sorted_by_hand():
    assert quantile_of_sorted([], 500000) == (I64_MAX, I64_MIN)
    assert [quantile_of_sorted([7], q) for q in QS] == [(7, 7)] * 7
    # two values: pos = q * 1; only q = 0 and 10^6 fall on an index
    assert [quantile_of_sorted([-3, 9], q) for q in QS] == [(-3, -3)] + [(-3, 9)] * 5 + [(9, 9)]
    d = [10, 20, 30, 40]        # even: the median is between the two middle values
    assert quantile_of_sorted(d, 500000) == (20, 30)
    assert quantile_of_sorted(d, 499999) == (20, 30) and quantile_of_sorted(d, 500001) == (20, 30)
    assert quantile_of_sorted(d, 333333) == (10, 20)      # pos = 999,999: index 0, remainder
    assert quantile_of_sorted(d, 333334) == (20, 30)      # pos = 1,000,002: index 1, remainder
    assert quantile_of_sorted(d, 0) == (10, 10) and quantile_of_sorted(d, 1000000) == (40, 40)
    d = [10, 20, 30, 40, 50]    # odd: the middle one
    assert quantile_of_sorted(d, 500000) == (30, 30)
    assert quantile_of_sorted(d, 499999) == (20, 30) and quantile_of_sorted(d, 500001) == (30, 40)
    assert quantile_of_sorted(d, 250000) == (20, 20) and quantile_of_sorted(d, 999999) == (40, 50)
    assert quantile_of_sorted([I64_MIN, -1, 0, I64_MAX], 500000) == (-1, 0)
    for bad in (-1, 1000001):
        with pytest.raises(ValueError):
            quantile_of_sorted(d, bad)


def _pairs(ds, base=0):
    recs = []
    for i, d in enumerate(ds):
        recs += [(1000, 0, A, base + i), (1000 + d, 0, B, base + i)]
    return recs


def test_quantile_reference_by_hand():
    r0 = _pairs([5, -10, 15, 1]) + [(3, 0, A, 77), (4, 0, A, 77), (9, 0, B, 77), (5, 0, A, 88)]  # repeated, open: no latency
    r1 = _pairs([100, 100, 100])
    r2 = _pairs([1, 2, 3, 4, 5, 6])            # truncated below
    r3 = [(1, 0, A, 5)]                        # no pairs
    recs = [r0, r1, r2, r3]
    emitted = [len(r0), len(r1), len(r2) + 50, len(r3)]
    total, per, pairs, truncated = quantile_reference(recs, emitted, 12, A, B, (0, 500000, 1000000, 250000))
    assert pairs == 7 and truncated == 1
    # all pairs: -10 1 5 15 100 100 100
    assert total == [(-10, -10), (15, 15), (100, 100), (1, 5)]
    assert per.shape == (4, 4, 2) and per.dtype == np.int64
    assert per[0].tolist() == [[-10, -10], [1, 5], [15, 15], [-10, 1]]     # -10 1 5 15
    assert per[1].tolist() == [[100, 100]] * 4
    assert per[2].tolist() == [[I64_MAX, I64_MIN]] * 4                     # truncated: the empty entry
    assert per[3].tolist() == [[I64_MAX, I64_MIN]] * 4
    # the swapped spec negates every latency
    total, per, pairs, _ = quantile_reference(recs, emitted, 12, B, A, (500000,))
    assert total == [(-15, -15)] and per[0].tolist() == [[-5, -1]] and pairs == 7
    # nothing at all
    total, per, pairs, truncated = quantile_reference([[], []], [0, 0], 4, A, B, (0, 1000000))
    assert total == [(I64_MAX, I64_MIN)] * 2 and pairs == 0 and truncated == 0


def test_quantile_struct_and_limits_match_header(tmp_path):
    src = tmp_path / "chk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "timewarp.h"\n'
                   'int main(void) { printf("%zu %zu %zu %u\\n", sizeof(tw_quantile), offsetof(tw_quantile, lo_us), '
                   'offsetof(tw_quantile, hi_us), (unsigned)TW_MEASURE_MAX_QUANTILES); return 0; }\n')
    exe = tmp_path / "chk"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, lo, hi, mx = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == abi.QUANTILE_DTYPE.itemsize == 16
    assert abi.QUANTILE_DTYPE.fields["lo_us"][1] == lo and abi.QUANTILE_DTYPE.fields["hi_us"][1] == hi
    assert mx == abi.MEASURE_MAX_QUANTILES == 16
    assert "tw_measure_quantiles" in engine.EXPORTS and "tw_measure_quantiles_ms" in engine.EXPORTS
    text = open(os.path.join(ROOT, "include", "timewarp.h")).read()
    assert re.search(r"^#define TW_ABI_VERSION 4u$", text, re.M)   # additive: the version stays
