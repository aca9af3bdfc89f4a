"""tw_measure_series' host side, CPU only: the HIP-free logic
(csrc/measure_series.hpp) in a stand-alone program built with ASan + UBSan,
timewarp.measures.series_reference (the yardstick of the GPU tests) against
hand-made records and against first_receipts on an oracle trace, and the ctypes
mirrors of the three structs against the header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lp_trace_shapes as shapes
from timewarp import abi, engine
from timewarp.measures import first_receipts, series_reference
from timewarp.scenarios import TAG_RUMOR_RECV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
A, B = 21, 22  # hand-made tags


def test_series_logic_under_sanitizers(tmp_path):
    """series_bin at the bin boundaries and at INT64_MAX, the fold over 1, 2
    and 3 shards against a direct computation, FIRST's chunk plan and the spec
    check, compiled without HIP with ASan + UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "series"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "measure_series_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "series ok" in r.stdout


# four replicas: r0 has events, a repeated id, an open id and node 3 tracing A
# three times with its earliest record last; r1 is truncated below; r2 is empty;
# r3 holds two records of one node at the same earliest time
R0 = [(10, 0, A, 100), (25, 0, B, 100),          # pair 100: t_from 10, d 15
      (12, 1, A, 101), (40, 2, B, 101),          # pair 101: t_from 12, d 28
      (30, 3, A, 102), (20, 3, A, 102), (50, 3, B, 102),   # id 102 twice under A: repeated, no pair
      (5, 3, A, 103),                            # open (and node 3's earliest A record, emitted last of its three)
      (19, 4, A, 104), (8, 4, B, 104)]           # pair 104: t_from 19, d -11
R1 = [(1, 0, A, 1), (2, 0, B, 1)] * 4
R2 = []
R3 = [(15, 7, A, 1), (15, 7, A, 2), (15, 8, A, 3), (16, 7, A, 4), (17, 7, B, 1)]
RECS = [R0, R1, R2, R3]
EMITTED = [len(R0), len(R1) + 3, 0, len(R3)]
CAP = 10


def _ref(mode, t0, width, n_bins, tag=A, tag_to=0):
    return series_reference(RECS, EMITTED, CAP, dict(tag=tag, tag_to=tag_to, mode=mode, t0_us=t0, bin_us=width,
                                                     n_bins=n_bins))


def _consistent(total, count, per, rows):
    assert int(count.sum()) + total["underflow"] + total["overflow"] == total["counted"]
    assert np.array_equal(rows.sum(axis=1) + per["underflow"] + per["overflow"], per["counted"])
    assert np.array_equal(rows.sum(axis=0), count)


def test_series_reference_events_by_hand():
    total, count, stat, per, rows = _ref("events", 10, 5, 4)        # bins [10,15) [15,20) [20,25) [25,30)
    # r0's A records at 10 12 30 20 5 19; r3's at 15 15 15 16
    assert stat is None
    assert total == dict(counted=10, underflow=1, overflow=1, truncated=1, t_min=5, t_max=30)
    assert count.tolist() == [2, 5, 1, 0] and count.dtype == np.uint64
    assert rows.tolist() == [[2, 1, 1, 0], [0] * 4, [0] * 4, [0, 4, 0, 0]]
    assert per[0].tolist() == (6, 1, 1, 0, 5, 30)
    assert per[1].tolist() == (0, 0, 0, 1, I64_MAX, I64_MIN)        # truncated: nothing else
    assert per[2].tolist() == (0, 0, 0, 0, I64_MAX, I64_MIN)        # empty
    assert per[3].tolist() == (4, 0, 0, 0, 15, 16)
    _consistent(total, count, per, rows)
    # the six boundary times of t0 = 10, bin = 5, n = 4: 9 10 14 15 29 30
    edge = [[(t, 0, A, i) for i, t in enumerate((9, 10, 14, 15, 29, 30))]]
    total, count, _stat, per, rows = series_reference(edge, [6], 6, dict(tag=A, mode="events", t0_us=10, bin_us=5,
                                                                         n_bins=4))
    assert (total["underflow"], total["overflow"]) == (1, 1) and count.tolist() == [2, 1, 0, 1]
    # tag B, one bin over everything
    total, count, _stat, per, rows = _ref("events", 0, 1 << 40, 1, tag=B)
    assert total["counted"] == 5 and count.tolist() == [5] and (total["t_min"], total["t_max"]) == (8, 50)


def test_series_reference_first_by_hand():
    total, count, stat, per, rows = _ref("first", 10, 5, 4)
    # r0: nodes 0, 1, 3, 4 first trace A at 10, 12, 5, 19; r3: nodes 7, 8 at 15 (two records at 15 count once)
    assert stat is None
    assert total == dict(counted=6, underflow=1, overflow=0, truncated=1, t_min=5, t_max=19)
    assert count.tolist() == [2, 3, 0, 0]
    assert rows.tolist() == [[2, 1, 0, 0], [0] * 4, [0] * 4, [0, 2, 0, 0]]
    assert per[0].tolist() == (4, 1, 0, 0, 5, 19) and per[3].tolist() == (2, 0, 0, 0, 15, 15)
    assert per[1].tolist() == (0, 0, 0, 1, I64_MAX, I64_MIN)
    _consistent(total, count, per, rows)
    # first_receipts over each replica's records says the same
    for r in (0, 3):
        times, hist = first_receipts(RECS[r], A, lo_us=10, bin_us=5, n_bins=4)
        assert hist.tolist() == rows[r].tolist() and len(times) == per[r]["counted"]
        assert (int(times.min()), int(times.max())) == (per[r]["t_min"], per[r]["t_max"])


def test_series_reference_latency_by_hand():
    total, count, stat, per, rows = _ref("latency", 10, 5, 2, tag_to=B)   # bins [10,15) [15,20)
    # pairs: r0's 100 (t_from 10, d 15), 101 (12, 28), 104 (19, -11); 102 is repeated, 103 open;
    # r3's id 1 (t_from 15, d 2); ids 2, 3, 4 are open
    assert total == dict(counted=4, underflow=0, overflow=0, truncated=1, t_min=10, t_max=19)
    assert count.tolist() == [2, 2]
    assert stat.tolist() == [[43, 15, 28], [-9, -11, 2]] and stat.dtype == np.int64
    assert rows.tolist() == [[2, 1], [0, 0], [0, 0], [0, 1]]
    assert per[0].tolist() == (3, 0, 0, 0, 10, 19) and per[3].tolist() == (1, 0, 0, 0, 15, 15)
    _consistent(total, count, per, rows)
    # binned so that one pair falls on either side; an empty bin keeps the empty stat
    total, count, stat, per, rows = _ref("latency", 11, 2, 3, tag_to=B)   # [11,13) [13,15) [15,17)
    assert (total["underflow"], total["overflow"]) == (1, 1) and count.tolist() == [1, 0, 1]
    assert stat.tolist() == [[28, 28, 28], [0, I64_MAX, I64_MIN], [2, 2, 2]]
    # swapped: t_from is the B record's time, d negated
    total, count, stat, _per, _rows = _ref("latency", 0, 100, 1, tag=B, tag_to=A)
    assert total["counted"] == 4 and (total["t_min"], total["t_max"]) == (8, 40)
    assert stat.tolist() == [[-34, -28, 11]]
    for bad in (dict(tag=A, tag_to=A, mode="latency"), dict(tag=A, mode="nothing"), dict(tag=A, n_bins=0),
                dict(tag=A, bin_us=0), dict(tag=A, t0_us=-1)):
        with pytest.raises(ValueError):
            series_reference(RECS, EMITTED, CAP, bad)


@pytest.mark.parametrize("shape", [shapes.SMALL, shapes.LARGE], ids=["130", "300"])
def test_first_mode_is_first_receipts_on_an_oracle_trace(oracle_mod, shape):
    _scn, _o, recs, _want = shapes.reference(shape, message_ids=True)
    spec = dict(tag=TAG_RUMOR_RECV, mode="first", t0_us=1_004_000, bin_us=2000, n_bins=6)
    total, count, _stat, per, rows = series_reference([list(recs)], [len(recs)], shapes.ORACLE_CAP, spec)
    times, hist = first_receipts(recs, TAG_RUMOR_RECV, lo_us=spec["t0_us"], bin_us=spec["bin_us"], n_bins=spec["n_bins"])
    assert np.array_equal(count, hist) and total["counted"] == len(times) >= 100
    assert (total["t_min"], total["t_max"]) == (int(times[0]), int(times[-1]))
    assert total["underflow"] == int((times < spec["t0_us"]).sum()) >= 1
    assert total["overflow"] == int((times >= spec["t0_us"] + 6 * spec["bin_us"]).sum()) >= 1
    _consistent(total, count, per, rows)


CHECK_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "timewarp.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f));
int main(void) {
  %FIELDS%
  printf("sizes %zu %zu %zu\n", sizeof(tw_series_spec), sizeof(tw_series_out), sizeof(tw_series_stat));
  printf("limits %u %u %d %d %d\n", (unsigned)TW_SERIES_MAX_BINS, (unsigned)TW_SERIES_MAX_LAT_BINS,
         (int)TW_SERIES_EVENTS, (int)TW_SERIES_FIRST, (int)TW_SERIES_LATENCY);
  return 0;
}
"""


def test_series_structs_and_limits_match_header(tmp_path):
    mirrors = (("tw_series_spec", abi.TwSeriesSpec), ("tw_series_out", abi.TwSeriesOut),
               ("tw_series_stat", abi.TwSeriesStat))
    fields = [f"F({T}, {f})" for T, cls in mirrors for f, _ in cls._fields_]
    src = tmp_path / "chk.c"
    src.write_text(CHECK_C.replace("%FIELDS%", "\n  ".join(fields)))
    exe = tmp_path / "chk"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = {l.split()[0]: tuple(int(x) for x in l.split()[1:]) for l in out}
    for T, cls in mirrors:
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert got[f"{T}.{f}"] == (d.offset, d.size), (T, f)
    assert got["sizes"] == tuple(__import__("ctypes").sizeof(cls) for _, cls in mirrors) == (40, 48, 24)
    assert got["limits"] == (abi.SERIES_MAX_BINS, abi.SERIES_MAX_LAT_BINS, abi.SERIES_EVENTS, abi.SERIES_FIRST,
                             abi.SERIES_LATENCY) == (8192, 1024, 0, 1, 2)
    assert abi.SERIES_DTYPE.itemsize == 48 and abi.SERIES_STAT_DTYPE.itemsize == 24
    for T, dt in (("tw_series_out", abi.SERIES_DTYPE), ("tw_series_stat", abi.SERIES_STAT_DTYPE)):
        for f in dt.names:
            assert dt.fields[f][1] == got[f"{T}.{f}"][0]
    for name in ("tw_measure_series", "tw_lp_measure_series", "tw_measure_series_ms"):
        assert name in engine.EXPORTS
    text = open(os.path.join(ROOT, "include", "timewarp.h")).read()
    assert re.search(r"^#define TW_ABI_VERSION 4u$", text, re.M)   # additive: the version stays
