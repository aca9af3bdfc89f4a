"""tw_measure's host side, CPU only: the restatement of its rules
(timewarp.measures.pair_latencies / measure_reference, the yardstick of the
GPU tests) on the oracle's hotspot traces and on hand-made records, the
ctypes mirror of its two structs against the header, and the HIP-free shard
combining (csrc/measure_combine.hpp) in a stand-alone program built with
ASan + UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from timewarp import abi, scenarios
from timewarp.measures import measure_reference, measures_from_trace, pair_latencies, trace_tuples
from timewarp.scenarios import TAG_PING, TAG_PING_SENT, TAG_PONG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
A, B = 21, 22  # hand-made tags


@pytest.fixture(scope="module")
def hotspot_traces(oracle_mod):
    S, M = 4, 6
    scn = scenarios.hotspot(n_senders=S, n_replicas=3, msg_num=M)
    return S, M, scn, [oracle_mod.run(scn, replica=r, trace_cap=1 << 12).traces for r in range(3)]


def test_one_way_latency_is_the_link_delay(hotspot_traces):
    S, M, scn, traces = hotspot_traces
    for rep, tr in enumerate(traces):
        lat, counts = pair_latencies(tr, TAG_PING_SENT, TAG_PING)
        assert counts == {"pairs": S * M, "open_from": 0, "open_to": 0, "repeated": 0}
        # ascending id order; id mid was sent by sender (mid - 1) % S over link (mid - 1) % S
        assert lat == [int(scn.link_table[(mid - 1) % S, 0, rep]) for mid in range(1, S * M + 1)]


def test_round_trip_equals_measures_from_trace(hotspot_traces):
    S, M, _scn, traces = hotspot_traces
    for tr in traces:
        ms = measures_from_trace(trace_tuples(tr))
        lat, counts = pair_latencies(tr, TAG_PING_SENT, TAG_PONG)
        assert counts["pairs"] == S * M
        assert lat == [ms[mid]["PongReceived"] - ms[mid]["PingSent"] for mid in sorted(ms)]


HAND = [
    (10, 0, A, 1), (25, 1, B, 1),                  # a pair, d = 15
    (11, 0, A, 2),                                 # open-from
    (12, 0, B, 3),                                 # open-to
    (13, 0, A, 4), (14, 0, A, 4), (30, 1, B, 4),   # repeated tag_from
    (15, 0, A, 5), (31, 1, B, 5), (32, 1, B, 5),   # repeated tag_to
    (16, 0, 99, 1), (17, 0, 99, 6),                # another tag: not part of the join
    (40, 0, B, -7), (50, 0, A, -7),                # a pair with a negative id and d = -10
    (60, 0, A, I64_MAX), (61, 0, B, I64_MAX),      # INT64_MAX is an id like any other
    (70, 0, A, 0), (75, 0, B, 0),                  # and so is 0
]


def test_class_counts_on_hand_made_records():
    lat, counts = pair_latencies(HAND, A, B)
    assert counts == {"pairs": 4, "open_from": 1, "open_to": 1, "repeated": 2}
    assert lat == [-10, 5, 15, 1]  # ids -7, 0, 1, INT64_MAX
    # swapped tags: the same classes with from / to exchanged and the signs flipped
    lat2, counts2 = pair_latencies(HAND, B, A)
    assert counts2 == {"pairs": 4, "open_from": 1, "open_to": 1, "repeated": 2}
    assert lat2 == [10, -5, -15, -1]
    with pytest.raises(ValueError):
        pair_latencies(HAND, A, A)


def test_reference_totals_and_truncation():
    spec = dict(tag_from=A, tag_to=B, lo_us=0, bin_us=4, n_bins=4)
    # replica 1 emitted more than the cap: it counts in `truncated` alone
    total, hist, per = measure_reference([HAND, HAND, []], [len(HAND), len(HAND) + 50, 0], len(HAND), spec)
    assert total == dict(pairs=4, open_from=1, open_to=1, repeated=2, truncated=1, underflow=1, overflow=0,
                         min_us=-10, max_us=15, sum_us=11)
    assert hist.dtype == np.uint64 and hist.tolist() == [1, 1, 0, 1]  # d = 1, 5, 15
    assert per.dtype == abi.MEASURE_DTYPE
    assert per[1]["truncated"] == 1 and per[1]["pairs"] == 0 and per[1]["repeated"] == 0
    assert per[1]["min_us"] == I64_MAX and per[1]["max_us"] == I64_MIN
    assert per[2]["pairs"] == 0 and per[2]["min_us"] == I64_MAX and per[2]["max_us"] == I64_MIN
    assert per[0]["sum_us"] == 11 and per[0]["min_us"] == -10 and per[0]["max_us"] == 15


@pytest.mark.parametrize("lo,width,n_bins", [(100, 10, 5), (-30, 7, 3), (0, 1, 1)])
def test_histogram_edges(lo, width, n_bins):
    end = lo + n_bins * width
    ds = [lo, lo - 1, end - 1, end, -(abs(lo) + 5)]
    recs = []
    for i, d in enumerate(ds):
        recs += [(1000, 0, A, i), (1000 + d, 0, B, i)]
    total, hist, _per = measure_reference([recs], [len(recs)], len(recs),
                                          dict(tag_from=A, tag_to=B, lo_us=lo, bin_us=width, n_bins=n_bins))
    # d == lo: first bin; lo - 1 and the negative one: underflow; end - 1: last bin; end: overflow
    assert total["pairs"] == 5 and total["underflow"] == 2 and total["overflow"] == 1
    want = [0] * n_bins
    want[0] += 1
    want[n_bins - 1] += 1
    assert hist.tolist() == want
    assert total["min_us"] == min(ds) and total["max_us"] == max(ds) and total["sum_us"] == sum(ds)


CHECK_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "timewarp.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("tw_measure_spec %zu\ntw_measure_out %zu\nmax_keys %u\nmax_bins %u\n", sizeof(tw_measure_spec),
         sizeof(tw_measure_out), (unsigned)TW_MEASURE_MAX_KEYS, (unsigned)TW_MEASURE_MAX_BINS);
  %FIELDS%
  return 0;
}
"""


def test_measure_struct_layout_matches_ctypes(tmp_path):
    pairs = (("tw_measure_spec", abi.TwMeasureSpec), ("tw_measure_out", abi.TwMeasureOut))
    fields = [f"F({T}, {f})" for T, cls in pairs for f, _ in cls._fields_]
    src = tmp_path / "chk.c"
    src.write_text(CHECK_C.replace("%FIELDS%", "\n  ".join(fields)))
    exe = tmp_path / "chk"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.split("\n") if line)
    for T, cls in pairs:
        assert int(got[T]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{T}.{f}"]) == getattr(cls, f).offset, (T, f)
    assert int(got["tw_measure_out"]) == abi.MEASURE_DTYPE.itemsize
    for f, _ in abi.TwMeasureOut._fields_:
        assert abi.MEASURE_DTYPE.fields[f][1] == getattr(abi.TwMeasureOut, f).offset
    assert int(got["max_keys"]) == abi.MEASURE_MAX_KEYS >= 2048
    assert int(got["max_bins"]) == abi.MEASURE_MAX_BINS >= 4096


def test_shard_combine_under_sanitizers(tmp_path):
    """The host logic tw_measure folds its shards with (sum the totals, min of
    the mins, max of the maxes, per-replica blocks placed by first replica),
    compiled without HIP into its own program with ASan + UBSan."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "combine"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tests", "measure_combine_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "combine ok" in r.stdout
