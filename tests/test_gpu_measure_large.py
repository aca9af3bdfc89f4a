"""tw_measure beyond TW_MEASURE_MAX_KEYS matching records per replica
(tw_set_measure_keys): replicas too large for the LDS sort are hash-partitioned
by id into HBM buckets and aggregated per bucket in an LDS table.  As in
test_gpu_measure.py every expectation is timewarp.measures.measure_reference
fed with the oracle's trace log, and the comparison is exact.  The trace layout
per geometry is pinned there: everything here runs once."""
import ctypes as C

import numpy as np
import pytest

import progs
from test_gpu_measure import (CAP, ROUND_TRIP, TAG_A, TAG_B, _measure, _oracle_traces, _raw_measure, _reference, _same,
                              scripted)
from timewarp import scenarios
from timewarp.abi import (MEASURE_DTYPE, MEASURE_MAX_KEYS, MEASURE_MAX_KEYS_LARGE, RESULT_FIELDS, TwMeasureOut,
                          TwMeasureSpec)
from timewarp.program import Program

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
ERR_INVALID = -1
BIG_CAP = 8192
A_TO_B = dict(tag_from=TAG_A, tag_to=TAG_B, lo_us=100, bin_us=100, n_bins=4096)   # the largest histogram
B_TO_A = dict(tag_from=TAG_B, tag_to=TAG_A, lo_us=-300000, bin_us=7, n_bins=1000)


def scripted_rows(rows, n_replicas, m):
    """test_gpu_measure.scripted with a fourth register per row: 0 as there;
    1: every iteration's id is r0 itself (one id, r1 times per tag); 2: one
    more TAG_A-only id, r0 - 5 (an odd record count).  Records per replica,
    all of them keys of (TAG_A, TAG_B): 2 * r1 + 10 (+ 1 with 2)."""
    p = Program()
    c = p.function("main")
    c.nstore(0, 0).nstore(1, 1).nstore(2, 2).nstore(3, 3)
    c.seti(0, I64_MAX).trace(TAG_A, 0)
    c.nload(0, 0).addi(0, -1).trace(TAG_A, 0).trace(TAG_A, 0)
    c.nload(0, 0).addi(0, -2).trace(TAG_A, 0)
    c.nload(0, 0).addi(0, -3).trace(TAG_A, 0)
    no_pad = c.label()
    c.nload(1, 3).jnei(1, 2, no_pad)
    c.nload(0, 0).addi(0, -5).trace(TAG_A, 0)
    c.bind(no_pad)

    def trace_id(tag):   # r3 = i
        keep = c.label()
        c.mov(0, 3).muli(0, 7919).modi(0, m)
        c.nload(1, 3).jnei(1, 1, keep)
        c.seti(0, 0)
        c.bind(keep)
        c.nload(1, 0).add(0, 1).trace(tag, 0)

    c.seti(3, 0)
    top, done = c.here(), c.label()
    c.nload(1, 1).jle(1, 3, done)
    trace_id(TAG_A)
    c.nload(1, 2).add(1, 3).wait_reg(1)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    c.nload(3, 1)
    top2, fin = c.here(), c.label()
    c.jeqi(3, 0, fin)
    c.addi(3, -1)
    trace_id(TAG_B)
    c.jmp(top2)
    c.bind(fin)
    c.nload(0, 0).addi(0, -1).trace(TAG_B, 0)
    c.nload(0, 0).addi(0, -2).trace(TAG_B, 0).trace(TAG_B, 0)
    c.nload(0, 0).addi(0, -4).trace(TAG_B, 0)
    c.seti(0, I64_MAX).trace(TAG_B, 0)
    c.end()
    scn = progs.single(p, "scripted_rows", n_replicas=n_replicas)
    keys = [tuple(rows[r % len(rows)]) for r in range(n_replicas)]
    scn.main_regs = np.array([list(k) for k in keys], dtype=np.int64)
    return scn, keys


# (id base r0, iterations r1, wait base r2, mode); m = 997: the rows of 1200 and
# more iterations bring every id up more than once per tag
MIXED_ROWS = [
    (100, 5, 5, 0),            # 20 keys
    (7, 1019, 1, 0),           # exactly 2,048: the LDS path's largest
    (9000, 1019, 1, 2),        # 2,049, the smallest large replica: 4 buckets
    (12345, 3000, 2, 0),       # 6,010 keys over 8 buckets, ids repeated about three times per tag
    (555, 3000, 1, 1),         # 6,010 keys, one id 3,000 times per tag: one bucket holds them all
    (-5000, 1200, 9, 0),       # a negative id base
    (1 << 40, 1500, 3, 0),     # and a large one
    (77, 4100, 1, 0),          # 8,210 records: over the trace cap, truncated
]
MIXED_KEYS = [20, 2048, 2049, 6010, 6010, 2410, 3010, 8210]


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    scn, keys = scripted_rows(MIXED_ROWS, 257, 997)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert [len(t) for t in traces[:8]] == MIXED_KEYS
    return scn, traces, {"ab": _reference(traces, BIG_CAP, A_TO_B), "ba": _reference(traces, BIG_CAP, B_TO_A)}


def test_mixed_batch(engine_mod, mixed):
    scn, traces, want = mixed
    tot = want["ab"][0]
    assert tot["truncated"] == 32 and tot["pairs"] > 0 and tot["repeated"] > 257 * 2
    assert tot["open_from"] == 257 - 32 + 32 and tot["open_to"] == 257 - 32     # r0 - 3 (and r0 - 5 in row 2), r0 - 4
    assert tot["underflow"] > 0 and tot["overflow"] > 0 and want["ab"][1].any()
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).reset()
        e.run()
        res0, h0 = e.results(), e.hashes()
        with pytest.raises(engine_mod.EngineError) as ei:     # the default setting refuses the batch
            _measure(e, A_TO_B)
        assert ei.value.code == ERR_INVALID
        e.set_measure_keys(8192)
        got = _measure(e, A_TO_B)
        _same(got, want["ab"], "A->B")
        assert e.measure_ms() > 0
        ph = e.measure_phases_ms()
        print("phases", ph)
        assert ph["part_scatter"] > 0 and ph["join_large"] > 0 and abs(sum(ph.values()) - e.measure_ms()) < 1e-6
        # the row of one id 3,000 times per tag: that id is one `repeated`
        assert got[2]["repeated"][4] == 3 and got[2]["pairs"][4] == 1
        res1, h1 = e.results(), e.hashes()
        for f in RESULT_FIELDS:
            assert np.array_equal(res0[f], res1[f]), f
        assert np.array_equal(h0, h1)
        _same(_measure(e, B_TO_A), want["ba"], "B->A")        # a second call, another spec, the same run
        _same(_measure(e, A_TO_B, per_replica=False), want["ab"], "A->B without per_replica")


def test_limits(engine_mod, mixed):
    scn, traces, want = mixed
    cspec = TwMeasureSpec(reserved=0, **A_TO_B)
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).reset()
        e.run()
        e.set_measure_keys(4096)                              # the rows of 6,010 keys are over it
        rc, tot, hist, per = _raw_measure(e, cspec, 4096, 257)
        assert rc == ERR_INVALID
        assert tot == b"\xa5" * C.sizeof(TwMeasureOut) and (hist == 0xA5A5A5A5A5A5A5A5).all()
        assert per.tobytes() == b"\xa5" * (MEASURE_DTYPE.itemsize * 257)
        e.set_measure_keys(8192)
        _same(_measure(e, A_TO_B), want["ab"], "after raising the limit")
        for bad in (MEASURE_MAX_KEYS - 1, MEASURE_MAX_KEYS_LARGE + 1, 0):
            with pytest.raises(engine_mod.EngineError) as ei:
                e.set_measure_keys(bad)
            assert ei.value.code == ERR_INVALID
        _same(_measure(e, A_TO_B), want["ab"], "a refused value changes nothing")
        e.set_measure_keys(MEASURE_MAX_KEYS_LARGE).set_measure_keys(MEASURE_MAX_KEYS).set_measure_keys(8192)
        # the setting outlives a load of another scenario (and set_trace, reset)
        e.load(scenarios.hotspot(n_senders=2, n_replicas=4, msg_num=3)).set_trace(64).reset()
        e.run()
        assert e.measure(scenarios.TAG_PING_SENT, scenarios.TAG_PONG)[0]["pairs"] == 4 * 2 * 3
        e.load(scn).set_trace(BIG_CAP).reset()
        e.run()
        _same(_measure(e, A_TO_B), want["ab"], "after another load")


def test_special_ids(engine_mod, oracle_mod):
    """INT64_MIN (the bucket table's empty mark), INT64_MAX, 0 and -1 once
    under each tag, N us apart, in replicas that are otherwise large."""
    N = 1100
    p = Program()
    c = p.function("main")
    special = (I64_MIN, I64_MAX, 0, -1)
    for v in special:
        c.seti(0, v).trace(TAG_A, 0)
    c.seti(3, 0).seti(2, N).seti(1, 1)
    top, done = c.here(), c.label()
    c.jle(2, 3, done)
    c.mov(0, 3).addi(0, 1000).trace(TAG_A, 0)     # id 1000 + i at t = i
    c.wait_reg(1)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    for v in special:                             # t = N
        c.seti(0, v).trace(TAG_B, 0)
    top2, fin = c.here(), c.label()
    c.jeqi(3, 0, fin)
    c.addi(3, -1)
    c.mov(0, 3).addi(0, 1000).trace(TAG_B, 0)
    c.jmp(top2)
    c.bind(fin)
    c.end()
    R = 3
    scn = progs.single(p, "special_ids", n_replicas=R)
    traces = _oracle_traces(oracle_mod, scn, rows=[0] * R)
    assert len(traces[0]) == 2 * N + 8 > MEASURE_MAX_KEYS
    spec = dict(tag_from=TAG_A, tag_to=TAG_B, lo_us=N, bin_us=1, n_bins=2)
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        e.run()
        got = _measure(e, spec)
        _same(got, _reference(traces, BIG_CAP, spec), "special ids")
        # d = N - i for id 1000 + i, and N for the four special ids
        assert got[0]["pairs"] == R * (N + 4) and got[0]["repeated"] == got[0]["open_from"] == got[0]["open_to"] == 0
        assert got[0]["min_us"] == 1 and got[0]["max_us"] == N and got[0]["sum_us"] == R * (N * (N + 1) // 2 + 4 * N)
        assert got[1].tolist() == [R * 5, 0] and got[0]["underflow"] == R * (N - 1)


@pytest.mark.parametrize("drop_log2", [0, 2])
def test_hotspot_replica_geometry(engine_mod, oracle_mod, drop_log2):
    S, M, R = 6, 200, 70                       # 2,400 keys of the round trip per replica
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M, drop_log2=drop_log2)
    traces = _oracle_traces(oracle_mod, scn)
    want = _reference(traces, BIG_CAP, ROUND_TRIP)
    if drop_log2:
        assert want[0]["open_from"] > 0 and want[0]["pairs"] > 0
        assert want[0]["open_from"] + want[0]["pairs"] == R * S * M
    else:
        assert want[0]["pairs"] == R * S * M
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), want, f"hotspot drop_log2={drop_log2}")


def test_hotspot_lpb(engine_mod, oracle_mod):
    S, M, R = 16, 80, 64                       # 2,560 keys per replica
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M)
    traces = _oracle_traces(oracle_mod, scn)
    want = _reference(traces, BIG_CAP, ROUND_TRIP)
    assert want[0]["pairs"] == R * S * M
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        assert e.geometry() == "lpb"
        e.run()
        _same(_measure(e, ROUND_TRIP), want, "lpb")


def test_two_shards_of_one_gpu(engine_mod, mixed):
    scn, traces, want = mixed
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        e.run()
        one = _measure(e, B_TO_A)
    with engine_mod.Engine(devices=[0, 0]) as e:   # replicas 0..127 and 128..256: large ones in both
        e.load(scn).set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        e.run()
        two = _measure(e, B_TO_A)
        assert e.measure_ms() > 0
    _same(two, one, "two shards vs one")
    _same(two, want["ba"], "two shards vs reference")


def test_hook_forces_the_partition_path(engine_mod, oracle_mod, monkeypatch):
    """TW_TEST_MEASURE=0:1024: every replica with a key takes the partition
    path, one bucket each."""
    hot = scenarios.hotspot(n_senders=6, n_replicas=70, msg_num=12)
    rows = [(100, 0, 5), (7, 1, 0), (-5000, 2, 9), (1 << 40, 37, 3), (0, 72, 1), (12345, 1000, 2)]
    scr, keys = scripted(rows, 257, 997)
    cases = [(hot, _oracle_traces(oracle_mod, hot), CAP, ROUND_TRIP),
             (scr, _oracle_traces(oracle_mod, scr, rows=keys), 2 * CAP, A_TO_B),
             (scr, None, 2 * CAP, B_TO_A),
             (scr, None, 2 * CAP, dict(tag_from=50, tag_to=51, lo_us=0, bin_us=1, n_bins=3))]   # no large replica
    got = {}
    for hook in ("0:1024", None):
        if hook:
            monkeypatch.setenv("TW_TEST_MEASURE", hook)
        else:
            monkeypatch.delenv("TW_TEST_MEASURE")
        with engine_mod.Engine() as e:             # (the hook is read when the context is made)
            loaded = None
            for i, (scn, traces, cap, spec) in enumerate(cases):
                if scn is not loaded:
                    e.load(scn).set_trace(cap).reset()
                    e.run()
                    loaded, tr = scn, traces
                got[hook, i] = _measure(e, spec)
                _same(got[hook, i], _reference(tr, cap, spec), f"hook {hook} case {i}")
                ph = e.measure_phases_ms()
                assert (ph["join_large"] > 0) == (bool(hook) and i < 3), ph   # (case 3: no replica holds a key)
    for i in range(len(cases)):
        _same(got["0:1024", i], got[None, i], f"hook against none, case {i}")


def test_hook_table_overflow_is_a_status(engine_mod, oracle_mod, monkeypatch):
    """TW_TEST_MEASURE=2048:1048576: a replica of 6,010 keys is one bucket of
    about 3,000 distinct ids, more than its table's 2,048 slots:
    TW_ERR_INVALID, nothing written."""
    rows = [(1000, 3000, 1, 0), (50, 5, 2, 0), (9, 0, 0, 0)]
    scn, keys = scripted_rows(rows, 3, 4099)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert len(traces[0]) == 6010 and len({t[3] for t in traces[0]}) > 2048 + 5
    spec = dict(tag_from=TAG_A, tag_to=TAG_B, lo_us=0, bin_us=4096, n_bins=64)
    cspec = TwMeasureSpec(reserved=0, **spec)
    monkeypatch.setenv("TW_TEST_MEASURE", "2048:1048576")
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        e.run()
        rc, tot, hist, per = _raw_measure(e, cspec, 64, 3)
        assert rc == ERR_INVALID
        assert tot == b"\xa5" * C.sizeof(TwMeasureOut) and (hist == 0xA5A5A5A5A5A5A5A5).all()
        assert per.tobytes() == b"\xa5" * (MEASURE_DTYPE.itemsize * 3)
        # the context stays usable: with replica 0 truncated the others are measured
        e.set_trace(100).reset()
        e.run()
        _same(_measure(e, spec), _reference(traces, 100, spec), "after the overflow")
    monkeypatch.delenv("TW_TEST_MEASURE")
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(BIG_CAP).set_measure_keys(BIG_CAP).reset()
        e.run()
        _same(_measure(e, spec), _reference(traces, BIG_CAP, spec), "without the hook")
