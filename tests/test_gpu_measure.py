"""tw_measure on the GPU: the batch-wide join of two TRACE tags per message id
(bench/Network/LogReader/Main.hs:85-119) and its reduction to counts, min /
max / sum and a histogram.  Every expectation is timewarp.measures.
measure_reference fed with the oracle's trace log, never with the engine's
own records; everything is integer, so the comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import progs
from timewarp import scenarios
from timewarp.abi import MEASURE_DTYPE, MEASURE_MAX_KEYS, RESULT_FIELDS, TwMeasureOut, TwMeasureSpec
from timewarp.measures import measure_reference
from timewarp.program import Program
from timewarp.scenarios import TAG_PING, TAG_PING_SENT, TAG_PONG

pytestmark = pytest.mark.gpu

I64_MAX = (1 << 63) - 1
ERR_INVALID, ERR_STATE = -1, -5
S, M, R = 6, 12, 70          # hotspot: senders, messages per sender, replicas (not a multiple of 64)
CAP = 1 << 11
ROUND_TRIP = dict(tag_from=TAG_PING_SENT, tag_to=TAG_PONG, lo_us=2000, bin_us=250, n_bins=40)


def _oracle_traces(oracle_mod, scn, rows=None):
    """Per-replica oracle trace logs (replicas with equal `rows` entries run
    the same thing: one oracle run serves them)."""
    seen, out = {}, []
    for r in range(scn.n_replicas):
        key = r if rows is None else rows[r]
        if key not in seen:
            seen[key] = oracle_mod.run(scn, replica=r, trace_cap=1 << 14).traces
            assert len(seen[key]) < (1 << 14)
        out.append(seen[key])
    return out


def _reference(traces, cap, spec):
    return measure_reference(traces, [len(t) for t in traces], cap, spec)


def _measure(e, spec, per_replica=True):
    return e.measure(spec["tag_from"], spec["tag_to"], lo_us=spec.get("lo_us", 0), bin_us=spec.get("bin_us", 1),
                     n_bins=spec.get("n_bins", 1), per_replica=per_replica)


def _same(got, want, tag=""):
    (tot, hist, per), (rtot, rhist, rper) = got, want
    print(tag, "gpu", tot, "ref", rtot)
    assert tot == rtot, tag
    assert hist.dtype == np.uint64 and np.array_equal(hist, rhist), tag
    if rper is not None and per is not None:
        assert per.dtype == MEASURE_DTYPE
        for f in MEASURE_DTYPE.names:
            assert np.array_equal(per[f], rper[f]), (tag, f, np.flatnonzero(per[f] != rper[f])[:8])


@pytest.fixture(scope="module")
def hotspot_ref(oracle_mod):
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M)
    return scn, _oracle_traces(oracle_mod, scn)


def test_round_trip_every_geometry(engine_mod, hotspot_ref):
    scn, traces = hotspot_ref
    want = _reference(traces, CAP, ROUND_TRIP)
    assert want[0]["pairs"] == R * S * M and int(want[1].sum()) + want[0]["underflow"] + want[0]["overflow"] == R * S * M
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        res0, h0 = e.results(), e.hashes()
        got = _measure(e, ROUND_TRIP)
        _same(got, want, e.geometry())
        assert got[0]["pairs"] == R * S * M
        res1, h1 = e.results(), e.hashes()
        for f in RESULT_FIELDS:
            assert np.array_equal(res0[f], res1[f]), f
        assert np.array_equal(h0, h1)


@pytest.mark.one_geometry
def test_one_way_and_swapped(engine_mod, hotspot_ref):
    scn, traces = hotspot_ref
    one_way = dict(tag_from=TAG_PING_SENT, tag_to=TAG_PING, lo_us=1000, bin_us=100, n_bins=41)
    swapped = dict(tag_from=TAG_PONG, tag_to=TAG_PING_SENT, lo_us=0, bin_us=1000, n_bins=8)
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        got = _measure(e, one_way)
        _same(got, _reference(traces, CAP, one_way), "one way")
        # every Ping crosses its sender's link i -> S once per message: the link table's entry
        assert got[0]["sum_us"] == M * int(scn.link_table[:S, 0, :].astype(np.int64).sum())
        assert got[0]["underflow"] == 0 and got[0]["overflow"] == 0   # delays are 1000..5000 us
        got = _measure(e, swapped)                                    # a second call on the same run
        _same(got, _reference(traces, CAP, swapped), "swapped")
        assert got[0]["pairs"] == got[0]["underflow"] == R * S * M and got[0]["max_us"] < 0
        assert not got[1].any() and (got[2]["max_us"] < 0).all()


@pytest.mark.one_geometry
def test_drops_leave_open_ids(engine_mod, oracle_mod):
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M, drop_log2=2)
    traces = _oracle_traces(oracle_mod, scn)
    want = _reference(traces, CAP, ROUND_TRIP)
    assert want[0]["open_from"] > 0 and want[0]["pairs"] > 0
    assert want[0]["open_from"] + want[0]["pairs"] == R * S * M
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), want, "drops")


# ------------------------------------------------------------ scripted ids
TAG_A, TAG_B = 40, 41


def scripted(rows, n_replicas, m, pad_a=0):
    """One main thread per replica with registers (r0, r1, r2) = rows[r % len]:
    r1 iterations, iteration i tracing TAG_A with id (i * 7919) mod m + r0 and
    waiting r2 + i us; then TAG_B for the same ids in descending i.  Around
    them: id INT64_MAX (a constant) under both tags, id r0 - 1 twice under
    TAG_A (once under TAG_B), r0 - 2 twice under TAG_B (once under TAG_A),
    r0 - 3 under TAG_A only, r0 - 4 under TAG_B only, and `pad_a` more
    TAG_A-only ids.  Records per replica, all of them keys of (TAG_A, TAG_B):
    2 * r1 + 10 + pad_a."""
    p = Program()
    c = p.function("main")
    c.nstore(0, 0).nstore(1, 1).nstore(2, 2)
    c.seti(0, I64_MAX).trace(TAG_A, 0)
    c.nload(0, 0).addi(0, -1).trace(TAG_A, 0).trace(TAG_A, 0)
    c.nload(0, 0).addi(0, -2).trace(TAG_A, 0)
    c.nload(0, 0).addi(0, -3).trace(TAG_A, 0)
    for k in range(pad_a):
        c.nload(0, 0).addi(0, -5 - k).trace(TAG_A, 0)
    c.seti(3, 0)
    top, done = c.here(), c.label()
    c.nload(1, 1).jle(1, 3, done)
    c.mov(0, 3).muli(0, 7919).modi(0, m).nload(1, 0).add(0, 1).trace(TAG_A, 0)
    c.nload(1, 2).add(1, 3).wait_reg(1)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    c.nload(3, 1)
    top2, fin = c.here(), c.label()
    c.jeqi(3, 0, fin)
    c.addi(3, -1)
    c.mov(0, 3).muli(0, 7919).modi(0, m).nload(1, 0).add(0, 1).trace(TAG_B, 0)
    c.jmp(top2)
    c.bind(fin)
    c.nload(0, 0).addi(0, -1).trace(TAG_B, 0)
    c.nload(0, 0).addi(0, -2).trace(TAG_B, 0).trace(TAG_B, 0)
    c.nload(0, 0).addi(0, -4).trace(TAG_B, 0)
    c.seti(0, I64_MAX).trace(TAG_B, 0)
    c.end()
    scn = progs.single(p, "scripted_ids", n_replicas=n_replicas)
    keys = [tuple(rows[r % len(rows)]) for r in range(n_replicas)]
    scn.main_regs = np.array([list(k) + [0] for k in keys], dtype=np.int64)
    return scn, keys


@pytest.mark.one_geometry
def test_scripted_ids(engine_mod, oracle_mod):
    # (id base r0, iterations r1, wait base r2); m = 997 < 1000: ids 0..2 of
    # the long row come up twice per tag (repeated); one base is negative
    rows = [(100, 0, 5), (7, 1, 0), (-5000, 2, 9), (1 << 40, 37, 3), (0, 72, 1), (12345, 1000, 2)]
    scn, keys = scripted(rows, 257, 997)   # 257: crosses a 256-lane workgroup of the count pass
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert [len(t) for t in traces[:6]] == [2 * r1 + 10 for _, r1, _ in rows]
    a_to_b = dict(tag_from=TAG_A, tag_to=TAG_B, lo_us=100, bin_us=100, n_bins=4096)   # the largest histogram
    b_to_a = dict(tag_from=TAG_B, tag_to=TAG_A, lo_us=-300000, bin_us=7, n_bins=1000)
    absent = dict(tag_from=50, tag_to=51, lo_us=0, bin_us=1, n_bins=3)                # replicas with 0 keys
    want = _reference(traces, CAP * 2, a_to_b)
    assert want[0]["repeated"] > 2 * 257 and want[0]["open_from"] == want[0]["open_to"] == 257
    assert want[0]["underflow"] > 0 and want[0]["overflow"] > 0 and want[1].any()
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP * 2).reset()
        e.run()
        _same(_measure(e, a_to_b), want, "A->B")
        _same(_measure(e, b_to_a), _reference(traces, CAP * 2, b_to_a), "B->A")
        got = _measure(e, absent)
        _same(got, _reference(traces, CAP * 2, absent), "absent tags")
        assert got[0]["pairs"] == 0 and got[0]["min_us"] == I64_MAX and got[0]["max_us"] == -I64_MAX - 1


def _raw_measure(e, spec, n_bins, n):
    """tw_measure straight through ctypes into buffers prefilled with 0xA5."""
    tot = TwMeasureOut()
    C.memset(C.addressof(tot), 0xA5, C.sizeof(tot))
    hist = np.full(n_bins, 0xA5A5A5A5A5A5A5A5, np.uint64)
    per = np.frombuffer(bytearray(b"\xa5" * (MEASURE_DTYPE.itemsize * n)), MEASURE_DTYPE)
    rc = e.lib.tw_measure(e.ctx, C.byref(spec), C.byref(tot), hist.ctypes.data, per.ctypes.data, n)
    return rc, bytes(tot), hist, per


@pytest.mark.one_geometry
def test_capacity_edges(engine_mod, oracle_mod):
    full = (MEASURE_MAX_KEYS - 10) // 2
    rows = [(1000, full, 1), (50, 5, 2), (9, 0, 0)]
    spec = dict(tag_from=TAG_A, tag_to=TAG_B, lo_us=0, bin_us=4096, n_bins=64)
    cspec = TwMeasureSpec(tag_from=TAG_A, tag_to=TAG_B, n_bins=64, reserved=0, lo_us=0, bin_us=4096)
    # exactly TW_MEASURE_MAX_KEYS matching records in replica 0: passes
    scn, keys = scripted(rows, 3, 4099)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert len(traces[0]) == MEASURE_MAX_KEYS
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(2 * CAP).reset()
        e.run()
        want = _reference(traces, 2 * CAP, spec)
        assert want[0]["pairs"] == full + 5 + 3 and want[0]["truncated"] == 0
        _same(_measure(e, spec), want, "exactly MAX_KEYS")
        # a trace cap below what replica 0 (2048) emits: it is truncated and
        # excluded; replicas 1 (20 records) and 2 (10) are unchanged
        e.set_trace(100).reset()
        e.run()
        got = _measure(e, spec)
        wt = _reference(traces, 100, spec)
        _same(got, wt, "truncated")
        assert got[0]["truncated"] == 1 and got[2]["truncated"].tolist() == [1, 0, 0]
        for f in MEASURE_DTYPE.names:
            assert np.array_equal(got[2][f][1:], want[2][f][1:]), f
    # one record more: TW_ERR_INVALID, decided before the join, nothing written
    scn, keys = scripted(rows, 3, 4099, pad_a=1)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert len(traces[0]) == MEASURE_MAX_KEYS + 1
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(2 * CAP).reset()
        e.run()
        rc, tot, hist, per = _raw_measure(e, cspec, 64, 3)
        assert rc == ERR_INVALID
        assert tot == b"\xa5" * C.sizeof(TwMeasureOut) and (hist == 0xA5A5A5A5A5A5A5A5).all()
        assert per.tobytes() == b"\xa5" * (MEASURE_DTYPE.itemsize * 3)
        with pytest.raises(engine_mod.EngineError) as ei:
            _measure(e, spec)
        assert ei.value.code == ERR_INVALID
        # the key limit binds non-truncated replicas only
        e.set_trace(100).reset()
        e.run()
        _same(_measure(e, spec), _reference(traces, 100, spec), "over the limit but truncated")


@pytest.mark.one_geometry
def test_errors(engine_mod):
    def code(fn):
        with pytest.raises(engine_mod.EngineError) as ei:
            fn()
        return ei.value.code

    scn = scenarios.hotspot(n_senders=2, n_replicas=4, msg_num=3)
    with engine_mod.Engine() as e:
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG)) == ERR_STATE       # nothing loaded
        e.load(scn)
        e.run()
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG)) == ERR_STATE       # tracing is off
        e.set_trace(64).reset()
        e.run()
        assert e.measure(TAG_PING_SENT, TAG_PONG)[0]["pairs"] == 4 * 2 * 3
        assert code(lambda: e.measure(TAG_PONG, TAG_PONG)) == ERR_INVALID
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG, n_bins=0)) == ERR_INVALID
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG, n_bins=4097)) == ERR_INVALID
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG, bin_us=0)) == ERR_INVALID
        spec = TwMeasureSpec(tag_from=TAG_PING_SENT, tag_to=TAG_PONG, n_bins=1, reserved=1, lo_us=0, bin_us=1)
        assert _raw_measure(e, spec, 1, 4)[0] == ERR_INVALID                       # reserved != 0
        spec.reserved = 0
        assert _raw_measure(e, spec, 1, 3)[0] == ERR_INVALID                       # n is not the replica count
        assert _raw_measure(e, spec, 1, 4)[0] == 0
        e.set_trace(0)
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG)) == ERR_STATE       # tracing off again
    lpb = scenarios.hotspot(n_senders=16, n_replicas=64, msg_num=30)
    with engine_mod.Engine() as e:
        e.load(lpb, geometry="lpb")
        assert code(lambda: e.measure(TAG_PING_SENT, TAG_PONG)) == ERR_INVALID     # as tw_set_trace


@pytest.mark.one_geometry
def test_two_shards_of_one_gpu(engine_mod, hotspot_ref):
    scn, traces = hotspot_ref
    want = _reference(traces, CAP, ROUND_TRIP)
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        one = _measure(e, ROUND_TRIP)
    with engine_mod.Engine(devices=[0, 0]) as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        two = _measure(e, ROUND_TRIP)
        assert e.measure_ms() > 0
    _same(two, one, "two shards vs one")
    _same(two, want, "two shards vs reference")
