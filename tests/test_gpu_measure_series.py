"""tw_measure_series on the GPU: TRACE records binned over virtual time -- the
records of a tag (events), each node's first record of it (first) and a latency
by the time its pair opened (latency) -- for the batch and per replica.  Every
expectation is timewarp.measures.series_reference fed with the oracle's trace
log, never with the engine's own records; everything is integer and compared
for equality.

A replica context emits a node's records in time order, so there the earliest
record of a node is always the first one emitted; the binning kernels walk the
records with many lanes in no particular order, which is what the several
records per node of the scripted program and of gossip exercise.  The
restatement's own handling of an earliest record emitted last is checked by
hand in test_series_host.py."""
import ctypes as C

import numpy as np
import pytest

import lp_trace_shapes as shapes
import progs
from timewarp import abi, scenarios
from timewarp.abi import RESULT_FIELDS, SERIES_DTYPE, SERIES_MAX_BINS, SERIES_MAX_LAT_BINS, SERIES_STAT_DTYPE
from timewarp.measures import first_receipts, series_reference
from timewarp.program import Program
from timewarp.scenarios import TAG_PING_SENT, TAG_PONG, TAG_RUMOR_RECV, TAG_RUMOR_SENT

pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
ERR_INVALID, ERR_STATE = -1, -5
S, M, R = 6, 12, 70          # hotspot: senders, messages per sender, replicas (not a multiple of 64)
CAP = 1 << 11
TAG_A, TAG_B = 40, 41
EMPTY = (0, 0, 0, 0, I64_MAX, I64_MIN)


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


def _spec(mode, tag, t0_us, bin_us, n_bins, tag_to=0):
    return dict(mode=mode, tag=tag, tag_to=tag_to, t0_us=t0_us, bin_us=bin_us, n_bins=n_bins)


_REFS = {}


def _reference(name, traces, cap, spec):
    """series_reference over the oracle's records, computed once per (records, cap, spec)."""
    key = (name, cap, tuple(sorted(spec.items())))
    if key not in _REFS:
        _REFS[key] = series_reference(traces, [len(t) for t in traces], cap, spec)
    return _REFS[key]


def _call(e, spec, per_replica):
    return e.measure_series(spec["tag"], spec["t0_us"], spec["bin_us"], spec["n_bins"], mode=spec["mode"],
                            tag_to=spec["tag_to"], per_replica=per_replica)


def _same(got, want, tag=""):
    (tot, count, stat, per, rows), (rtot, rcount, rstat, rper, rrows) = got, want
    print(tag, "gpu", tot, count.tolist()[:16], "ref", rtot, rcount.tolist()[:16])
    assert tot == rtot, tag
    assert count.dtype == np.uint64 and np.array_equal(count, rcount), tag
    assert int(count.sum()) + tot["underflow"] + tot["overflow"] == tot["counted"], tag
    if rstat is None:
        assert stat is None, tag
    else:
        assert stat.dtype == SERIES_STAT_DTYPE, tag
        for i, f in enumerate(("sum_us", "min_us", "max_us")):
            assert np.array_equal(stat[f], rstat[:, i]), (tag, f)
    if per is not None:
        assert per.dtype == SERIES_DTYPE and per.tobytes() == rper.tobytes(), (tag, np.argwhere(per != rper)[:8])
        assert rows.dtype == np.uint64 and np.array_equal(rows, rrows), (tag, np.argwhere(rows != rrows)[:8])


def _check(e, name, traces, cap, spec, tag=""):
    want = _reference(name, traces, cap, spec)
    got = _call(e, spec, True)
    _same(got, want, f"{tag} {spec['mode']} {spec['tag']}")
    only_total = _call(e, spec, False)                               # without the per-replica outputs
    assert only_total[3] is None and only_total[4] is None
    _same(only_total, want, f"{tag} {spec['mode']} {spec['tag']} (total only)")
    return got, want


# ----------------------------------------------------------------- hotspot
HOT_SPECS = (_spec("events", TAG_PING_SENT, 2000, 1500, 10), _spec("events", TAG_PONG, 2000, 1500, 10),
             _spec("latency", TAG_PING_SENT, 2000, 1500, 6, tag_to=TAG_PONG),
             # every sender's first send is at 1,001 .. 1,006 us in every replica; the first pongs come at
             # 3,271 .. 10,768 us, different in every replica: bins that leave both ends outside
             _spec("first", TAG_PING_SENT, 1003, 1, 2), _spec("first", TAG_PONG, 4000, 1500, 4))


@pytest.fixture(scope="module")
def hotspot_ref(oracle_mod):
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M)
    traces = _oracle_traces(oracle_mod, scn)
    # what the specs rest on, on the oracle, before any engine runs
    sent = [t for tr in traces for t, _n, k, _v in tr if k == TAG_PING_SENT]
    pong_last = [max(t for t, _n, k, _v in tr if k == TAG_PONG) for tr in traces]
    assert (min(sent), max(sent)) == (1001, 12017) and len(sent) == R * S * M
    # (the replicas' last pongs: 18,661 us in replica 0, 18,112 .. 21,779 us over all: behind the last bin)
    assert pong_last[0] == 18661 and (min(pong_last), max(pong_last)) == (18112, 21779) and min(pong_last) > 2000 + 10 * 1500
    for spec in HOT_SPECS:
        tot, count, _stat, per, _rows = _reference("hotspot", traces, CAP, spec)
        assert tot["truncated"] == 0 and int(count.sum()) >= 1
        if spec["mode"] != "first":
            # sends before 2,000 us are the underflow, pongs behind 17,000 us the
            # overflow; latency bins the sends into 6 bins: both ends
            assert tot["underflow"] >= 1 or spec["tag"] == TAG_PONG, spec
            assert tot["overflow"] >= 1 or (spec["mode"], spec["tag"]) == ("events", TAG_PING_SENT), spec
            assert tot["counted"] == R * S * M
        else:
            # the six sender nodes of every replica; the pongs at times that differ between replicas
            assert (per["counted"] == S).all() and tot["underflow"] >= 1 and tot["overflow"] >= 1
            assert spec["tag"] == TAG_PING_SENT or len(set(per["t_min"].tolist())) > R // 2
    return scn, traces


def test_hotspot_every_geometry(engine_mod, hotspot_ref):
    scn, traces = hotspot_ref
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        res0, h0 = e.results(), e.hashes()
        m0 = e.measure(TAG_PING_SENT, TAG_PONG, lo_us=2000, bin_us=250, n_bins=40, per_replica=True)
        for spec in HOT_SPECS:
            _check(e, "hotspot", traces, CAP, spec, str(e.geometry()))
        # against tw_measure on the device: counted is its pairs, and one bin over everything folds its min / max / sum
        (tot, count, stat, per, rows), _ = _check(e, "hotspot", traces, CAP,
                                                  _spec("latency", TAG_PING_SENT, 0, 1 << 40, 1, tag_to=TAG_PONG), "one bin")
        mt, _, mper = m0
        assert tot["counted"] == mt["pairs"] == R * S * M and count.tolist() == [mt["pairs"]]
        assert stat[0].tolist() == (mt["sum_us"], mt["min_us"], mt["max_us"])
        assert np.array_equal(per["counted"], mper["pairs"]) and np.array_equal(rows[:, 0], mper["pairs"])
        ph = e.measure_series_ms()
        print("phases", ph)
        assert ph["join_emit"] > 0 and ph["latency_fold"] > 0 and ph["first_fill"] == 0 and ph["bin"] == 0
        _call(e, HOT_SPECS[3], False)
        ph = e.measure_series_ms()
        assert ph["first_fill"] > 0 and ph["bin"] > 0 and ph["join_emit"] == 0 and ph["latency_fold"] == 0
        _call(e, HOT_SPECS[0], False)
        ph = e.measure_series_ms()
        assert ph["bin"] > 0 and ph["first_fill"] == 0 and ph["join_emit"] == 0
        # the calls changed nothing: results, hashes and a following tw_measure
        res1, h1 = e.results(), e.hashes()
        for f in RESULT_FIELDS:
            assert np.array_equal(res0[f], res1[f]), f
        assert np.array_equal(h0, h1)
        m1 = e.measure(TAG_PING_SENT, TAG_PONG, lo_us=2000, bin_us=250, n_bins=40, per_replica=True)
        assert m0[0] == m1[0] and np.array_equal(m0[1], m1[1]) and m0[2].tobytes() == m1[2].tobytes()


@pytest.mark.one_geometry
def test_drops_leave_uneven_replicas(engine_mod, oracle_mod):
    # a dropped link loses all of a sender's messages: replicas of unequal counts, some with no pair
    odd_m = 11
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=odd_m, drop_log2=2)
    traces = _oracle_traces(oracle_mod, scn)
    lat = _spec("latency", TAG_PING_SENT, 2000, 1500, 6, tag_to=TAG_PONG)
    tot, _count, _stat, per, _rows = _reference("drops", traces, CAP, lat)
    assert 0 < tot["counted"] < R * S * odd_m and len(set(per["counted"].tolist())) > 2 and 0 in per["counted"]
    assert per[per["counted"] == 0]["t_min"].tolist() == [I64_MAX] * int((per["counted"] == 0).sum())
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        _check(e, "drops", traces, CAP, lat, "drops")
        _check(e, "drops", traces, CAP, _spec("events", TAG_PONG, 2000, 1500, 10), "drops")
        (_tot, _c, _s, fper, _r), _ = _check(e, "drops", traces, CAP, _spec("first", TAG_PONG, 2000, 1500, 10), "drops")
        assert 0 in fper["counted"] and S in fper["counted"]       # senders that never heard a Pong are no items


# ------------------------------------------------------- a scripted program
T0, BIN, NB = 1000, 100, 4
EDGES = (T0 - 1, T0, T0 + BIN - 1, T0 + BIN, T0 + NB * BIN - 1, T0 + NB * BIN)
# (start, n, w): after `start` us, n times TAG_A of id i, w us later TAG_B of id i, w us later the next
ROWS = [(t, 1, 7) for t in EDGES] + [(1, 0, 1),      # no record
                                     (500, 25, 3),   # 50 records: over the cap below
                                     (1000, 15, 10)]  # the one node traces TAG_A 15 times, 20 us apart
SCRIPTED_R, SCRIPTED_CAP = 67, 40


def scripted(rows, n_replicas):
    p = Program()
    c = p.function("main")
    c.nstore(0, 0).nstore(1, 1).nstore(2, 2)
    c.nload(1, 0).wait_reg(1)
    c.seti(3, 0)
    top, done = c.here(), c.label()
    c.nload(1, 1).jle(1, 3, done)
    c.mov(0, 3).trace(TAG_A, 0).nload(1, 2).wait_reg(1)
    c.mov(0, 3).trace(TAG_B, 0).nload(1, 2).wait_reg(1)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    c.end()
    scn = progs.single(p, "scripted_series", n_replicas=n_replicas)
    keys = [tuple(rows[r % len(rows)]) for r in range(n_replicas)]
    scn.main_regs = np.array([list(k) + [0] for k in keys], dtype=np.int64)
    return scn, keys


@pytest.fixture(scope="module")
def scripted_ref(oracle_mod):
    scn, keys = scripted(ROWS, SCRIPTED_R)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert [len(t) for t in traces[:9]] == [2] * 6 + [0, 50, 30]
    for r, t in enumerate(EDGES):                     # a TAG_A record exactly at every boundary time
        assert [x[0] for x in traces[r] if x[2] == TAG_A] == [t]
    assert [x[0] for x in traces[8] if x[2] == TAG_A] == [1000 + 20 * i for i in range(15)]
    return scn, traces


def _reps(k):
    return sum(1 for r in range(SCRIPTED_R) if r % len(ROWS) == k)


@pytest.mark.one_geometry
def test_scripted_boundaries(engine_mod, scripted_ref):
    scn, traces = scripted_ref
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(SCRIPTED_CAP).reset()
        e.run()
        (tot, count, _s, per, rows), _ = _check(e, "scripted", traces, SCRIPTED_CAP, _spec("events", TAG_A, T0, BIN, NB))
        # by hand: the boundary replicas, the empty one, the truncated one, the node of 15 records
        assert [rows[r].tolist() for r in range(6)] == [[0] * 4, [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0],
                                                        [0, 0, 0, 1], [0] * 4]
        assert per[0].tolist() == (1, 1, 0, 0, T0 - 1, T0 - 1)
        assert per[5].tolist() == (1, 0, 1, 0, T0 + NB * BIN, T0 + NB * BIN)
        assert per[6].tolist() == EMPTY and per[7].tolist() == (0, 0, 0, 1, I64_MAX, I64_MIN)
        assert rows[8].tolist() == [5, 5, 5, 0] and per[8].tolist() == (15, 0, 0, 0, 1000, 1280)
        assert tot["truncated"] == _reps(7) and tot["underflow"] == _reps(0) and tot["overflow"] == _reps(5)
        (_t, _c, _s, per, rows), _ = _check(e, "scripted", traces, SCRIPTED_CAP, _spec("first", TAG_A, T0, BIN, NB))
        assert rows[8].tolist() == [1, 0, 0, 0] and per[8].tolist() == (1, 0, 0, 0, 1000, 1000)
        assert per[7].tolist() == (0, 0, 0, 1, I64_MAX, I64_MIN) and per[6].tolist() == EMPTY
        (_t, _c, stat, per, rows), _ = _check(e, "scripted", traces, SCRIPTED_CAP,
                                              _spec("latency", TAG_A, T0, BIN, NB, tag_to=TAG_B))
        assert rows[8].tolist() == [5, 5, 5, 0] and (stat["min_us"] == np.array([7, 7, 10, 7])).all()
        assert (stat["max_us"] == np.array([10, 10, 10, 7])).all()
        # one bin, and each mode's maximum; bins of 1 us; tags nobody traced
        for mode, most in (("events", SERIES_MAX_BINS), ("first", SERIES_MAX_BINS), ("latency", SERIES_MAX_LAT_BINS)):
            tag_to = TAG_B if mode == "latency" else 0
            _check(e, "scripted", traces, SCRIPTED_CAP, _spec(mode, TAG_A, T0, BIN, 1, tag_to=tag_to), "one bin")
            _check(e, "scripted", traces, SCRIPTED_CAP, _spec(mode, TAG_A, T0 - 1, 1, most, tag_to=tag_to), "most bins")
            _check(e, "scripted", traces, SCRIPTED_CAP, _spec(mode, TAG_B, 0, 1 << 40, 3, tag_to=TAG_A if tag_to else 0),
                   "wide bins")
            tot, count, _s, per, rows = _call(e, _spec(mode, 50, 0, 10, 5, tag_to=51 if tag_to else 0), True)
            assert tot == dict(counted=0, underflow=0, overflow=0, truncated=_reps(7), t_min=I64_MAX, t_max=I64_MIN)
            assert not count.any() and not rows.any() and per[0].tolist() == EMPTY


@pytest.mark.one_geometry
def test_one_replica(engine_mod, oracle_mod):
    scn, keys = scripted([ROWS[8]], 1)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert len(traces[0]) == 30
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(SCRIPTED_CAP).reset()
        e.run()
        for mode in ("events", "first", "latency"):
            _check(e, "one", traces, SCRIPTED_CAP, _spec(mode, TAG_A, T0 + 30, 50, 3, tag_to=TAG_B if mode == "latency" else 0),
                   "R = 1")
        e.set_trace(29).reset()                                   # one record short: truncated, nothing else
        e.run()
        for mode in ("events", "first", "latency"):
            (tot, count, _s, per, _r), _ = _check(e, "one", traces, 29,
                                                  _spec(mode, TAG_A, T0, 50, 3, tag_to=TAG_B if mode == "latency" else 0), "cut")
            assert tot == dict(counted=0, underflow=0, overflow=0, truncated=1, t_min=I64_MAX, t_max=I64_MIN)
            assert not count.any() and per[0].tolist() == (0, 0, 0, 1, I64_MAX, I64_MIN)


# ------------------------------------------------------ other kinds of context
@pytest.mark.one_geometry
@pytest.mark.parametrize("trace_batch", [False, True])
def test_traced_lpb_context(engine_mod, oracle_mod, trace_batch):
    scn = scenarios.hotspot(n_senders=16, n_replicas=64, msg_num=10, drop_log2=2)
    traces = _oracle_traces(oracle_mod, scn)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(CAP).set_trace_batch(trace_batch).reset()
        assert e.geometry() == "lpb"
        e.run()
        for spec in (_spec("events", TAG_PONG, 2000, 1500, 10), _spec("first", TAG_PONG, 2000, 1500, 10),
                     _spec("first", TAG_PING_SENT, 1003, 1, 7),
                     _spec("latency", TAG_PING_SENT, 2000, 1500, 6, tag_to=TAG_PONG)):
            (tot, _c, _s, _p, _r), _ = _check(e, "lpb", traces, CAP, spec, f"lpb batch={trace_batch}")
            assert tot["counted"] > 0 and tot["truncated"] == 0


GOSSIP = dict(t0_us=1_004_000, bin_us=2000, n_bins=6)
GOSSIP_ORACLE = {130: (455, 126, 10, 5, 5), 300: (1045, 288, 15, 1, 45)}   # records, nodes, most per node, under, over


def _lp_engine(engine_mod, scn, **kw):
    return engine_mod.LPEngine(engine_mod.lp_scenario(scn), 0, scn.n_nodes, int(scn.meta["lookahead_us"]), **kw)


def _lp_call(e, spec):
    return e.lp_measure_series(spec["tag"], spec["t0_us"], spec["bin_us"], spec["n_bins"], mode=spec["mode"],
                               tag_to=spec["tag_to"])


@pytest.mark.one_geometry
@pytest.mark.parametrize("shape", [shapes.SMALL, shapes.LARGE], ids=["130", "300"])
def test_node_partitioned_gossip(engine_mod, oracle_mod, shape):
    scn, _o, recs, _want = shapes.reference(shape, message_ids=True)
    name = f"gossip{scn.n_nodes}"
    specs = [_spec(mode, TAG_RUMOR_RECV, **GOSSIP) for mode in ("first", "events")]
    specs.append(_spec("latency", TAG_RUMOR_SENT, tag_to=TAG_RUMOR_RECV, **GOSSIP))
    wants = [_reference(name, [list(recs)], shapes.ORACLE_CAP, s) for s in specs]
    # on the oracle, before any engine runs
    per_node = {}
    for _t, node, k, _v in recs:
        if k == TAG_RUMOR_RECV:
            per_node[node] = per_node.get(node, 0) + 1
    ftot, fcount = wants[0][0], wants[0][1]
    assert (sum(per_node.values()), len(per_node), max(per_node.values()), ftot["underflow"],
            ftot["overflow"]) == GOSSIP_ORACLE[scn.n_nodes]
    assert ftot["counted"] == len(per_node) and wants[1][0]["counted"] == sum(per_node.values())
    times, hist = first_receipts(recs, TAG_RUMOR_RECV, lo_us=GOSSIP["t0_us"], bin_us=GOSSIP["bin_us"],
                                 n_bins=GOSSIP["n_bins"])
    assert np.array_equal(hist, fcount) and len(times) == ftot["counted"]
    large = shape is shapes.LARGE
    assert (shapes.matching_keys(recs) > abi.MEASURE_MAX_KEYS) == large      # LARGE: the join's partition path
    seen = []
    for k in (1, 3):
        with _lp_engine(engine_mod, scn, devices=[0] * k) as e:
            e.lp_set_trace(1 << 12)
            if large:
                e.set_measure_keys(4096)
            e.reset()
            st = e.run_lp()
            assert st.done == 1 and st.err == 0
            agg0, hashes0 = e.lp_results()
            m0 = e.lp_measure(TAG_RUMOR_SENT, TAG_RUMOR_RECV, lo_us=2000, bin_us=250, n_bins=8)
            got = []
            for spec, want in zip(specs, wants):
                tot, count, stat = _lp_call(e, spec)
                _same((tot, count, stat, None, None), want, f"{name} k={k} {spec['mode']}")
                got.append((tot, count.tolist(), None if stat is None else stat.tobytes()))
            assert np.array_equal(got[0][1], hist.tolist())                   # first == first_receipts
            assert got[2][0]["counted"] == m0[0]["pairs"]
            ph = e.measure_series_ms()
            assert ph["join_emit"] > 0 and ph["latency_fold"] > 0
            agg1, hashes1 = e.lp_results()
            m1 = e.lp_measure(TAG_RUMOR_SENT, TAG_RUMOR_RECV, lo_us=2000, bin_us=250, n_bins=8)
            assert all(int(agg0[f]) == int(agg1[f]) for f in RESULT_FIELDS) and np.array_equal(hashes0, hashes1)
            assert m0[0] == m1[0] and np.array_equal(m0[1], m1[1])
            seen.append(got)
    assert seen[0] == seen[1]


@pytest.mark.one_geometry
def test_node_partitioned_truncated_and_statuses(engine_mod, oracle_mod):
    scn, _o, recs, _want = shapes.reference(shapes.SMALL, message_ids=True)
    spec = _spec("first", TAG_RUMOR_RECV, **GOSSIP)
    for k in (1, 3):
        with _lp_engine(engine_mod, scn, devices=[0] * k) as e:
            assert _raw(e, spec, 0, lp=True) == (ERR_STATE, True)             # tracing off
            assert _raw(e, spec, 0) == (ERR_INVALID, True)                    # tw_measure_series: the other kind
            e.lp_set_trace(len(recs) - 1)                                     # E > cap, over all shards
            e.reset()
            assert e.run_lp().done == 1
            for mode in ("events", "first", "latency"):
                s = _spec(mode, TAG_RUMOR_SENT, tag_to=TAG_RUMOR_RECV if mode == "latency" else 0, **GOSSIP)
                tot, count, stat = _lp_call(e, s)
                assert tot == dict(counted=0, underflow=0, overflow=0, truncated=1, t_min=I64_MAX, t_max=I64_MIN)
                assert not count.any() and (stat is None or stat.tolist() == [(0, I64_MAX, I64_MIN)] * 6)
            assert _raw(e, dict(spec, n_bins=0), 0, lp=True) == (ERR_INVALID, True)
            assert _raw(e, dict(spec, tag_to=5), 0, lp=True) == (ERR_INVALID, True)
            assert _raw(e, spec, 0, lp=True, stat=True) == (ERR_INVALID, True)   # stat outside latency
            e.lp_set_trace(len(recs))                                         # exactly enough: complete
            e.reset()
            assert e.run_lp().done == 1
            tot, count, _stat = _lp_call(e, spec)
            _same((tot, count, None, None, None), _reference("gossip130", [list(recs)], shapes.ORACLE_CAP, spec), "exact cap")


@pytest.mark.one_geometry
def test_two_shards_of_one_gpu(engine_mod, hotspot_ref, scripted_ref):
    for name, (scn, traces), cap, specs in (
            ("hotspot", hotspot_ref, CAP, HOT_SPECS),
            ("scripted", scripted_ref, SCRIPTED_CAP, (_spec("events", TAG_A, T0, BIN, NB), _spec("first", TAG_A, T0, BIN, NB),
                                                      _spec("latency", TAG_A, T0, BIN, NB, tag_to=TAG_B)))):
        with engine_mod.Engine() as e:
            e.load(scn).set_trace(cap).reset()
            e.run()
            one = [_call(e, s, True) for s in specs]
        with engine_mod.Engine(devices=[0, 0]) as e:
            e.load(scn).set_trace(cap).reset()
            e.run()
            for s, o in zip(specs, one):
                (tot, count, stat, per, rows), _ = _check(e, name, traces, cap, s, "two shards")
                assert tot == o[0] and count.tobytes() == o[1].tobytes() and per.tobytes() == o[3].tobytes()
                assert rows.tobytes() == o[4].tobytes() and (stat is None or stat.tobytes() == o[2].tobytes())


@pytest.mark.one_geometry
@pytest.mark.parametrize("entries", ["16", "50"])
def test_first_in_several_chunks(engine_mod, hotspot_ref, monkeypatch, entries):
    """TW_TEST_SERIES lowers the first-time table to `entries` (replica, node)
    pairs at a time, read when the context is made: the hotspot's 8 nodes per
    replica then take 2 (6) replicas a chunk, 35 (12) chunks, the last one
    shorter.  The outputs are the same."""
    scn, traces = hotspot_ref
    assert scn.n_nodes == 8
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        whole = [_call(e, s, True) for s in HOT_SPECS[3:]]
    monkeypatch.setenv("TW_TEST_SERIES", entries)
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        for s, w in zip(HOT_SPECS[3:], whole):
            (tot, count, _s, per, rows), _ = _check(e, "hotspot", traces, CAP, s, f"chunks of {entries}")
            assert tot == w[0] and count.tobytes() == w[1].tobytes() and per.tobytes() == w[3].tobytes()
            assert rows.tobytes() == w[4].tobytes()
        _check(e, "hotspot", traces, CAP, HOT_SPECS[0], "events under the hook")
    monkeypatch.setenv("TW_TEST_SERIES", "7")                    # fewer entries than one replica's nodes: refused
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        assert _raw(e, HOT_SPECS[3], R) == (ERR_INVALID, True)
        assert _raw(e, HOT_SPECS[0], R)[0] == 0                  # the other modes keep no table


# ------------------------------------------------------------------ refusals
def _raw(e, spec, n, lp=False, stat=None, null_spec=False, reserved=0):
    """tw_measure_series (lp: tw_lp_measure_series) straight through ctypes
    into prefilled buffers; returns the status and whether every output is
    untouched.  stat: given iff the mode is latency, unless said otherwise."""
    mode = abi.SERIES_MODES.get(spec["mode"], spec["mode"])
    s = abi.TwSeriesSpec(tag=spec["tag"], tag_to=spec["tag_to"], mode=mode, n_bins=spec["n_bins"], t0_us=spec["t0_us"],
                         bin_us=spec["bin_us"], reserved=reserved)
    most = SERIES_MAX_BINS + 8
    bufs = [bytearray(b"\xa5" * k) for k in (48, 8 * most, 24 * most, 48 * max(n, 1), 8 * most * max(n, 1))]
    tot, count, st, per, rows = ((C.c_char * len(b)).from_buffer(b) for b in bufs)
    if stat is None:
        stat = mode == abi.SERIES_LATENCY
    sp = None if null_spec else C.byref(s)
    if lp:
        rc = e.lib.tw_lp_measure_series(e.ctx, sp, C.cast(tot, C.POINTER(abi.TwSeriesOut)), C.addressof(count),
                                        C.addressof(st) if stat else None)
    else:
        rc = e.lib.tw_measure_series(e.ctx, sp, C.cast(tot, C.POINTER(abi.TwSeriesOut)), C.addressof(count),
                                     C.addressof(st) if stat else None, C.addressof(per), C.addressof(rows), n)
    return rc, all(bytes(b) == b"\xa5" * len(b) for b in bufs)


@pytest.mark.one_geometry
def test_refusals_write_nothing(engine_mod):
    scn = scenarios.hotspot(n_senders=2, n_replicas=4, msg_num=3)
    ev = _spec("events", TAG_PONG, 2000, 1500, 10)
    lat = _spec("latency", TAG_PING_SENT, 2000, 1500, 6, tag_to=TAG_PONG)
    with engine_mod.Engine() as e:
        assert _raw(e, ev, 4) == (ERR_STATE, True)                              # nothing loaded
        assert _raw(e, ev, 0, lp=True) == (ERR_STATE, True)
        e.load(scn)
        e.run()
        assert _raw(e, ev, 4) == (ERR_STATE, True)                              # tracing is off
        e.set_trace(64).reset()
        e.run()
        for bad in (dict(ev, mode=3), dict(ev, n_bins=0), dict(ev, n_bins=SERIES_MAX_BINS + 1),
                    dict(ev, mode="first", n_bins=SERIES_MAX_BINS + 1), dict(lat, n_bins=SERIES_MAX_LAT_BINS + 1),
                    dict(ev, t0_us=-1), dict(ev, bin_us=0), dict(ev, bin_us=-5), dict(lat, tag_to=TAG_PING_SENT),
                    dict(ev, tag_to=TAG_PING_SENT), dict(ev, mode="first", tag_to=TAG_PING_SENT)):
            assert _raw(e, bad, 4) == (ERR_INVALID, True), bad
        assert _raw(e, ev, 4, reserved=1) == (ERR_INVALID, True)
        assert _raw(e, ev, 4, null_spec=True) == (ERR_INVALID, True)
        assert _raw(e, ev, 4, stat=True) == (ERR_INVALID, True)                 # stat outside latency
        assert _raw(e, dict(ev, mode="first"), 4, stat=True) == (ERR_INVALID, True)
        assert _raw(e, ev, 3) == (ERR_INVALID, True) and _raw(e, lat, 5) == (ERR_INVALID, True)   # another n
        assert _raw(e, ev, 0, lp=True) == (ERR_INVALID, True)                   # tw_lp_measure_series: the other kind
        for good in (ev, lat, dict(ev, mode="first"), dict(ev, n_bins=SERIES_MAX_BINS),
                     dict(lat, n_bins=SERIES_MAX_LAT_BINS)):
            rc, clean = _raw(e, good, 4)
            assert rc == 0 and not clean, good
        assert _raw(e, lat, 4, stat=False)[0] == 0                              # stat is optional
        with pytest.raises(engine_mod.EngineError) as ei:
            e.measure_series(TAG_PONG, 0, 1, 10, mode="latency", tag_to=TAG_PONG)
        assert ei.value.code == ERR_INVALID
        tot, count, stat, per, rows = e.measure_series(TAG_PONG, 0, 1 << 40, 1)                   # the context stays usable
        assert tot["counted"] == 4 * 2 * 3 == int(count[0]) and stat is None and per is None and rows is None
        e.set_trace(0)
        assert _raw(e, ev, 4) == (ERR_STATE, True)                              # tracing off again
    lpb = scenarios.hotspot(n_senders=16, n_replicas=64, msg_num=30)
    with engine_mod.Engine() as e:
        e.load(lpb, geometry="lpb")
        assert _raw(e, ev, 64) == (ERR_INVALID, True)                           # lpb, tracing off


@pytest.mark.one_geometry
def test_overfull_replica_is_a_status(engine_mod, oracle_mod):
    """latency keeps tw_measure's key limit: a replica of more matching records
    than TW_MEASURE_MAX_KEYS is refused with nothing written until
    tw_set_measure_keys raises the limit; then it goes down the partition path."""
    p = Program()
    c = p.function("main")
    c.seti(3, 0).seti(2, 1100).seti(1, 1)
    top, done = c.here(), c.label()
    c.jle(2, 3, done)
    c.mov(0, 3).trace(TAG_A, 0).wait_reg(1).trace(TAG_B, 0)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    c.end()
    scn = progs.single(p, "many_keys", n_replicas=2)
    traces = _oracle_traces(oracle_mod, scn, rows=[0, 0])
    assert len(traces[0]) == 2200 > abi.MEASURE_MAX_KEYS
    lat = _spec("latency", TAG_A, 100, 100, 8, tag_to=TAG_B)
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(4096).reset()
        e.run()
        assert _raw(e, lat, 2) == (ERR_INVALID, True)
        _check(e, "many", traces, 4096, _spec("events", TAG_A, 100, 100, 8), "the other modes have no key limit")
        e.set_measure_keys(4096)
        (tot, _c, stat, _p, _r), _ = _check(e, "many", traces, 4096, lat, "partition path")
        assert tot["counted"] == 2200 and (stat["min_us"] == 1).all() and (stat["max_us"] == 1).all()
