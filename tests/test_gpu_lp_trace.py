"""TRACE records and latency measures of node-partitioned contexts
(tw_lp_load): tw_lp_set_trace, tw_lp_read_trace, tw_lp_measure.

The context is one replica whose nodes are lanes; the lanes of a wavefront that
trace together claim their record indices with one atomic, every shard keeps
the records of its own node block, tw_lp_read_trace merges them into the
canonical order and tw_lp_measure gathers them onto one device and joins them.

Every expectation is the oracle's trace log sorted by (t, node, tag, val), and
timewarp.measures.measure_reference over it (lp_trace_shapes.py); everything is
integer, so the comparisons are exact.  Shapes: gossip with message ids at 130
nodes (128 + 2 lanes; the LDS join) and 300 nodes (two full 128-lane workgroups
and a 44-lane tail; the partition path), one case at 6,000 nodes over four
shards with record blocks of 8, and a hand-written ring whose handler holds a
fused TRACE pair."""
import ctypes as C

import numpy as np
import pytest

import lp_trace_shapes as shapes
from timewarp import isa, scenarios
from timewarp.abi import MEASURE_MAX_KEYS, TwMeasureOut, TwMeasureSpec
from timewarp.measures import first_receipts, measure_reference, trace_tuples
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.scenarios import TAG_RUMOR_FIRST, TAG_RUMOR_RECV, TAG_RUMOR_SENT

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

ERR_INVALID, ERR_STATE = -1, -5
CAP = 1 << 12
T_INF = (1 << 63) - 1
FIELDS = ("final_t", "events", "delivered", "dropped", "undeliverable", "status", "main_exc", "threads")
IDENTITY = dict(pairs=0, open_from=0, open_to=0, repeated=0, truncated=0, underflow=0, overflow=0,
                min_us=(1 << 63) - 1, max_us=-(1 << 63), sum_us=0)


def _engine(engine_mod, scn, **kw):
    return engine_mod.LPEngine(engine_mod.lp_scenario(scn), 0, scn.n_nodes, int(scn.meta["lookahead_us"]), **kw)


def _measure(e, spec=shapes.LATENCY):
    return e.lp_measure(spec["tag_from"], spec["tag_to"], lo_us=spec["lo_us"], bin_us=spec["bin_us"],
                        n_bins=spec["n_bins"])


def _same_measure(got, want, tag=""):
    (tot, hist), (rtot, rhist, _rper) = got, want
    print(tag, "gpu", tot, hist.tolist(), "ref", rtot, rhist.tolist())
    assert tot == rtot, tag
    assert hist.dtype == np.uint64 and np.array_equal(hist, rhist), tag


def _same_records(e, recs, tag=""):
    got, emitted = e.lp_trace()
    print(tag, "emitted", emitted, "oracle", len(recs))
    assert emitted == len(recs), tag
    assert trace_tuples(got) == list(recs), tag


def _same_results(e, o, tag=""):
    agg, hashes = e.lp_results()
    for f in FIELDS:
        assert int(agg[f]) == int(o.result[f]), (tag, f, int(agg[f]), o.result[f])
    assert np.array_equal(hashes, o.hashes), tag
    return agg, hashes


def _run(e, loop):
    """One run from t = 0 through the named loop of a single context."""
    e.reset()
    if loop == "run_lp":
        st = e.run_lp()
    elif loop == "run_windows":
        e.loop_begin()
        st = e.run_windows()
    else:
        raise ValueError(loop)
    assert st.done == 1 and st.err == 0
    return st


# ------------------------------------------------------------ 1, 2: records
@pytest.mark.parametrize("message_ids", [True, False], ids=["ids", "plain"])
@pytest.mark.parametrize("fork_strategy", ["fork", "inline"])
@pytest.mark.parametrize("loop", ["run_windows", "run_lp"])
def test_records_equal_the_oracle(engine_mod, oracle_mod, loop, fork_strategy, message_ids):
    scn, o, recs, _want = shapes.reference(shapes.LARGE, message_ids=message_ids, fork_strategy=fork_strategy)
    assert len(recs) >= 287 and (not message_ids or len(recs) > 2048)
    with _engine(engine_mod, scn) as e:
        _run(e, loop)
        agg_u, h_u = _same_results(e, o, "untraced")
        e.lp_set_trace(CAP)
        _run(e, loop)
        _same_records(e, recs, loop)
        agg, h = _same_results(e, o, "traced")  # tracing changes nothing else
        assert all(int(agg[f]) == int(agg_u[f]) for f in FIELDS) and np.array_equal(h, h_u)
        # the propagation curve needs no user code
        times, _hist = first_receipts(e.lp_trace()[0], TAG_RUMOR_FIRST)
        assert times.tolist() == sorted(t for t, _n, k, _v in recs if k == TAG_RUMOR_FIRST)


@pytest.mark.parametrize("fork_strategy", ["fork", "inline"])
def test_host_driven_loop_each_context_read_on_its_own(engine_mod, oracle_mod, fork_strategy):
    """The window / take_outbox / inject loop over two contexts of one process:
    each context's records are its node block's, and together they are the
    oracle's."""
    scn, o, recs, _want = shapes.reference(shapes.LARGE, message_ids=True, fork_strategy=fork_strategy)
    s, L, N = engine_mod.lp_scenario(scn), int(scn.meta["lookahead_us"]), scn.n_nodes
    bounds = [(0, 140), (140, N)]
    engines = [engine_mod.LPEngine(s, b0, b1 - b0, L) for b0, b1 in bounds]
    try:
        for e in engines:
            e.lp_set_trace(CAP).reset()
        T, windows = 0, 0
        while T < T_INF and windows < 10000:
            nexts, outs = [], []
            for e in engines:
                nt, nf = e.window(T + L)
                nexts.append(nt)
                outs.append(e.take_outbox() if nf else None)
            for o_ in outs:
                if o_ is not None and o_.size:
                    for i, (b0, b1) in enumerate(bounds):
                        mine = o_[(o_["dst"] >= b0) & (o_["dst"] < b1)]
                        if mine.size:
                            nexts[i] = min(nexts[i], engines[i].inject(mine))
            T = min(nexts)
            windows += 1
        got = []
        for e, (b0, b1) in zip(engines, bounds):
            r, emitted = e.lp_trace()
            part = [x for x in recs if b0 <= x[1] < b1]
            assert emitted == len(part) and trace_tuples(r) == part
            got += trace_tuples(r)
        assert sorted(got) == list(recs)
        agg, hashes = engine_mod._combine(engines, N)
        for f in FIELDS:
            assert int(agg[f]) == int(o.result[f]), f
        assert np.array_equal(hashes, o.hashes)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("env", [("TW_LP_GRID", "1"), ("TW_NO_GRAPH", "1")], ids=["grid_stride", "no_graph"])
def test_records_under_other_launch_paths(engine_mod, oracle_mod, monkeypatch, env):
    """TW_LP_GRID=1: one workgroup walks the work list grid-stride (the gs
    variants of the recording kernel); TW_NO_GRAPH=1: every tick's kernels are
    launched from the host."""
    monkeypatch.setenv(*env)
    scn, o, recs, want = shapes.reference(shapes.LARGE, message_ids=True)
    with _engine(engine_mod, scn) as e:
        e.lp_set_trace(CAP).set_measure_keys(4096)
        _run(e, "run_windows")
        _same_records(e, recs, env[0])
        _same_results(e, o, env[0])
        _same_measure(_measure(e), want, env[0])


# ------------------------------------------------------------------ 3: shards
def _blocks(n_nodes, k):
    base, rem = divmod(n_nodes, k)
    b0 = [i * base + min(i, rem) for i in range(k)]
    return b0 + [n_nodes]


def _cross_shard_pairs(recs, n_nodes, k):
    """pairs whose SENT and RECV records lie in different node blocks"""
    starts = np.array(_blocks(n_nodes, k)[:-1])
    sent = {v: n for _t, n, tag, v in recs if tag == TAG_RUMOR_SENT}
    cross = 0
    for _t, n, tag, v in recs:
        if tag == TAG_RUMOR_RECV and v in sent:
            a = np.searchsorted(starts, sent[v], side="right")
            b = np.searchsorted(starts, n, side="right")
            cross += int(a != b)
    return cross


@pytest.mark.parametrize("shape", [shapes.SMALL, shapes.LARGE], ids=["130", "300"])
def test_shards_agree(engine_mod, oracle_mod, shape):
    """devices=[0]*k: the records, the measure and the results do not depend on
    k, and pairs whose two records lie on different shards are pairs."""
    large = shape is shapes.LARGE
    shapes.oracle_conditions(shape, large, message_ids=True)
    scn, o, recs, want = shapes.reference(shape, message_ids=True)
    seen = []
    for k in (1, 2, 3, 4):
        assert k == 1 or _cross_shard_pairs(recs, scn.n_nodes, k) >= 1
        with _engine(engine_mod, scn, devices=[0] * k) as e:
            e.lp_set_trace(CAP)
            if large:
                e.set_measure_keys(4096)
            _run(e, "run_lp")
            _same_records(e, recs, f"k={k}")
            got = _measure(e)
            _same_measure(got, want, f"k={k}")
            _same_results(e, o, f"k={k}")
            ph = e.measure_phases_ms()
            assert e.measure_ms() > 0 and ph["count"] > 0
            assert (ph["join_large"] > 0) == large and (ph["part_scatter"] > 0) == large
            seen.append((trace_tuples(e.lp_trace()[0]), got[0], got[1].tolist()))
    assert all(s == seen[0] for s in seen[1:])


def test_one_rank_rccl_job(engine_mod, oracle_mod):
    scn, o, recs, want = shapes.reference(shapes.SMALL, message_ids=True)
    with _engine(engine_mod, scn, comm=(1, 0, engine_mod.comm_id())) as e:
        e.lp_set_trace(CAP)
        _run(e, "run_lp")
        _same_records(e, recs, "rccl x1")
        _same_measure(_measure(e), want, "rccl x1")
        _same_results(e, o, "rccl x1")


def test_four_shards_small_record_blocks(engine_mod, oracle_mod, monkeypatch):
    """test_gpu_multi.py's shape: 6,000 nodes over four shards, record blocks
    of 8, so most foreign records wait a tick in the carry buffer."""
    monkeypatch.setenv("TW_LP_XCAP", "8")
    scn = scenarios.gossip(6000, drop_log2=4, seed=21, message_ids=True)
    o = oracle_mod.run(scn, trace_cap=1 << 17)
    recs = sorted(o.traces)
    assert MEASURE_MAX_KEYS < shapes.matching_keys(recs) < (1 << 16) and len(recs) < (1 << 17)
    want = measure_reference([recs], [len(recs)], 1 << 17, shapes.LATENCY)
    assert want[0]["pairs"] == o.result["delivered"] >= 1 and want[0]["open_from"] == o.result["dropped"] >= 1
    with _engine(engine_mod, scn, devices=[0] * 4) as e:
        e.lp_set_trace(1 << 17).set_measure_keys(1 << 16)
        st = _run(e, "run_lp")
        assert st.windows > 1
        got, emitted = e.lp_trace(1 << 17)
        assert emitted == len(recs) and trace_tuples(got) == recs
        _same_measure(_measure(e), want, "6000 x4")
        _same_results(e, o, "6000 x4")


# -------------------------------------------------------------- 4: join paths
def _raw_measure(e, spec, fill=0xAB):
    """tw_lp_measure into sentinel-filled buffers: (rc, out bytes, hist bytes)"""
    cspec = TwMeasureSpec(reserved=0, **spec)
    out = (C.c_uint8 * C.sizeof(TwMeasureOut))(*([fill] * C.sizeof(TwMeasureOut)))
    hist = np.full(max(1, spec["n_bins"]), 0xABABABABABABABAB, np.uint64)
    rc = e.lib.tw_lp_measure(e.ctx, C.byref(cspec), C.cast(out, C.POINTER(TwMeasureOut)), hist.ctypes.data)
    return rc, bytes(out), hist


def test_both_join_paths(engine_mod, oracle_mod, monkeypatch):
    assert shapes.oracle_conditions(shapes.SMALL, False, message_ids=True) <= MEASURE_MAX_KEYS
    assert shapes.oracle_conditions(shapes.LARGE, True, message_ids=True) > MEASURE_MAX_KEYS
    scn, _o, recs, want = shapes.reference(shapes.SMALL, message_ids=True)
    with _engine(engine_mod, scn) as e:
        e.lp_set_trace(CAP)
        _run(e, "run_windows")
        _same_measure(_measure(e), want, "lds")
        ph = e.measure_phases_ms()
        assert ph["join"] > 0 and ph["plan"] == 0 and ph["join_large"] == 0
        # the other direction, and another histogram
        spec = dict(tag_from=TAG_RUMOR_RECV, tag_to=TAG_RUMOR_SENT, lo_us=-5000, bin_us=500, n_bins=12)
        w2 = measure_reference([list(recs)], [len(recs)], CAP, spec)
        assert w2[0]["open_to"] >= 1 and w2[0]["max_us"] < 0
        _same_measure(_measure(e, spec), w2, "lds reversed")
    scn, _o, recs, want = shapes.reference(shapes.LARGE, message_ids=True)
    with _engine(engine_mod, scn) as e:
        e.lp_set_trace(CAP)
        _run(e, "run_windows")
        rc, out, hist = _raw_measure(e, shapes.LATENCY)  # over the default key limit
        assert rc == ERR_INVALID and out == b"\xab" * len(out) and (hist == 0xABABABABABABABAB).all()
        e.set_measure_keys(4096)
        _same_measure(_measure(e), want, "partition")
        ph = e.measure_phases_ms()
        assert ph["plan"] > 0 and ph["part_count"] > 0 and ph["join_large"] > 0
        _same_records(e, recs, "after the measures")
    # small buckets (the testing hook, read when the context is made): 130 nodes through the partition path
    monkeypatch.setenv("TW_TEST_MEASURE", "0:16")
    scn, _o, recs, want = shapes.reference(shapes.SMALL, message_ids=True)
    with _engine(engine_mod, scn, devices=[0, 0]) as e:
        e.lp_set_trace(CAP)
        _run(e, "run_lp")
        _same_measure(_measure(e), want, "hook 0:16")
        assert e.measure_phases_ms()["join_large"] > 0


# --------------------------------------------------------------- 5: cap edges
def _truncated(e, E, recs, cap, tag):
    got, emitted = e.lp_trace()
    assert emitted == E, tag  # exact, past the cap
    got = trace_tuples(got)
    assert len(got) == cap, tag
    pool = {}
    for r in recs:
        pool[r] = pool.get(r, 0) + 1
    for r in got:  # distinct members of the oracle's multiset
        assert pool.get(r, 0) >= 1, (tag, r)
        pool[r] -= 1
    assert got == sorted(got), tag
    tot, hist = _measure(e)
    assert tot == dict(IDENTITY, truncated=1) and not hist.any(), tag


def test_cap_edges(engine_mod, oracle_mod):
    scn, o, recs, want = shapes.reference(shapes.SMALL, message_ids=True)
    E = len(recs)
    with _engine(engine_mod, scn) as e:
        for cap in (37, E - 1):  # no multiple of 64 and below E; one short
            e.lp_set_trace(cap)
            _run(e, "run_windows")
            _truncated(e, E, recs, cap, f"cap={cap}")
            _same_results(e, o, f"cap={cap}")
        e.lp_set_trace(E)  # exactly enough: complete
        _run(e, "run_windows")
        _same_records(e, recs, "cap=E")
        _same_measure(_measure(e), want, "cap=E")
        got, emitted = e.lp_trace(cap=10)  # a caller's buffer smaller than E
        assert emitted == E and trace_tuples(got) == list(recs[:10])
    # three shards, a cap between the largest shard's count and E: every shard kept all, truncated
    b = _blocks(scn.n_nodes, 3)
    per = [sum(1 for r in recs if b[i] <= r[1] < b[i + 1]) for i in range(3)]
    cap = E - 1
    assert max(per) < cap < E
    with _engine(engine_mod, scn, devices=[0] * 3) as e:
        e.lp_set_trace(cap)
        _run(e, "run_lp")
        _truncated(e, E, recs, cap, "3 shards")
        e.lp_set_trace(E)
        _run(e, "run_lp")
        _same_records(e, recs, "3 shards cap=E")
        _same_measure(_measure(e), want, "3 shards cap=E")


# --------------------------------------------------------- 6: reset and re-arm
def test_reset_and_rearm(engine_mod, oracle_mod):
    """The tick graph is captured per kernel variant: runs on both sides of
    every lp_set_trace switch are right."""
    scn, o, recs, want = shapes.reference(shapes.SMALL, message_ids=True)
    with _engine(engine_mod, scn) as e:
        _run(e, "run_windows")  # untraced: the graph of the plain variant
        _same_results(e, o, "before")
        with pytest.raises(engine_mod.EngineError) as ei:
            _measure(e)
        assert ei.value.code == ERR_STATE
        e.lp_set_trace(CAP)
        for i in range(2):  # survives tw_reset
            _run(e, "run_windows")
            _same_records(e, recs, f"run {i}")
            _same_measure(_measure(e), want, f"run {i}")
        e.lp_set_trace(0)
        _run(e, "run_windows")
        _same_results(e, o, "off")
        for call in (lambda: _measure(e), lambda: e.lp_trace()):
            with pytest.raises(engine_mod.EngineError) as ei:
                call()
            assert ei.value.code == ERR_STATE
        e.lp_set_trace(CAP)
        _run(e, "run_windows")
        _same_records(e, recs, "re-armed")
        _same_results(e, o, "re-armed")
        # set without a reset: the buffers are empty until the next run
        e.lp_set_trace(64)
        got, emitted = e.lp_trace()
        assert emitted == 0 and len(got) == 0
        tot, hist = _measure(e)
        assert tot == IDENTITY and not hist.any()


# ------------------------------------------------------- 7: fused TRACE pair
TAG_HOP, TAG_HOP_T = 20, 21


def _ring_flood(n_nodes=130, ttl=4, delay_us=1500, lookahead_us=1000):
    """A symmetric ring; the main thread sends ttl to both neighbours of node
    0, and every delivery traces (ttl, now) with two adjacent TRACEs -- one
    fused instruction -- and sends ttl - 1 on to both neighbours while it is
    positive.  All delays are equal, so neighbouring lanes of a wavefront trace
    in the same pass, and a node gets up to C(5, 2) = 10 copies at one time."""
    N = n_nodes
    p = Program()
    K = p.kind("hop")
    lset = p.listener_set({"hop": "on_hop"})
    c = p.function("main")
    c.wait(scenarios.for_(1000))
    c.seti(0, ttl)
    for k in range(2):
        c.link(1, k).send(1, K, 0)
    c.end()
    c = p.function("on_hop")  # r0 = ttl
    done = c.label()
    c.now(3)
    c.trace(TAG_HOP, 0).trace(TAG_HOP_T, 3)
    c.jeqi(0, 0, done)
    c.addi(0, -1)
    for k in range(2):
        c.link(1, k).send(1, K, 0)
    c.bind(done)
    c.end()
    img = p.finalize()
    topo = Topology.from_out_lists(N, [[(n + 1) % N, (n - 1) % N] for n in range(N)])
    table = np.full((2 * N, 1, 1), delay_us, np.uint32)
    return Scenario(name="ring_flood", image=img, topo=topo, n_replicas=1, main_pc=img.pc_of("main"), main_node=0,
                    link_table=table, node_listen=np.full(N, lset + 1, np.uint32), max_slots=64,
                    queue_capacity=256, meta=dict(lookahead_us=lookahead_us))


def test_fused_trace_pair(engine_mod, oracle_mod):
    scn = _ring_flood()
    w0 = scn.image.insns[:, 0].astype(np.int64)
    fused = ((w0 & 0xFF) == isa.OP_TRACE) & (((w0 >> 16) & isa.TRACE_PAIR) != 0)
    assert fused.sum() == 1
    o = oracle_mod.run(scn)
    recs = sorted(o.traces)
    assert o.result["delivered"] == 62 and len(recs) == 124 and len(set(recs)) < len(recs)  # equal records exist
    for k in (1, 2):
        with _engine(engine_mod, scn, devices=[0] * k) as e:
            e.lp_set_trace(200)
            _run(e, "run_lp")
            _same_records(e, recs, f"fused k={k}")
            _same_results(e, o, f"fused k={k}")
            e.lp_set_trace(100)  # below E: the count runs on past the cap at both TRACE sites
            _run(e, "run_lp")
            got, emitted = e.lp_trace()
            assert emitted == 124 and len(got) == 100


# ------------------------------------------------------------ 8: status codes
def _code(engine_mod, call):
    with pytest.raises(engine_mod.EngineError) as ei:
        call()
    return ei.value.code


def test_status_codes(engine_mod):
    ring = scenarios.token_ring(n_nodes=8, n_replicas=64, launch_duration=20_000_000)
    calls = (lambda e: e.lp_set_trace(64), lambda e: e.lp_trace(), lambda e: _measure(e))
    with engine_mod.Engine() as e:  # before a load
        for call in calls:
            assert _code(engine_mod, lambda: call(e)) == ERR_STATE
        e.load(ring, geometry="dense")
        for call in calls:
            assert _code(engine_mod, lambda: call(e)) == ERR_INVALID
        e.set_trace(64).reset()
        for call in calls:
            assert _code(engine_mod, lambda: call(e)) == ERR_INVALID
    with engine_mod.Engine() as e:
        e.load(scenarios.hotspot(n_senders=8, n_replicas=4, msg_num=4), geometry="lpb")
        for call in calls:
            assert _code(engine_mod, lambda: call(e)) == ERR_INVALID
        e.set_trace(64).reset()
        for call in calls:
            assert _code(engine_mod, lambda: call(e)) == ERR_INVALID
    scn = shapes.scenario(shapes.SMALL, message_ids=True)
    with _engine(engine_mod, scn) as e:
        assert _code(engine_mod, lambda: e.lp_trace()) == ERR_STATE  # tracing off
        assert _code(engine_mod, lambda: _measure(e)) == ERR_STATE
        assert _code(engine_mod, lambda: e.set_trace(64)) == ERR_INVALID  # the replica call still refuses
        assert _code(engine_mod, lambda: e.trace(0)) == ERR_INVALID
        assert _code(engine_mod, lambda: e.measure(1, 2)) == ERR_INVALID
        e.lp_set_trace(64)
        assert _code(engine_mod, lambda: e.set_trace(64)) == ERR_INVALID
        assert _code(engine_mod, lambda: e.measure(1, 2)) == ERR_INVALID
        for bad in (dict(tag_from=3, tag_to=3), dict(tag_from=1, tag_to=2, n_bins=0),
                    dict(tag_from=1, tag_to=2, n_bins=4097), dict(tag_from=1, tag_to=2, bin_us=0)):
            assert _code(engine_mod, lambda: e.lp_measure(**bad)) == ERR_INVALID, bad
        rc = e.lib.tw_lp_measure(e.ctx, None, None, None)
        assert rc == ERR_INVALID
        rc = e.lib.tw_lp_read_trace(e.ctx, None, 4, None)  # a buffer size without a buffer
        assert rc == ERR_INVALID
        assert e.lp_measure(1, 2)[0] == IDENTITY  # nothing run yet: no records
