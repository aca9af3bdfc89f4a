"""TRACE records and tw_measure in the batched node-partitioned mode
(tw_lpb_load, geometry "lpb"): every (node, replica) pair is a lane, and a
record claims its replica's next index from one counter in HBM.

Every expectation is timewarp.measures.measure_reference (or the sorted log
itself) fed with the oracle's trace log, never the engine's own replica-mode
output; everything is integer, so the comparisons are exact.  Shapes: a small
hotspot (the senders' pongs arrive through light inboxes, drained in the event
kernel), a receiver of 64 senders (hundreds of records per window, sorted by
tw_lp_due; tracing keeps them off tw_lp_batch), the same with drops and a cap
below some replicas' counts, the inline fork strategy, and the token ring,
whose inboxes are all light and whose observer runs in phase 1 of every
window."""
from collections import Counter

import numpy as np
import pytest

from timewarp import scenarios
from timewarp.abi import MEASURE_DTYPE, MEASURE_MAX_KEYS, RESULT_FIELDS
from timewarp.measures import measure_reference, trace_tuples
from timewarp.scenarios import TAG_GOT_TOKEN, TAG_NOTE, TAG_PING_SENT, TAG_PONG

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

ERR_INVALID = -1
ROUND_TRIP = dict(tag_from=TAG_PING_SENT, tag_to=TAG_PONG, lo_us=2000, bin_us=250, n_bins=40)
TOKEN_NOTE = dict(tag_from=TAG_GOT_TOKEN, tag_to=TAG_NOTE, lo_us=0, bin_us=1000, n_bins=16)


def _oracle_traces(oracle_mod, scn):
    out = []
    for r in range(scn.n_replicas):
        out.append(oracle_mod.run(scn, replica=r, trace_cap=1 << 14).traces)
        assert len(out[-1]) < (1 << 14)
    return out


def _reference(traces, cap, spec):
    return measure_reference(traces, [len(t) for t in traces], cap, spec)


def _measure(e, spec):
    return e.measure(spec["tag_from"], spec["tag_to"], lo_us=spec["lo_us"], bin_us=spec["bin_us"],
                     n_bins=spec["n_bins"], per_replica=True)


def _same(got, want, tag=""):
    (tot, hist, per), (rtot, rhist, rper) = got, want
    print(tag, "gpu", tot, "ref", rtot)
    assert tot == rtot, tag
    assert hist.dtype == np.uint64 and np.array_equal(hist, rhist), tag
    assert per.dtype == MEASURE_DTYPE
    for f in MEASURE_DTYPE.names:
        assert np.array_equal(per[f], rper[f]), (tag, f, np.flatnonzero(per[f] != rper[f])[:8])


def _keys(recs, spec):
    return sum(1 for _t, _n, tag, _v in recs if tag in (spec["tag_from"], spec["tag_to"]))


@pytest.fixture(scope="module")
def light_ref(oracle_mod):
    scn = scenarios.hotspot(n_senders=8, n_replicas=64, msg_num=30)
    return scn, _oracle_traces(oracle_mod, scn)


@pytest.fixture(scope="module")
def heavy_drop_ref(oracle_mod):
    scn = scenarios.hotspot(n_senders=64, n_replicas=32, msg_num=12, drop_log2=2)
    return scn, _oracle_traces(oracle_mod, scn)


@pytest.fixture(scope="module")
def ring_ref(oracle_mod):
    scn = scenarios.token_ring(n_nodes=16, n_replicas=64, launch_duration=40_000_000, drop_log2=3)
    return scn, _oracle_traces(oracle_mod, scn)


def _untraced(engine_mod, scn):
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").reset()
        e.run()
        return e.results(), e.hashes(), e.lpb_batch()


def test_light_inboxes(engine_mod, light_ref):
    scn, traces = light_ref
    want = _reference(traces, 2048, ROUND_TRIP)
    assert want[0]["pairs"] == 15360 and all(len(t) == 960 for t in traces)
    res_u, h_u, _ = _untraced(engine_mod, scn)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(2048).reset()
        assert e.geometry() == "lpb"
        e.run()
        res0, h0 = e.results(), e.hashes()
        _same(_measure(e, ROUND_TRIP), want, "light")
        res1, h1 = e.results(), e.hashes()
        for f in RESULT_FIELDS:
            assert np.array_equal(res0[f], res1[f]), f      # unchanged by the measure call
            assert np.array_equal(res0[f], res_u[f]), f     # and what an untraced run gives
        assert np.array_equal(h0, h1) and np.array_equal(h0, h_u)


def test_heavy_receiver_runs_on_the_chain(engine_mod, oracle_mod):
    scn = scenarios.hotspot(n_senders=64, n_replicas=32, msg_num=12)
    traces = _oracle_traces(oracle_mod, scn)
    want = _reference(traces, 4096, ROUND_TRIP)
    assert all(len(t) == 3072 for t in traces) and want[0]["pairs"] == 24576
    assert max(_keys(t, ROUND_TRIP) for t in traces) == 1536 <= MEASURE_MAX_KEYS
    res_u, h_u, (batched_u, due_u) = _untraced(engine_mod, scn)
    print("untraced: batched", batched_u, "due", due_u)
    assert batched_u > 0                      # the receiver is heavy and its handler batchable
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(4096).reset()
        e.run()
        batched, due = e.lpb_batch()
        print("traced: batched", batched, "due", due)
        assert due > 0 and batched == 0       # the due path, with tw_lp_batch off
        _same(_measure(e, ROUND_TRIP), want, "heavy")
        res, h = e.results(), e.hashes()
        for f in RESULT_FIELDS:
            assert np.array_equal(res[f], res_u[f]), f
        assert np.array_equal(h, h_u)


def test_drops_and_truncation(engine_mod, heavy_drop_ref):
    scn, traces = heavy_drop_ref
    emitted = [len(t) for t in traces]
    full = _reference(traces, 4096, ROUND_TRIP)
    assert full[0]["pairs"] == 13776 and full[0]["open_from"] == 10800 and full[0]["truncated"] == 0
    cap = int(np.median(emitted))
    cut = _reference(traces, cap, ROUND_TRIP)
    print("median emitted", cap, "truncated replicas", cut[0]["truncated"])
    assert 1 <= cut[0]["truncated"] < scn.n_replicas      # some replicas truncated, some not
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(4096).reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), full, "drops, cap 4096")
        e.set_trace(cap).reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), cut, f"drops, cap {cap}")


def test_two_phase_windows(engine_mod, ring_ref):
    scn, traces = ring_ref
    want = _reference(traces, 256, TOKEN_NOTE)
    assert want[0]["pairs"] == 424 and want[0]["min_us"] == want[0]["max_us"] == 0
    assert max(len(t) for t in traces) <= 256
    assert any(n == 16 for t in traces for _t, n, _k, _v in t)   # the observer (phase 1) traces
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(256).reset()
        e.run()
        _same(_measure(e, TOKEN_NOTE), want, "ring")


def _check_trace(e, traces, cap, replicas):
    for r in replicas:
        want = sorted(trace_tuples(traces[r]))
        recs, n = e.trace(r)
        got = trace_tuples(recs)
        assert n == len(want), r
        if n <= cap:
            assert got == want, r                      # canonical order: (t, node, tag, val)
        else:
            assert len(got) == cap, r
            assert got == sorted(got), r
            assert not (Counter(got) - Counter(want)), r   # a sub-multiset of the oracle's log


def test_engine_trace(engine_mod, heavy_drop_ref, ring_ref):
    scn, traces = heavy_drop_ref
    emitted = [len(t) for t in traces]
    cap = int(np.median(emitted))
    over = [r for r in range(scn.n_replicas) if emitted[r] > cap]
    under = [r for r in range(scn.n_replicas) if emitted[r] <= cap]
    assert over and under
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(cap).reset()
        e.run()
        _check_trace(e, traces, cap, over[:3] + under[:3])
        # tracing off again: the context runs as before and cannot be measured
        e.set_trace(0).reset()
        st = e.run()
        assert st.events == int(e.results()["events"].sum()) > 0
        assert e.trace(0)[1] == 0
        with pytest.raises(engine_mod.EngineError) as ei:
            _measure(e, ROUND_TRIP)
        assert ei.value.code == ERR_INVALID
    scn, traces = ring_ref
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(256).reset()
        e.run()
        _check_trace(e, traces, 256, [0, 31, 63])


def test_inline_handler(engine_mod, oracle_mod):
    # ForkStrategy `const id`: the Ping handler -- its fused TRACE pair included --
    # runs in the phantom deliverer, not in a thread of its own
    scn = scenarios.hotspot(n_senders=16, n_replicas=16, msg_num=20, fork_strategy="inline")
    traces = _oracle_traces(oracle_mod, scn)
    want = _reference(traces, 2048, ROUND_TRIP)
    assert want[0]["pairs"] == 16 * 16 * 20 and all(len(t) == 4 * 16 * 20 for t in traces)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(2048).reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), want, "inline")
        _check_trace(e, traces, 2048, [0, 15])


def test_two_shards_of_one_gpu(engine_mod, light_ref):
    scn, traces = light_ref
    want = _reference(traces, 2048, ROUND_TRIP)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(2048).reset()
        e.run()
        one = _measure(e, ROUND_TRIP)
    with engine_mod.Engine(devices=[0, 0]) as e:
        e.load(scn, geometry="lpb").set_trace(2048).reset()
        e.run()
        two = _measure(e, ROUND_TRIP)
        assert e.measure_ms() > 0
        _check_trace(e, traces, 2048, [0, 31, 32, 63])   # both shards' replicas
    _same(two, one, "two shards vs one")
    _same(two, want, "two shards vs reference")


def test_rerun_zeroes_the_counter(engine_mod, light_ref):
    scn, traces = light_ref
    want = _reference(traces, 2048, ROUND_TRIP)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(2048).reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), want, "first run")
        e.reset()
        e.run()
        _same(_measure(e, ROUND_TRIP), want, "second run")
        assert e.trace(5)[1] == len(traces[5])


def test_node_partitioned_context_refuses(engine_mod):
    scn = scenarios.gossip(256, seed=1)
    s = engine_mod.lp_scenario(scn)
    with engine_mod.LPEngine(s, 0, scn.n_nodes, int(scn.meta["lookahead_us"])) as e:
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_trace(64)
        assert ei.value.code == ERR_INVALID
