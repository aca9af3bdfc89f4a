"""TRACE records of tw_lp_batch (Engine.set_trace_batch, tw_set_trace_batch):
a traced batched-LP context that keeps the data-parallel batch of its heavy
receiver's due records running, in the kernel variant that records them.

Every expectation is timewarp.measures.measure_reference, or the sorted log
itself, fed with the oracle's trace log -- never the engine's chain output --
and the oracle's trace lengths are asserted, so no replica is silently over a
cap.  Everything is integer: the comparisons are exact.  TAG_PING and
TAG_PONG_SENT are traced by the receiver's Ping handler, which is what the
batch runs: ONE_WAY and SERVICE read its records, ROUND_TRIP none of them.

Shapes: the receiver of 64 senders (tens of due records per window: tw_lp_due
sorts them and tw_lp_batch<true> runs them, one per thread), the same with
drops at a cap some replicas exceed (a claim that straddles the cap), handlers
with 7 traces (fused pairs) and with 72 (over the 63 a record's count may
reach: those stay on the chain), 256 senders (more due records per window than
the workgroup has threads: chunks of two), a stateful and an inline handler
(never batched), the setting toggled on one context, and two shards."""
from collections import Counter

import numpy as np
import pytest

from timewarp import scenarios
from timewarp.abi import MEASURE_DTYPE, RESULT_FIELDS
from timewarp.measures import measure_reference, trace_tuples
from timewarp.scenarios import TAG_PING, TAG_PING_SENT, TAG_PONG, TAG_PONG_SENT

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

ERR_INVALID, ERR_STATE = -1, -5
ONE_WAY = dict(tag_from=TAG_PING_SENT, tag_to=TAG_PING, lo_us=1000, bin_us=125, n_bins=40)
SERVICE = dict(tag_from=TAG_PING, tag_to=TAG_PONG_SENT, lo_us=0, bin_us=1, n_bins=4)
ROUND_TRIP = dict(tag_from=TAG_PING_SENT, tag_to=TAG_PONG, lo_us=2000, bin_us=250, n_bins=40)
SPECS = (("one way", ONE_WAY), ("service", SERVICE), ("round trip", ROUND_TRIP))


def _oracle_traces(oracle_mod, scn, cap=1 << 14):
    out = []
    for r in range(scn.n_replicas):
        out.append(oracle_mod.run(scn, replica=r, trace_cap=cap).traces)
        assert len(out[-1]) < cap
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


def _same_measures(e, traces, cap, tag):
    for name, spec in SPECS:
        _same(_measure(e, spec), _reference(traces, cap, spec), f"{tag}, {name}")


def _check_trace(e, traces, cap, replicas):
    for r in replicas:
        want = sorted(trace_tuples(traces[r]))
        recs, n = e.trace(r, cap=max(cap, 1))
        got = trace_tuples(recs)
        assert n == len(want), r                       # the emitted count is exact either way
        if n <= cap:
            assert got == want, r                      # canonical order: (t, node, tag, val)
        else:
            assert len(got) == cap, r
            assert got == sorted(got), r
            assert not (Counter(got) - Counter(want)), r   # a sub-multiset of the oracle's log


def _untraced(engine_mod, scn):
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").reset()
        e.run()
        return e.results(), e.hashes(), e.lpb_batch()


def _same_results(e, res_u, h_u):
    res, h = e.results(), e.hashes()
    for f in RESULT_FIELDS:
        assert np.array_equal(res[f], res_u[f]), f
    assert np.array_equal(h, h_u)


@pytest.fixture(scope="module")
def heavy_ref(oracle_mod, engine_mod):
    scn = scenarios.hotspot(n_senders=64, n_replicas=32, msg_num=12)
    traces = _oracle_traces(oracle_mod, scn)
    assert all(len(t) == 3072 for t in traces)
    return scn, traces, _untraced(engine_mod, scn)


@pytest.fixture(scope="module")
def heavy_drop_ref(oracle_mod):
    scn = scenarios.hotspot(n_senders=64, n_replicas=32, msg_num=12, drop_log2=2)
    traces = _oracle_traces(oracle_mod, scn)
    assert max(len(t) for t in traces) < 4096
    return scn, traces


def test_heavy_receiver_batched_and_traced(engine_mod, heavy_ref):
    scn, traces, (res_u, h_u, (batched_u, due_u)) = heavy_ref
    print("untraced: batched", batched_u, "due", due_u)
    assert batched_u > 0
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(4096).set_trace_batch(True).reset()
        e.run()
        batched, due = e.lpb_batch()
        print("traced, batch on: batched", batched, "due", due)
        assert batched > 0                     # (0 without tw_lp_batch<true>)
        assert due == due_u
        assert batched == batched_u            # every record traces twice: none is over the count
        _check_trace(e, traces, 4096, range(scn.n_replicas))
        _same_measures(e, traces, 4096, "heavy")
        _same_results(e, res_u, h_u)


def test_drops_and_truncation(engine_mod, heavy_drop_ref):
    scn, traces = heavy_drop_ref
    emitted = [len(t) for t in traces]
    cap = int(np.median(emitted))
    cut = _reference(traces, cap, ROUND_TRIP)
    print("median emitted", cap, "truncated replicas", cut[0]["truncated"])
    assert 1 <= cut[0]["truncated"] < scn.n_replicas      # some replicas truncated, some not
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(4096).set_trace_batch(True).reset()
        e.run()
        assert e.lpb_batch()[0] > 0
        _same_measures(e, traces, 4096, "drops, cap 4096")
        _check_trace(e, traces, 4096, range(scn.n_replicas))
        e.set_trace(cap).reset()
        e.run()
        assert e.lpb_batch()[0] > 0
        _same_measures(e, traces, cap, f"drops, cap {cap}")
        _check_trace(e, traces, cap, range(scn.n_replicas))


@pytest.mark.parametrize("probes,cap", [(5, 4096), (70, 32768)])
def test_many_traces_per_record(engine_mod, oracle_mod, probes, cap):
    # the Ping handler traces probes + 2 times (the assembler fuses pairs): 7
    # fit a record's count, 72 do not -- those records stay on the chain
    scn = scenarios.hotspot(n_senders=64, n_replicas=16, msg_num=4, probe_traces=probes)
    traces = _oracle_traces(oracle_mod, scn, cap=cap)
    assert all(len(t) == 64 * 4 * (probes + 4) for t in traces)
    service = _reference(traces, cap, SERVICE)
    assert service[0]["repeated"] == 64 * 4 * 16 and service[0]["pairs"] == 0   # TAG_PING repeats per id
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_measure_keys(cap).set_trace(cap).set_trace_batch(True).reset()
        e.run()
        batched, due = e.lpb_batch()
        print("probes", probes, "batched", batched, "due", due)
        assert due > 0
        if probes == 5:
            assert batched > 0
        _check_trace(e, traces, cap, range(scn.n_replicas))
        _same(_measure(e, SERVICE), service, f"{probes} probes, service")
        _same(_measure(e, ROUND_TRIP), _reference(traces, cap, ROUND_TRIP), f"{probes} probes, round trip")


def test_prefix_longer_than_the_workgroup(engine_mod, oracle_mod):
    # 256 senders at one ping per ms, delays of 1-5 ms: the receiver's windows
    # hold up to ~190 due records, more than tw_lp_batch's 128 threads, so a
    # thread's chunk of the prefix is two records (three traces each)
    scn = scenarios.hotspot(n_senders=256, n_replicas=4, msg_num=4, probe_traces=1)
    traces = _oracle_traces(oracle_mod, scn)
    assert all(len(t) == 256 * 4 * 5 for t in traces)
    res_u, h_u, (batched_u, due_u) = _untraced(engine_mod, scn)
    assert batched_u > 0
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_measure_keys(8192).set_trace(8192).set_trace_batch(True).reset()
        e.run()
        assert e.lpb_batch() == (batched_u, due_u)
        _check_trace(e, traces, 8192, range(scn.n_replicas))
        _same_measures(e, traces, 8192, "256 senders")
        _same_results(e, res_u, h_u)


@pytest.mark.parametrize("kw", [dict(receiver_counter=True), dict(fork_strategy="inline")],
                         ids=["stateful", "inline"])
def test_handlers_the_batch_refuses(engine_mod, oracle_mod, kw):
    scn = scenarios.hotspot(n_senders=64, n_replicas=8, msg_num=6, **kw)
    traces = _oracle_traces(oracle_mod, scn)
    assert all(len(t) == 4 * 64 * 6 for t in traces)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(2048).set_trace_batch(True).reset()
        e.run()
        batched, due = e.lpb_batch()
        assert due > 0 and batched == 0
        _check_trace(e, traces, 2048, range(scn.n_replicas))
        _same_measures(e, traces, 2048, str(kw))


def test_default_and_toggle(engine_mod, heavy_ref):
    scn, traces, (res_u, h_u, (batched_u, _due_u)) = heavy_ref
    some = [0, 13, 31]
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(4096).reset()
        e.run()
        assert e.lpb_batch()[0] == 0               # off after a load
        _check_trace(e, traces, 4096, some)
        e.set_trace_batch(True).reset()
        e.run()
        assert e.lpb_batch()[0] == batched_u
        _check_trace(e, traces, 4096, some)
        first = [_measure(e, spec) for _n, spec in SPECS]
        e.reset()                                  # the same context again: the counters start at 0
        e.run()
        assert e.lpb_batch()[0] == batched_u
        for (name, spec), one in zip(SPECS, first):
            _same(_measure(e, spec), one, f"re-run, {name}")
            _same(one, _reference(traces, 4096, spec), f"on, {name}")
        _same_results(e, res_u, h_u)
        e.set_trace_batch(False).reset()
        e.run()
        assert e.lpb_batch()[0] == 0
        _check_trace(e, traces, 4096, some)
        _same_measures(e, traces, 4096, "off again")
        # tracing off: the setting changes nothing, the plain batch runs
        e.set_trace_batch(True).set_trace(0).reset()
        e.run()
        assert e.lpb_batch()[0] == batched_u
        assert e.trace(0)[1] == 0
        _same_results(e, res_u, h_u)
        # a load turns it off again
        e.load(scn, geometry="lpb").set_trace(4096).reset()
        e.run()
        assert e.lpb_batch()[0] == 0


def test_two_shards_of_one_gpu(engine_mod, heavy_ref):
    scn, traces, (res_u, h_u, _bat) = heavy_ref
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(4096).set_trace_batch(True).reset()
        e.run()
        one = [_measure(e, spec) for _n, spec in SPECS]
    with engine_mod.Engine(devices=[0, 0]) as e:
        e.load(scn, geometry="lpb").reset()
        e.run()
        batched_2u = e.lpb_batch()[0]               # both shards' batches, untraced
        assert batched_2u > 0
        e.set_trace(4096).set_trace_batch(True).reset()
        e.run()
        assert e.lpb_batch()[0] == batched_2u       # the setting reached both shards
        two = [_measure(e, spec) for _n, spec in SPECS]
        _check_trace(e, traces, 4096, [0, 15, 16, 31])   # both shards' replicas
        _same_results(e, res_u, h_u)
    for (name, spec), a, b in zip(SPECS, one, two):
        _same(b, a, f"two shards vs one, {name}")
        _same(b, _reference(traces, 4096, spec), f"two shards vs reference, {name}")


def test_status_codes(engine_mod):
    with engine_mod.Engine() as e:
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_trace_batch(True)
        assert ei.value.code == ERR_STATE              # nothing loaded
        e.load(scenarios.ping_pong(n_replicas=64), geometry="dense")
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_trace_batch(True)
        assert ei.value.code == ERR_INVALID            # a replica context
    scn = scenarios.gossip(256, seed=1)
    s = engine_mod.lp_scenario(scn)
    with engine_mod.LPEngine(s, 0, scn.n_nodes, int(scn.meta["lookahead_us"])) as e:
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_trace_batch(True)
        assert ei.value.code == ERR_INVALID            # tw_lp_load
