"""The surface of TRACE records for node-partitioned contexts, CPU only: the
header and the Python binding name the three calls, gossip() without message
ids is the image it was, gossip(message_ids=True) is tie-insensitive on the
oracle, and the test shapes give what test_gpu_lp_trace.py relies on."""
import os
import re

import numpy as np
import pytest

import lp_trace_shapes as shapes
from timewarp import scenarios
from timewarp.measures import first_receipts
from timewarp.scenarios import TAG_RUMOR_FIRST, TAG_RUMOR_RECV, TAG_RUMOR_SENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("tw_lp_set_trace", "tw_lp_read_trace", "tw_lp_measure")


def test_header_and_exports_name_the_calls():
    from timewarp import engine, isa

    with open(os.path.join(ROOT, "include", "timewarp.h")) as f:
        text = f.read()
    for name in CALLS:
        assert re.search(r"^int %s\(tw_ctx\* ctx, " % name, text, re.M), name
        assert name in engine.EXPORTS
    assert len(set(engine.EXPORTS)) == len(engine.EXPORTS)
    assert re.search(r"^#define TW_ABI_VERSION 4u$", text, re.M) and isa.ABI_VERSION == 4
    for name in ("lp_set_trace", "lp_trace", "lp_measure"):
        assert callable(getattr(engine.LPEngine, name))


def _same_scenario(a, b):
    assert a.name == b.name and a.main_pc == b.main_pc and a.main_node == b.main_node
    assert a.image.insns.tobytes() == b.image.insns.tobytes()
    assert a.image.consts.tobytes() == b.image.consts.tobytes()
    assert a.image.listener_pc.tobytes() == b.image.listener_pc.tobytes()
    assert a.link_table.tobytes() == b.link_table.tobytes()
    assert a.topo.dst.tobytes() == b.topo.dst.tobytes() and a.topo.out_off.tobytes() == b.topo.out_off.tobytes()
    assert a.meta == b.meta


@pytest.mark.parametrize("fork_strategy", ["fork", "inline"])
def test_default_gossip_image_unchanged(fork_strategy):
    kw = dict(n_nodes=300, drop_log2=3, seed=1, fork_strategy=fork_strategy)
    _same_scenario(scenarios.gossip(**kw), scenarios.gossip(message_ids=False, **kw))
    ids = scenarios.gossip(message_ids=True, **kw)
    assert ids.image.insns.tobytes() != scenarios.gossip(**kw).image.insns.tobytes()
    assert ids.link_table.tobytes() == scenarios.gossip(**kw).link_table.tobytes()
    if fork_strategy == "fork":
        _same_scenario(scenarios.gossip(), scenarios.gossip(message_ids=False))


@pytest.mark.parametrize("shape", [shapes.SMALL, shapes.LARGE], ids=["130", "300"])
@pytest.mark.parametrize("fork_strategy", ["fork", "inline"])
def test_message_ids_tie_insensitive_on_the_oracle(oracle_mod, shape, fork_strategy):
    """TimedT's own pqueue order and the canonical (t, seq) order give the same
    results, node hashes and sorted traces: which of several equal-time copies
    of the rumor arrives first reaches no output."""
    scn = shapes.scenario(shape, message_ids=True, fork_strategy=fork_strategy)
    a = oracle_mod.run(scn, mode=oracle_mod.MODE_CANONICAL)
    for mode in (oracle_mod.MODE_PQUEUE, oracle_mod.MODE_LIFO, oracle_mod.MODE_SCRAMBLE):
        b = oracle_mod.run(scn, mode=mode)
        assert a.result == b.result, mode
        assert np.array_equal(a.hashes, b.hashes), mode
        assert sorted(a.traces) == sorted(b.traces), mode
    # TRACEs add no pops and the payload does not steer forwarding: the base scenario's counters
    base = oracle_mod.run(shapes.scenario(shape, fork_strategy=fork_strategy))
    for f in ("final_t", "events", "delivered", "dropped", "undeliverable", "threads"):
        assert a.result[f] == base.result[f], f
    first = [r for r in a.traces if r[2] == TAG_RUMOR_FIRST]
    assert sorted((t, n) for t, n, _k, _v in first) == sorted((t, n) for t, n, _k, _v in base.traces)
    assert {v for _t, _n, _k, v in first} == {1}  # a constant, not the payload


def test_shapes_on_the_oracle(oracle_mod):
    m_small = shapes.oracle_conditions(shapes.SMALL, large=False, message_ids=True)
    m_large = shapes.oracle_conditions(shapes.LARGE, large=True, message_ids=True)
    assert (m_small, m_large) == (959, 2197)
    _scn, o, recs, (tot, _h, _p) = shapes.reference(shapes.SMALL, message_ids=True)
    # ids are link ids: one SENT per id, a RECV for every delivered one
    sent = [v for _t, _n, k, v in recs if k == TAG_RUMOR_SENT]
    recv = [v for _t, _n, k, v in recs if k == TAG_RUMOR_RECV]
    assert len(set(sent)) == len(sent) and set(recv) <= set(sent) and len(recv) == o.result["delivered"]
    assert tot["min_us"] >= 1000 and tot["max_us"] <= 5000  # the link delays' range


def test_first_receipts_gives_the_propagation_curve(oracle_mod):
    scn, _o, recs, _want = shapes.reference(shapes.SMALL, message_ids=True)
    times, hist = first_receipts(recs, TAG_RUMOR_FIRST, lo_us=1_000_000, bin_us=2000, n_bins=8)
    first = sorted(t for t, _n, k, _v in recs if k == TAG_RUMOR_FIRST)
    assert times.dtype == np.int64 and times.tolist() == first and len(first) == 125
    want = np.zeros(8, np.uint64)
    for t in first:
        if 0 <= (t - 1_000_000) // 2000 < 8:
            want[(t - 1_000_000) // 2000] += 1
    assert hist.dtype == np.uint64 and np.array_equal(hist, want) and 0 < int(hist.sum()) <= len(first)
    # a node counts once, at its earliest record; records as a structured array work too
    from timewarp.engine import TRACE_DTYPE

    arr = np.array([(5, 0, 2, 9), (3, 0, 2, 9), (4, 0, 1, 9), (7, 0, 2, 8)],
                   dtype=[("t", np.int64), ("val", np.int64), ("node", np.uint32), ("tag", np.uint32)])
    assert arr.dtype == TRACE_DTYPE
    t2, h2 = first_receipts(arr, 9, lo_us=0, bin_us=4, n_bins=2)
    assert t2.tolist() == [3, 4] and h2.tolist() == [1, 1]
    with pytest.raises(ValueError):
        first_receipts(recs, TAG_RUMOR_FIRST, n_bins=0)
