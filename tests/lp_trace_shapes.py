"""Shapes and oracle references shared by test_lp_trace_api.py (CPU) and
test_gpu_lp_trace.py (GPU): the gossip scenario with message ids at 130 nodes
(two workgroups: 128 + 2 lanes; its matching keys fit the LDS join) and 300
nodes (two full 128-lane workgroups plus a 44-lane tail; its keys take the
partition path), with drops.  The reference of every check is the oracle's
trace log sorted by (t, node, tag, val) and measures.measure_reference over it,
computed once per shape and never changed."""
import functools

from timewarp import scenarios
from timewarp.abi import MEASURE_MAX_KEYS
from timewarp.measures import measure_reference
from timewarp.scenarios import TAG_RUMOR_RECV, TAG_RUMOR_SENT

SMALL = dict(n_nodes=130, drop_log2=3, seed=3)   # 455 deliveries, 49 drops, 959 matching keys: LDS join
LARGE = dict(n_nodes=300, drop_log2=3, seed=1)   # 1,045 deliveries, 107 drops, 2,197 matching keys: partition path
# link delays are U[1 ms, 5 ms]: bins over [2 ms, 4 ms) leave both an underflow and an overflow
LATENCY = dict(tag_from=TAG_RUMOR_SENT, tag_to=TAG_RUMOR_RECV, lo_us=2000, bin_us=250, n_bins=8)
ORACLE_CAP = 1 << 16


def scenario(shape, **kw):
    return scenarios.gossip(**dict(shape, **kw))


@functools.lru_cache(maxsize=None)
def _reference(key):
    import oracle

    shape, kw = dict(key[0]), dict(key[1])
    scn = scenario(shape, **kw)
    o = oracle.run(scn, trace_cap=ORACLE_CAP)
    assert len(o.traces) < ORACLE_CAP
    recs = tuple(sorted(o.traces))
    want = measure_reference([list(recs)], [len(recs)], ORACLE_CAP, LATENCY)
    return scn, o, recs, want


def reference(shape, **kw):
    """(scenario, oracle run, canonical records, (total, hist, per) of LATENCY)"""
    return _reference((tuple(sorted(shape.items())), tuple(sorted(kw.items()))))


def matching_keys(recs, spec=LATENCY):
    return sum(1 for _t, _n, tag, _v in recs if tag in (spec["tag_from"], spec["tag_to"]))


def oracle_conditions(shape, large, **kw):
    """What a shape must give on the oracle before any engine runs: pairs and
    open_from (drops) exist, both histogram ends are hit, and the matching keys
    are on the intended side of the LDS join's limit."""
    _scn, o, recs, (tot, hist, _per) = reference(shape, **kw)
    assert tot["pairs"] >= 1 and tot["pairs"] == o.result["delivered"]
    assert tot["open_from"] >= 1 and tot["open_from"] == o.result["dropped"]
    assert tot["repeated"] == 0 and tot["truncated"] == 0
    assert tot["underflow"] >= 1 and tot["overflow"] >= 1 and int(hist.sum()) >= 1
    m = matching_keys(recs)
    assert (m > MEASURE_MAX_KEYS) if large else (m <= MEASURE_MAX_KEYS), m
    return m
