"""Rows the prefix apply leaves unstored against the oracle and
against the same context with the prefix off: every result field and every
node hash bit-exact in every step, with the testing hook on everywhere --
TW_TEST_PREFIX_AUDIT=1 follows every apply that skips rows with a read-only
pass that compares all R elements of every skipped row with the snapshot's
value -- so the invariant itself is tested, not only its consequences.

A sweep that retires every replica's kill wakes compares, per replica, the tid
and queued seq of every parked killer and victim with the snapshot's; the next
apply skips quads 1 - 3 of the threads that matched everywhere.  The rings
drop one message in four (drop_log2=2): tokens die at different hops, so a
worker's slot is dirty in some replicas only.  With 40 nodes and 20 s a few
nodes are visited and most are not; with 4 nodes every worker is.  301
replicas are more than one dense or half workgroup, 70 more than one narrow one.
"""
import functools

import numpy as np
import pytest

from timewarp import scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.timeunits import sec

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "forkfirst": 5}
T_KILL = sec(20)
GEOS = [("dense", 301), ("narrow", 70), ("half", 301)]
ORDERS = ["fifo", "forkfirst"]

_ORACLE = {}


@pytest.fixture(autouse=True)
def _audit_hook(monkeypatch):
    monkeypatch.setenv("TW_TEST_PREFIX_AUDIT", "1")  # (read when a context is made)


@functools.lru_cache(maxsize=None)
def _ring(n_nodes, n_replicas, link_depth=1):
    return scenarios.token_ring(n_nodes=n_nodes, n_replicas=n_replicas, launch_duration=T_KILL, drop_log2=2,
                                link_depth=link_depth)


def _oracle(oracle_mod, scn, order):
    key = (id(scn), order)  # (the builders are cached: one object per scenario)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


def _claimed_ok(cs, N):
    """One kill wake per ring node and the observer's, two victims each, all
    parked from the snapshot on: 3 (N + 1) slots.  Main has ended by then and
    its slot 0 was handed to a later fork; slot 0 is never claimed (tw_reset
    writes it), so the one position that names it, if any, is not claimable."""
    assert cs["claimed_slots"] in (3 * N, 3 * (N + 1)), cs


def _same(tag, res, h, ores, oh):
    for f in FIELDS:
        assert np.array_equal(res[f], ores[f]), (tag, f, res[f][:6], ores[f][:6])
    assert np.array_equal(h, oh), tag


def _engine(engine_mod, scn, order, geo, prefix=True):
    e = engine_mod.Engine(0)
    e.load(scn, geometry=geo)
    e.set_tie_mode(order)
    if not prefix:
        e.set_prefix(False)
    return e


def _step(e, runs=({},)):
    """reset, the tw_run calls `runs`: results, hashes, tw_prefix_stats, tw_prefix_clean_stats
    (the apply is the first call's: its counts are read behind that call)"""
    e.reset()
    cs = None
    for kw in runs:
        e.run(**kw)
        if cs is None:
            cs = e.prefix_clean_stats()
            ps = e.prefix_stats()
    cs["verified"] = e.prefix_clean_stats()["verified"]  # (of the last call)
    return e.results(), e.hashes(), ps, cs


def _stores_all(ps, cs, want="applied"):
    assert ps["last"] == want, ps
    assert cs["rows_skipped"] == 0 and cs["bytes_stored"] == ps["bytes"] and cs["audit_mismatches"] == 0, cs


def _skips(ps, cs):
    assert ps["last"] == "applied", ps
    assert 0 < cs["rows_skipped"] <= 3 * cs["claimed_slots"], cs
    assert cs["bytes_stored"] + 16 * cs["rows_skipped"] == ps["bytes"], (ps, cs)
    assert cs["audit_mismatches"] == 0, cs


def _off(engine_mod, scn, order, geo, **kw):
    """the same context with the prefix off"""
    with _engine(engine_mod, scn, order, geo, prefix=False) as e0:
        e0.reset()
        e0.run(**kw)
        assert e0.prefix_stats()["last"] == "not_eligible" and e0.prefix_clean_stats()["claimed_slots"] == 0
        return e0.results(), e0.hashes()


# --------------------------------------------------------- pilot, then skipping applies
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_unvisited_nodes_are_skipped(engine_mod, oracle_mod, order, geo, R):
    N = 40
    scn = _ring(N, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    res0, h0 = _off(engine_mod, scn, order, geo)
    _same((order, geo, "off"), res0, h0, ores, oh)
    with _engine(engine_mod, scn, order, geo) as e:
        for i in range(4):
            res, h, ps, cs = _step(e)
            _same((order, geo, i), res, h, ores, oh)
            _same((order, geo, i, "off"), res, h, res0, h0)
            _claimed_ok(cs, N)
            assert cs["verified"], cs
            if i == 0:
                _stores_all(ps, cs, "piloted")
            else:
                _skips(ps, cs)
                # some node was visited in some replica: its three threads are stored
                assert cs["rows_skipped"] < 3 * cs["claimed_slots"], cs
                # ... and most were not
                assert cs["rows_skipped"] > 3 * cs["claimed_slots"] // 2, cs


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_every_worker_visited(engine_mod, oracle_mod, order, geo, R):
    """4 nodes: the token passes every worker in some replica, and a position
    whose victim changed marks its killer too: at most the kill wakes' rows
    (three per position) are skipped"""
    N = 4
    scn = _ring(N, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        for i in range(3):
            res, h, ps, cs = _step(e)
            _same((order, geo, i), res, h, ores, oh)
            _claimed_ok(cs, N)
            assert cs["verified"], cs
            assert cs["rows_skipped"] <= 3 * (N + 1) and cs["audit_mismatches"] == 0, cs
            assert cs["bytes_stored"] + 16 * cs["rows_skipped"] == ps["bytes"], (ps, cs)
            if i == 0:
                _stores_all(ps, cs, "piloted")


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_link_depth(engine_mod, oracle_mod, order, geo, R):
    scn = _ring(40, R, link_depth=3)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        for i in range(3):
            res, h, ps, cs = _step(e)
            _same((order, geo, i), res, h, ores, oh)
            if i == 0:
                _stores_all(ps, cs, "piloted")
            else:
                _skips(ps, cs)


# ------------------------------------------------- the next apply stores everything
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_runs_that_do_not_verify(engine_mod, oracle_mod, order, geo, R):
    scn = _ring(40, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        res, h, ps, cs = _step(e)
        _stores_all(ps, cs, "piloted")
        res, h, ps, cs = _step(e)
        _skips(ps, cs)
        # the sweep off: nothing is checked (and the setter ends the last run's verification)
        e.set_sweep(False)
        res, h, ps, cs = _step(e)
        _stores_all(ps, cs)
        assert not cs["verified"]
        _same((order, geo, "sweep off"), res, h, ores, oh)
        e.set_sweep(True)
        res, h, ps, cs = _step(e)
        _stores_all(ps, cs)
        assert cs["verified"]
        _same((order, geo, "sweep on"), res, h, ores, oh)
        res, h, ps, cs = _step(e)
        _skips(ps, cs)
        # in pieces, stopping before T; then reset
        res, h, ps, cs = _step(e, ({"t_end": sec(5)}, {"t_end": T_KILL - 1}))
        _skips(ps, cs)
        assert not cs["verified"]
        res, h, ps, cs = _step(e)
        _stores_all(ps, cs)
        assert cs["verified"]
        _same((order, geo, "after pieces"), res, h, ores, oh)
        # in pieces across T: the piece that holds the sweep verifies
        pieces = ({"t_end": sec(5)}, {"t_end": T_KILL - 1}, {"t_end": T_KILL}, {})
        res, h, ps, cs = _step(e, pieces)
        _skips(ps, cs)
        _same((order, geo, "pieces"), res, h, ores, oh)
        # (the last piece found nothing to do: a run after the verifying one ends the verification)
        assert not cs["verified"]
        res, h, ps, cs = _step(e)
        _stores_all(ps, cs)
        res, h, ps, cs = _step(e, ({"t_end": sec(5)}, {"t_end": T_KILL}))
        _skips(ps, cs)
        assert cs["verified"]
        _same((order, geo, "pieces to T"), res, h, ores, oh)
        res, h, ps, cs = _step(e)
        _skips(ps, cs)
        _same((order, geo, "after pieces to T"), res, h, ores, oh)


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_sweep_refused_at_the_event_cap(engine_mod, oracle_mod, order, geo, R):
    """max_events inside the sweep: every replica is refused and pops its kill
    wakes one by one up to the cap; nothing was checked"""
    scn = _ring(40, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    cap = int(ores["events"].min()) - 1
    res0, h0 = _off(engine_mod, scn, order, geo, max_events=cap)
    with _engine(engine_mod, scn, order, geo) as e:
        _step(e)
        res, h, ps, cs = _step(e)
        _skips(ps, cs)
        res, h, ps, cs = _step(e, ({"max_events": cap},))
        _skips(ps, cs)
        assert not cs["verified"] and e.sweep_stats()["killers"] == 0
        _same((order, geo, "cap"), res, h, res0, h0)
        res, h, ps, cs = _step(e)
        _stores_all(ps, cs)
        _same((order, geo, "after cap"), res, h, ores, oh)
        res, h, ps, cs = _step(e)
        _skips(ps, cs)
        _same((order, geo, "again"), res, h, ores, oh)


@pytest.mark.parametrize("geo,R", GEOS)
def test_setters_and_state_writing_calls(engine_mod, oracle_mod, geo, R):
    scn = _ring(40, R)
    with _engine(engine_mod, scn, "fifo", geo) as e, _engine(engine_mod, scn, "fifo", geo, prefix=False) as e0:
        order = "fifo"
        ores, oh = _oracle(oracle_mod, scn, order)

        def verified_step():
            res, h, ps, cs = _step(e)
            assert cs["verified"]
            return res, h, ps, cs

        _stores_all(*verified_step()[2:], "piloted")
        _skips(*verified_step()[2:])
        # a tie-mode change and a counter base re-pilot
        for order in ("forkfirst", "fifo"):
            e.set_tie_mode(order)
            res, h, ps, cs = verified_step()
            _stores_all(ps, cs, "piloted")
            _same((geo, order, "piloted"), res, h, *_oracle(oracle_mod, scn, order))
            res, h, ps, cs = verified_step()
            _skips(ps, cs)
            _same((geo, order, "applied"), res, h, *_oracle(oracle_mod, scn, order))
        e.set_counter_base(1000, 77)
        e0.set_counter_base(1000, 77)
        e0.reset()
        e0.run()
        res0, h0 = e0.results(), e0.hashes()
        for i in range(2):
            res, h, ps, cs = verified_step()
            _stores_all(ps, cs, "piloted") if i == 0 else _skips(ps, cs)
            _same((geo, "base", i), res, h, res0, h0)
        e.set_counter_base(0, 1)
        _stores_all(*verified_step()[2:], "piloted")
        _skips(*verified_step()[2:])
        # calls between the verifying run and the next apply
        for name, call in (("set_prefix", lambda: e.set_prefix(True)), ("set_trace", lambda: e.set_trace(0)),
                           ("tie_audit", lambda: e.tie_audit(probes=1))):
            call()
            res, h, ps, cs = verified_step()
            _stores_all(ps, cs)
            _same((geo, name), res, h, ores, oh)
            res, h, ps, cs = verified_step()
            _skips(ps, cs)
            _same((geo, name, "again"), res, h, ores, oh)
        # read-only calls between them leave the verification alone
        e.results(); e.hashes(); e.prefix_stats(); e.sweep_stats(); e.launch_ms()
        _skips(*verified_step()[2:])
