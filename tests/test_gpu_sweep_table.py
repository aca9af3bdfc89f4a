"""The sweep's terminal path against the oracle, against the same
context with the path forced off (TW_TEST_SWEEP_SLOW=1) and against the same
context with the prefix off: every result field and every node hash bit-exact
in every step, with TW_TEST_PREFIX_AUDIT=1 everywhere.

A replica that the sweep ends -- every thread it has left is a kill wake of the
sweep or a victim of one, every ref is one the kill table recorded, the table
names no victim twice -- gets its hash terms, listener releases and counts and
nothing else: no dead header, no claim swap, no free-stack append.  An entry
whose words validate found equal to the table's takes them from the effects
row without loading a header ("fast"); any other loads them ("slow").
tw_sweep_path_stats says which path ran.

The rings drop one message in four: tokens die at different hops, so a
position is clean in some replicas of a wave and not in others.  The hand-made
programs (`units`) have a send at 2 s, so they take the prefix and get a
table; what the message's handler does differs by case, and the message is
dropped in half the replicas: terminal and surviving replicas share waves.
"""
import functools

import numpy as np
import pytest

from timewarp import isa, scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.scenarios import draw_table
from timewarp.timeunits import at, for_, ms, sec

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "forkfirst": 5}
T_KILL = sec(20)   # beyond the 10 s on-chip horizon: the kill wakes queue in the far runs
T_LATE = sec(40)
GEOS = [("dense", 301), ("narrow", 70), ("half", 301)]
ORDERS = ["fifo", "forkfirst"]

_ORACLE = {}


@pytest.fixture(autouse=True)
def _audit_hook(monkeypatch):
    monkeypatch.setenv("TW_TEST_PREFIX_AUDIT", "1")  # (read when a context is made)


@functools.lru_cache(maxsize=None)
def _ring(n_nodes, n_replicas):
    return scenarios.token_ring(n_nodes=n_nodes, n_replicas=n_replicas, launch_duration=T_KILL, drop_log2=2)


@functools.lru_cache(maxsize=None)
def units(case, K=40, n_replicas=70, drop_log2=1):
    """main (node K) forks K units, one per node, waits 2 s, sends one ping to
    node 0 and ends.  A unit forks a sleeper and a server (which owns the
    node's listener) and schedules `throwTo r1; throwTo r2; END` at T_KILL.
    The ping is dropped in one replica of 2^drop_log2; its handler, by case:

    plain: ends
    dup: ends; every unit schedules its kill pair twice (each victim named by
        two kill wakes: the table is not exclusive)
    survivor: forks a thread that sleeps to T_LATE, then forks 2 K leaves that
        live for a while -- more than there were free slots before the sweep --
        and sends a ping to node 1, whose server the sweep killed
    late_wake: forks one more sleeper and schedules a kill wake for it at
        T_KILL: a kill wake the snapshot does not have
    stale_dup: ends; unit 1 forks, in the server's place, a child that ends at
        once (r2 is stale in the snapshot: its positions are not claimable)
        and schedules its kill pair twice, so two positions whose refs are
        only recorded name one sleeper; main also forks a thread that sleeps
        to T_LATE, in every replica
    """
    p = Program()
    KP = p.kind("ping")
    lset = p.listener_set({"ping": "on_ping"})
    c = p.function("main")
    c.seti(0, 0).seti(2, K)
    loop = c.here()
    c.fork("unit", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 2, loop)
    if case == "stale_dup":
        c.fork_("sleep_late")
    c.wait(for_(sec(2)))
    c.seti(0, 7).link(1, 0).send(1, KP, 0)
    c.end()
    c = p.function("sleep_late")
    c.wait(at(T_LATE)).end()
    c = p.function("quick")
    c.end()

    c = p.function("unit")
    c.fork("sleeper", ref=1)
    if case == "stale_dup":
        even = c.label()
        c.jnei(0, 1, even)
        c.fork("quick", ref=2)
        c.schedule(at(T_KILL), "kill_pair")
        c.schedule(at(T_KILL), "kill_pair")
        c.end()
        c.bind(even)
    c.fork("server", ref=2)
    for _ in range(2 if case == "dup" else 1):
        c.schedule(at(T_KILL), "kill_pair")
    c.end()
    c = p.function("kill_pair")
    c.kill_thread(1).kill_thread(2).end()
    c = p.function("kill_one")
    c.kill_thread(1).end()
    c = p.function("sleeper")
    c.sleep_forever()
    c = p.function("server")
    c.listen(lset, owned=True)
    c.sleep_forever()

    c = p.function("on_ping")
    if case == "survivor":
        c.fork_("late")
    elif case == "late_wake":
        c.fork("sleeper", ref=1)
        c.schedule(at(T_KILL), "kill_one")
    c.end()
    c = p.function("late")
    c.wait(at(T_LATE))
    c.seti(0, 0).seti(2, 2 * K)
    loop = c.here()
    c.fork_("leaf")
    c.addi(0, 1).jlt(0, 2, loop)
    c.seti(0, 9).link(1, 0).send(1, KP, 0)
    c.end()
    c = p.function("leaf")
    c.wait(for_(sec(1))).end()

    img = p.finalize()
    out = [[1]] + [[] for _ in range(K - 1)] + [[0]]   # node 0 -> node 1; main's node -> node 0
    topo = Topology.from_out_lists(K + 1, out)
    L = topo.n_links
    links = np.arange(L)
    lo, hi = np.full(L, ms(1), np.int64), np.full(L, ms(5), np.int64)
    table = draw_table(L, n_replicas, links, lo, hi, link_depth=1, drop_log2=drop_log2, seed_base=0)
    return Scenario(name=f"units_{case}_{K}_{drop_log2}", image=img, topo=topo, n_replicas=n_replicas,
                    main_pc=img.pc_of("main"), main_node=K, link_table=table, max_slots=4 * K + 16,
                    queue_capacity=8 * K + 64, run_capacity=256, max_frames=2)


def _oracle(oracle_mod, scn, order):
    key = (id(scn), order)  # (the builders are cached: one object per scenario)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


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


def _slow_engine(engine_mod, monkeypatch, scn, order, geo):
    """the same context with every replica on tw_sweep_apply's general path"""
    monkeypatch.setenv("TW_TEST_SWEEP_SLOW", "1")
    e = _engine(engine_mod, scn, order, geo)
    monkeypatch.delenv("TW_TEST_SWEEP_SLOW")
    return e


def _step(e, runs=({},)):
    """reset and the tw_run calls `runs`: results, hashes, the sweep's counts
    and paths summed over the calls, tw_prefix_clean_stats of the first call's apply"""
    e.reset()
    sw = {"killers": 0, "victims": 0, "refused_replicas": 0, "terminal_replicas": 0, "fast_entries": 0,
          "slow_entries": 0}
    cs = None
    for kw in runs:
        e.run(**kw)
        for k, v in dict(e.sweep_stats(), **e.sweep_path_stats()).items():
            sw[k] += v
        if cs is None:
            cs = e.prefix_clean_stats()
    return e.results(), e.hashes(), sw, cs


def _off(engine_mod, scn, order, geo, **kw):
    with _engine(engine_mod, scn, order, geo, prefix=False) as e0:
        e0.reset()
        e0.run(**kw)
        assert e0.sweep_path_stats() == {"terminal_replicas": 0, "fast_entries": 0,
                                         "slow_entries": e0.sweep_stats()["killers"]}
        return e0.results(), e0.hashes()


def _slow_counts(sw):
    assert sw["terminal_replicas"] == 0 and sw["fast_entries"] == 0 and sw["slow_entries"] == sw["killers"], sw


# --------------------------------------------------------------- the token ring
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", [40, 4])
def test_ring_ends_on_the_terminal_path(engine_mod, oracle_mod, monkeypatch, N, order, geo, R):
    """Four reset / run pairs.  Every replica ends at the sweep; the observer's
    kill wake names slot 0 and is no table position, but its refs are the
    recorded ones, so every replica is table-bound.  An entry is slow where the
    token changed its worker (and at the observer's); with 40 nodes most
    entries are fast.  (With 4 nodes a replica whose token is dropped at its
    first send still leaves three workers untouched, so some entries are fast
    there too; the slow ones are counted exactly from the oracle's deliveries.)"""
    scn = _ring(N, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    res0, h0 = _off(engine_mod, scn, order, geo)
    _same((N, order, geo, "off"), res0, h0, ores, oh)
    with _engine(engine_mod, scn, order, geo) as e, _slow_engine(engine_mod, monkeypatch, scn, order, geo) as es:
        for i in range(4):
            res, h, sw, cs = _step(e)
            ress, hs, sws, css = _step(es)
            print((N, order, geo, i), sw, cs)
            _same((N, order, geo, i), res, h, ores, oh)
            _same((N, order, geo, i, "slow"), ress, hs, ores, oh)
            assert (res["status"] == isa.REP_DONE).all()
            _slow_counts(sws)
            assert sw["killers"] == (N + 1) * R and sw["victims"] == 2 * (N + 1) * R and sw["refused_replicas"] == 0
            assert {k: sws[k] for k in ("killers", "victims", "refused_replicas")} == \
                   {k: sw[k] for k in ("killers", "victims", "refused_replicas")}
            assert sw["fast_entries"] + sw["slow_entries"] == sw["killers"], sw
            assert cs["audit_mismatches"] == 0 and css["audit_mismatches"] == 0
            assert cs["rows_skipped"] == css["rows_skipped"] and cs["bytes_stored"] == css["bytes_stored"], (cs, css)
            assert cs["verified"] and css["verified"]
            if i >= 1:
                assert sw["terminal_replicas"] == R, sw
                # Exactly: the observer's entry, and one per worker the token
                # reached.  A token delivery re-stamps the node's worker and
                # sends one note over the observer's 0 us link, which never
                # drops: delivered = 2 x token deliveries, and the token goes
                # round the ring, so it reached min(deliveries, N) workers.
                assert (ores["delivered"] % 2 == 0).all()
                want = int((1 + np.minimum(ores["delivered"] // 2, N)).sum())
                assert sw["slow_entries"] == want, (sw, want)
                assert cs["rows_skipped"] > 0 or N == 4, cs


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_after_a_terminal_sweep(engine_mod, oracle_mod, order, geo, R):
    """The records and the free stack of an ended replica are as the event
    kernel parked them, not as the pops would have left them.  Nothing reads
    them: a second tw_run is a no-op; a tie-mode change re-pilots over them;
    with the prefix off or the sweep off the next reset / run starts over them."""
    scn = _ring(40, R)
    other = "fifo" if order == "forkfirst" else "forkfirst"
    with _engine(engine_mod, scn, order, geo) as e:
        ores, oh = _oracle(oracle_mod, scn, order)
        for i in range(2):
            res, h, sw, cs = _step(e)
            _same((order, geo, i), res, h, ores, oh)
        assert sw["terminal_replicas"] == R
        e.run()
        assert e.sweep_stats()["killers"] == 0 and e.sweep_path_stats()["terminal_replicas"] == 0
        _same((order, geo, "again"), e.results(), e.hashes(), ores, oh)
        e.set_tie_mode(other)
        for i in range(2):
            res, h, sw, cs = _step(e)
            _same((other, geo, "re-pilot", i), res, h, *_oracle(oracle_mod, scn, other))
        assert sw["terminal_replicas"] == R
        e.set_tie_mode(order)
        res, h, sw, cs = _step(e)
        res, h, sw, cs = _step(e)
        assert sw["terminal_replicas"] == R
        e.set_prefix(False)
        res, h, sw, cs = _step(e)
        _same((order, geo, "prefix off"), res, h, ores, oh)
        _slow_counts(sw)
        e.set_prefix(True)
        res, h, sw, cs = _step(e)
        res, h, sw, cs = _step(e)
        assert sw["terminal_replicas"] == R
        e.set_sweep(False)
        res, h, sw, cs = _step(e)
        _same((order, geo, "sweep off"), res, h, ores, oh)
        assert sw["killers"] == 0 and sw["terminal_replicas"] == 0
        e.set_sweep(True)
        for i in range(2):
            res, h, sw, cs = _step(e)
            _same((order, geo, "sweep on", i), res, h, ores, oh)
        assert sw["terminal_replicas"] == R and cs["audit_mismatches"] == 0


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_cuts_through_the_sweep(engine_mod, oracle_mod, order, geo, R):
    """t_end = T then on to the end; t_end = T - 1 then reset (the sweep never
    fired); the event cap inside the sweep (refused) and the step after it."""
    scn = _ring(40, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    cap = int(ores["events"].min()) - 1
    res0, h0 = _off(engine_mod, scn, order, geo, max_events=cap)
    with _engine(engine_mod, scn, order, geo) as e:
        _step(e)
        res, h, sw, cs = _step(e, ({"t_end": T_KILL}, {}))
        _same((order, geo, "pieces"), res, h, ores, oh)
        assert sw["terminal_replicas"] == R and sw["killers"] == 41 * R
        res, h, sw, cs = _step(e, ({"t_end": T_KILL - 1},))
        assert sw["killers"] == 0 and sw["terminal_replicas"] == 0
        assert (res["status"] == isa.REP_RUNNING).all()
        res, h, sw, cs = _step(e)
        _same((order, geo, "after T - 1"), res, h, ores, oh)
        assert sw["terminal_replicas"] == R
        res, h, sw, cs = _step(e, ({"max_events": cap},))
        _same((order, geo, "cap"), res, h, res0, h0)
        assert sw["killers"] == 0 and sw["terminal_replicas"] == 0 and sw["fast_entries"] == 0
        for i in range(2):
            res, h, sw, cs = _step(e)
            _same((order, geo, "after cap", i), res, h, ores, oh)
            assert sw["terminal_replicas"] == R and cs["audit_mismatches"] == 0


# --------------------------------------------------------- hand-made programs
def _units_case(engine_mod, oracle_mod, monkeypatch, case, order, geo, R, drop_log2=1, K=40):
    scn = units(case, K, R, drop_log2)
    ores, oh = _oracle(oracle_mod, scn, order)
    out = None
    with _engine(engine_mod, scn, order, geo) as e, _slow_engine(engine_mod, monkeypatch, scn, order, geo) as es:
        for i in range(3):
            res, h, sw, cs = _step(e)
            ress, hs, sws, css = _step(es)
            print((case, order, geo, i), sw, cs)
            _same((case, order, geo, i), res, h, ores, oh)
            _same((case, order, geo, i, "slow"), ress, hs, ores, oh)
            _slow_counts(sws)
            assert sw["fast_entries"] + sw["slow_entries"] == sw["killers"] == sws["killers"], (sw, sws)
            assert sw["victims"] == sws["victims"] and sw["refused_replicas"] == 0
            assert cs["audit_mismatches"] == 0 and css["audit_mismatches"] == 0
            assert cs["rows_skipped"] == css["rows_skipped"] and cs["bytes_stored"] == css["bytes_stored"], (cs, css)
            out = (res, sw)
    return out


@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
@pytest.mark.parametrize("order", ORDERS)
def test_units_all_terminal(engine_mod, oracle_mod, monkeypatch, order, geo, R):
    """every server owns its listener and dies on the terminal path, from the effects rows"""
    K = 40
    res, sw = _units_case(engine_mod, oracle_mod, monkeypatch, "plain", order, geo, R)
    assert (res["status"] == isa.REP_DONE).all()
    assert sw["terminal_replicas"] == R and sw["killers"] == K * R and sw["victims"] == 2 * K * R
    assert sw["fast_entries"] == K * R, sw  # (the ping's handler touches no parked thread)


@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("drop_log2", [0, 1])
def test_surviving_thread(engine_mod, oracle_mod, monkeypatch, drop_log2, order, geo, R):
    """Where the ping arrives a thread sleeps past T: that replica is not ended
    by the sweep, keeps the general path, and its free stack must hold every
    freed slot exactly once -- the thread then forks more leaves than slots
    were free before the sweep -- and node 1's listener must be released (the
    late ping is undeliverable).  Where the ping is dropped the replica ends on
    the terminal path: with drop_log2 = 1 both kinds share every wave."""
    K = 40
    res, sw = _units_case(engine_mod, oracle_mod, monkeypatch, "survivor", order, geo, R, drop_log2)
    got = res["delivered"] > 0
    assert got.any() and (drop_log2 == 0 or not got.all())
    assert sw["terminal_replicas"] == int((~got).sum()), sw
    assert sw["killers"] == K * R and sw["victims"] == 2 * K * R
    # (the late ping finds no listener, unless its link drops it too)
    assert (res["undeliverable"][got] + res["dropped"][got] == 1).all() and res["undeliverable"][got].any()
    assert (res["undeliverable"][~got] == 0).all() and (res["dropped"][~got] == 1).all()
    assert sw["fast_entries"] == K * int((~got).sum()), sw


@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
@pytest.mark.parametrize("order", ORDERS)
def test_kill_wake_forked_after_the_snapshot(engine_mod, oracle_mod, monkeypatch, order, geo, R):
    """a kill wake at T that the table does not have: its refs come from its
    registers, the replica is not table-bound and keeps the general path"""
    K = 40
    res, sw = _units_case(engine_mod, oracle_mod, monkeypatch, "late_wake", order, geo, R)
    got = res["delivered"] > 0
    n = int(got.sum())
    assert 0 < n < R
    assert (res["status"] == isa.REP_DONE).all()
    assert sw["killers"] == K * R + n and sw["victims"] == 2 * K * R + n
    assert sw["terminal_replicas"] == R - n, sw


@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
@pytest.mark.parametrize("order", ORDERS)
def test_victim_named_by_two_kill_wakes(engine_mod, oracle_mod, monkeypatch, order, geo, R):
    """the table is not exclusive: no terminal path, the claim swap decides (V < H)"""
    K = 40
    res, sw = _units_case(engine_mod, oracle_mod, monkeypatch, "dup", order, geo, R)
    assert (res["status"] == isa.REP_DONE).all()
    assert sw["killers"] == 2 * K * R and sw["victims"] == 2 * K * R
    _slow_counts(sw)


@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
@pytest.mark.parametrize("order", ORDERS)
def test_recorded_refs_name_one_victim_twice(engine_mod, oracle_mod, monkeypatch, order, geo, R):
    """Unit 1's two positions are not claimable (a stale second ref), their
    refs are the recorded ones, and both name its sleeper: H = V + 1, and with
    the one thread that sleeps past T, live == killers + H holds although the
    sweep does not end the replica.  The table is not exclusive: no terminal
    path, the claim swap decides, and the replica goes on to T_LATE."""
    K = 40
    res, sw = _units_case(engine_mod, oracle_mod, monkeypatch, "stale_dup", order, geo, R)
    assert (res["status"] == isa.REP_DONE).all() and (res["final_t"] >= T_LATE).all()
    assert sw["killers"] == (K + 1) * R and sw["victims"] == (2 * K - 1) * R, sw
    _slow_counts(sw)


def test_frames_hook_changes_no_result(engine_mod, oracle_mod, monkeypatch):
    """TW_TEST_SWEEP_FRAMES=1 (validate loads every victim's frames quad): the
    same results, counts and paths as without it"""
    scn = _ring(40, 301)
    ores, oh = _oracle(oracle_mod, scn, "forkfirst")
    monkeypatch.setenv("TW_TEST_SWEEP_FRAMES", "1")
    ef = _engine(engine_mod, scn, "forkfirst", "dense")
    monkeypatch.delenv("TW_TEST_SWEEP_FRAMES")
    with ef, _engine(engine_mod, scn, "forkfirst", "dense") as e:
        for i in range(3):
            resf, hf, swf, csf = _step(ef)
            res, h, sw, cs = _step(e)
            _same(("frames", i), resf, hf, ores, oh)
            _same(("plain", i), res, h, ores, oh)
            assert swf == sw and csf == cs, (swf, sw, csf, cs)
        assert sw["terminal_replicas"] == 301
