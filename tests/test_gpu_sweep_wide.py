"""The sweep kernels at hundreds of kill wakes per replica against
the oracle: every result field and every node hash bit-exact, and
tw_sweep_stats with the exact counts.

tests/test_gpu_sweep.py sweeps at most 48 kill wakes per replica, fewer than
the waves a replica's prefix entries are dealt to.  With 64 replicas there is
one replica group and 256 such waves, so K kill wakes give a wave floor(K / 256)
entries or one more: the cases below put 0 to 6 entries in a wave (the shapes
a loop over several entries per trip, measured and not kept, would have to get
right at its tail too) and aim at what tw_sweep_apply does per entry:

* a replica refused beside swept ones in every wave, several entries deep;
* one victim named by two kill wakes, in one wave or in two, and by both refs
  of one killer: one 8-byte swap on the header's w2 and w3 claims;
* the hash terms of an entry on one node (one merged add) and on two;
* the free stack after a sweep holds every freed slot exactly once;
* a swept prefix that crosses its run's ring end.
"""
import functools

import numpy as np
import pytest

from timewarp import isa
from timewarp.abi import RESULT_FIELDS
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.timeunits import at, for_, sec

from test_gpu_teardown import sweep as td_sweep

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "forkfirst": 5}
ORDERS = ["fifo", "forkfirst"]
T_KILL = sec(20)   # beyond the 10 s on-chip horizon: the kill wakes queue in the far runs
T_LATE = sec(40)

_ORACLE = {}


def _oracle(oracle_mod, scn, order):
    key = (id(scn), order)  # (the builders are cached: one object per scenario)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


def _gpu(engine_mod, scn, order, geo, sweep_on=True):
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry=geo)
        e.set_tie_mode(order)
        if not sweep_on:
            e.set_sweep(False)
        e.reset()
        e.run()
        return e.results(), e.hashes(), e.sweep_stats()


def _same(tag, res, h, ores, oh):
    for f in FIELDS:
        assert np.array_equal(res[f], ores[f]), (tag, f, res[f][:6], ores[f][:6])
    assert np.array_equal(h, oh), tag


def _check(engine_mod, oracle_mod, scn, order, geo="dense"):
    res, h, st = _gpu(engine_mod, scn, order, geo)
    ores, oh = _oracle(oracle_mod, scn, order)
    _same((scn.name, order, geo), res, h, ores, oh)
    return res, h, st


# ---------------------------------------------------------- entries per wave
@pytest.mark.parametrize("geo,K", [("dense", 40), ("dense", 300), ("dense", 700), ("dense", 1100), ("dense", 1400),
                                   ("narrow", 1400), ("half", 1400)])
@pytest.mark.parametrize("order", ORDERS)
def test_entries_per_wave(engine_mod, oracle_mod, order, geo, K):
    """0-1, 1-2, 2-3, 4-5 and 5-6 entries in a wave.  Every replica is swept
    and ends DONE; the same outputs with the sweep switched off."""
    R = 64
    scn = td_sweep(K, n_replicas=R, run_capacity=8192)
    res, h, st = _check(engine_mod, oracle_mod, scn, order, geo)
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}
    assert (res["status"] == isa.REP_DONE).all()
    res0, h0, st0 = _gpu(engine_mod, scn, order, geo, sweep_on=False)
    assert st0 == {"killers": 0, "victims": 0, "refused_replicas": 0}
    _same(("off", K, order, geo), res0, h0, res, h)


@pytest.mark.parametrize("order", ORDERS)
def test_refusal_beside_swept_replicas(engine_mod, oracle_mod, order):
    """Replicas with replica % 3 != 0 hold sleepers that catch ThreadKilled:
    they are refused in every wave, each with four or five entries, and come
    out exactly as with the sweep off; the others of the wave are swept."""
    K, R = 1100, 64
    scn = td_sweep(K, n_replicas=R, victims="catch", run_capacity=8192)
    swept = len([r for r in range(R) if r % 3 == 0])
    res, h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": K * swept, "victims": 2 * K * swept, "refused_replicas": R - swept}
    res0, h0, _st0 = _gpu(engine_mod, scn, order, "dense", sweep_on=False)
    _same(("off", order), res0, h0, res, h)


@pytest.mark.parametrize("order", ORDERS)
def test_same_victim_from_two_entries(engine_mod, oracle_mod, order):
    """Two kill pairs per unit, 1,400 kill wakes: the two killers of a victim
    sit in one wave or in two; each victim is claimed once."""
    K, R = 700, 64
    scn = td_sweep(K, n_replicas=R, killers=2, run_capacity=8192)
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": 2 * K * R, "victims": 2 * K * R, "refused_replicas": 0}


@functools.lru_cache(maxsize=None)
def prog(case, K=300, n_replicas=70):
    """main forks K units, one per node; a unit forks a sleeper (r1) and a
    server (r2, owns the node's listener) and schedules its killers at T_KILL.

    dup: the killers are `throwTo r1; throwTo r1; END` and `throwTo r2; END`
    nodes: the sleeper of unit i is forked onto node (i + 1) mod K, the server
        and the kill pair stay on node i: the pair's terms go to two nodes,
        two of the three to one
    """
    p = Program()
    lset = p.listener_set({"ping": "on_ping"})
    c = p.function("main")
    c.seti(0, 0).seti(2, K)
    loop = c.here()
    c.fork("unit", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 2, loop)
    c.end()

    c = p.function("unit")
    if case == "nodes":
        c.mov(3, 0).addi(3, 1).modi(3, K)
        c.fork("sleeper", ref=1, node_reg=3)
    else:
        c.fork("sleeper", ref=1)
    c.fork("server", ref=2)
    if case == "dup":
        c.schedule(at(T_KILL), "kill_dup")
        c.schedule(at(T_KILL), "kill_server")
    else:
        c.schedule(at(T_KILL), "kill_pair")
    c.end()

    c = p.function("kill_pair")
    c.kill_thread(1).kill_thread(2).end()
    c = p.function("kill_dup")
    c.kill_thread(1).kill_thread(1).end()
    c = p.function("kill_server")
    c.kill_thread(2).end()
    c = p.function("sleeper")
    c.sleep_forever()
    c = p.function("server")
    c.listen(lset, owned=True)
    c.sleep_forever()
    c = p.function("on_ping")
    c.end()

    img = p.finalize()
    topo = Topology.from_out_lists(K + 1, [[] for _ in range(K + 1)])
    return Scenario(name=f"sweep_wide_{case}_{K}", image=img, topo=topo, n_replicas=n_replicas,
                    main_pc=img.pc_of("main"), main_node=K, max_slots=6 * K + 16, queue_capacity=8 * K + 64,
                    run_capacity=8192, max_frames=2)


@pytest.mark.parametrize("order", ORDERS)
def test_both_refs_of_a_killer_name_one_thread(engine_mod, oracle_mod, order):
    """`throwTo r1; throwTo r1; END`: the first ref claims the thread, the
    second finds its header dead.  One victim per killer."""
    K = 300
    scn = prog("dup", K)
    R = scn.n_replicas
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": 2 * K * R, "victims": 2 * K * R, "refused_replicas": 0}


@pytest.mark.parametrize("order", ORDERS)
def test_hash_terms_on_different_nodes(engine_mod, oracle_mod, order):
    """The killer and its server share a node, its sleeper is on the next one:
    the per-node merge adds two terms in one atomic and the third on its own."""
    K = 300
    scn = prog("nodes", K)
    R = scn.n_replicas
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}


# ------------------------------------------------------- the free stack after
@pytest.mark.parametrize("order", ORDERS)
def test_second_sweep_on_the_first_ones_free_stack(engine_mod, oracle_mod, order):
    """Even units kill at 40 s, odd ones at 20 s: the second sweep appends
    behind the free stack the first one left."""
    K, R = 300, 64
    scn = td_sweep(K, n_replicas=R, two_sweeps=True, run_capacity=8192)
    res, _h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}
    assert (res["status"] == isa.REP_DONE).all()


def _refill_prog(K, max_slots, n_replicas=64):
    """A unit forks its sleeper and server and is its own killer (`wait (at
    t); jmp kill_pair`), odd units at 20 s and even ones at 40 s: three threads
    per unit and main, 3 K + 1 at the most during start-up.  The first sweep
    frees 3 (K / 2) slots; at 30 s main forks as many short threads, which
    all live at once: again 3 K + 1 threads."""
    p = Program()
    lset = p.listener_set({"ping": "on_ping"})
    c = p.function("main")
    c.seti(0, 0).seti(2, K)
    loop = c.here()
    c.fork("unit", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 2, loop)
    c.wait(at(sec(30)))
    c.seti(0, 0).seti(2, 3 * (K // 2))
    loop2 = c.here()
    c.fork("short", ref=1)
    c.addi(0, 1).jlt(0, 2, loop2)
    c.end()

    c = p.function("unit")
    c.fork("sleeper", ref=1)
    c.fork("server", ref=2)
    c.mov(3, 0).modi(3, 2)
    late = c.label()
    c.jeqi(3, 0, late)
    c.wait(at(T_KILL)).jmp("kill_pair")
    c.bind(late)
    c.wait(at(T_LATE)).jmp("kill_pair")
    c = p.function("kill_pair")
    c.kill_thread(1).kill_thread(2).end()
    c = p.function("short")
    c.wait(for_(sec(1))).end()
    c = p.function("sleeper")
    c.sleep_forever()
    c = p.function("server")
    c.listen(lset, owned=True)
    c.sleep_forever()
    c = p.function("on_ping")
    c.end()

    img = p.finalize()
    topo = Topology.from_out_lists(K + 1, [[] for _ in range(K + 1)])
    return Scenario(name=f"sweep_wide_refill_{K}_{max_slots}", image=img, topo=topo, n_replicas=n_replicas,
                    main_pc=img.pc_of("main"), main_node=K, max_slots=max_slots, queue_capacity=8 * K + 64,
                    run_capacity=8192, max_frames=2)


@functools.lru_cache(maxsize=None)
def _refill_tight(oracle_mod, K, order):
    """the scenario with the fewest slots the oracle finishes it in (3 K + 1
    by the count above; found by the oracle, not assumed)"""
    for s in range(3 * K - 2, 3 * K + 6):
        scn = _refill_prog(K, s)
        if int(oracle_mod.run(scn, replica=0, mode=ORACLE_MODE[order]).result["status"]) == isa.REP_DONE:
            return scn
    raise AssertionError("no slot count near 3 K + 1 lets the oracle finish")


@pytest.mark.parametrize("order", ORDERS)
def test_no_slot_lost_or_doubled(engine_mod, oracle_mod, order):
    """With one slot fewer the oracle runs out of slots, so the short threads
    forked after the first sweep fit only if every slot it freed came back:
    a slot lost ends in ERR_SLOTS, a slot handed out twice in two threads on
    one record."""
    K, R = 300, 64
    scn = _refill_tight(oracle_mod, K, order)
    fewer = _refill_prog(K, scn.max_slots - 1)
    assert int(oracle_mod.run(fewer, replica=0, mode=ORACLE_MODE[order]).result["status"]) == isa.REP_ERR_SLOTS
    res, _h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}
    assert (res["status"] == isa.REP_DONE).all()


# ------------------------------------------------------------ ring wrap-around
@functools.lru_cache(maxsize=None)
def _wrap_prog(K=700, P=600, run_capacity=1024, n_replicas=64):
    """The kill wakes' run has popped P entries before they are pushed, so
    the swept prefix starts at ring position P + 1 of 1,024 and its entry 423
    is at position 0: between two entries of every wave (y, y + 256, y + 512).

    How the run gets there (run_push: an entry goes to the non-empty run with
    the largest tail <= its key, else to the first empty run).  At time 0 main
    forks `far2` (wakes at 50 s), P threads `pre` (12 s) and `anchor` (25 s) and
    waits until 13 s; its own entry is pushed first: run 0 = [13 s].  far2:
    run 0 = [13, 50].  pre: below run 0's tail, so run 1 = [12 x P]; anchor:
    run 1 = [12 x P, 25].  At 12 s the P pops move run 1's head to P.  At 13 s
    main forks the K units: their sleepers and servers park 100,500 min ahead,
    on run 0 (tail 50 s, the largest); the kill wakes at 30 s do not fit there
    and go behind the anchor: run 1 = [25, 30 x K] from position P.  The
    anchor pops at 25 s; the sweep at 30 s takes positions P + 1 .. P + K
    modulo the capacity.  (As in test_restamp_run_changes, the case compares
    results only: this derivation is what ties it to its name.)"""
    t_kill = sec(30)
    p = Program()
    lset = p.listener_set({"ping": "on_ping"})
    c = p.function("main")
    c.fork("far2", ref=1)
    c.seti(0, 0).seti(2, P)
    loop = c.here()
    c.fork("pre", ref=1)
    c.addi(0, 1).jlt(0, 2, loop)
    c.fork("anchor", ref=1)
    c.wait(at(sec(13)))
    c.seti(0, 0).seti(2, K)
    loop2 = c.here()
    c.fork("unit", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 2, loop2)
    c.end()

    c = p.function("far2")
    c.wait(at(sec(50))).end()
    c = p.function("pre")
    c.wait(at(sec(12))).end()
    c = p.function("anchor")
    c.wait(at(sec(25))).end()
    c = p.function("unit")
    c.fork("sleeper", ref=1)
    c.fork("server", ref=2)
    c.schedule(at(t_kill), "kill_pair")
    c.end()
    c = p.function("kill_pair")
    c.kill_thread(1).kill_thread(2).end()
    c = p.function("sleeper")
    c.sleep_forever()
    c = p.function("server")
    c.listen(lset, owned=True)
    c.sleep_forever()
    c = p.function("on_ping")
    c.end()

    img = p.finalize()
    topo = Topology.from_out_lists(K + 1, [[] for _ in range(K + 1)])
    return Scenario(name=f"sweep_wide_wrap_{K}_{P}_{run_capacity}", image=img, topo=topo, n_replicas=n_replicas,
                    main_pc=img.pc_of("main"), main_node=K, max_slots=6 * K + 16, queue_capacity=8 * K + 64,
                    run_capacity=run_capacity, max_frames=2)


@pytest.mark.parametrize("order", ORDERS)
def test_prefix_wraps_around_the_ring(engine_mod, oracle_mod, order):
    K, R = 700, 64
    scn = _wrap_prog(K)
    res, h, st = _check(engine_mod, oracle_mod, scn, order)
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}
    res0, h0, _st0 = _gpu(engine_mod, scn, order, "dense", sweep_on=False)
    _same(("off", order), res0, h0, res, h)
