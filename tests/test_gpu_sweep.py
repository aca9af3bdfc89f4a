"""Same-time killThread sweeps in data-parallel kernels against the
oracle: every result field and every node hash bit-exact, and tw_sweep_stats
saying whether the sweep kernels or the event kernel's one-pop-at-a-time path
carried the kill wakes out.

The kill time is 20 s, beyond the 10 s on-chip horizon, so the kill wakes
queue in the far runs (the only place a sweep takes them from).  Programs are
built the way tests/test_gpu_teardown.py builds them: main forks K units, a
unit forks its victims and schedules its killer(s) at the kill time.  64
replicas are one full wave, 70 a full and a partial one.

A replica is swept only when every event at the kill time is a kill-stub wake
whose victims are plain (queued, started, not main, no frame that catches or
finalises, nothing pending, not themselves kill wakes); the refusal cases break
one condition each and still match the oracle, on the sequential path.
"""
import functools

import numpy as np
import pytest

from timewarp import isa, scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.timeunits import at, for_, sec

from test_gpu_teardown import sweep as td_sweep

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "lifo": 2, "forkfirst": 5}
T_KILL = sec(20)
T_LATE = sec(40)
TK = isa.EXC_THREAD_KILLED
SWEPT_GEOS = ["dense", "narrow", "half"]
SWEPT_ORDERS = ["fifo", "forkfirst"]

_ORACLE = {}


def _oracle(oracle_mod, scn, order="fifo"):
    key = (id(scn), order)  # (the builders are cached: one object per scenario)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


def _gpu(engine_mod, scn, order, geo, sweep_on=True, runs=({},)):
    """results, hashes and tw_sweep_stats summed over the tw_run calls `runs`"""
    tot = {"killers": 0, "victims": 0, "refused_replicas": 0}
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry=geo)
        e.set_tie_mode(order)
        if not sweep_on:
            e.set_sweep(False)
        e.reset()
        for kw in runs:
            e.run(**kw)
            for k, v in e.sweep_stats().items():
                tot[k] += v
        return e.results(), e.hashes(), tot


def _same(tag, res, h, ores, oh):
    for f in FIELDS:
        assert np.array_equal(res[f], ores[f]), (tag, f, res[f][:6], ores[f][:6])
    assert np.array_equal(h, oh), tag


def _check(engine_mod, oracle_mod, scn, order, geo, **kw):
    res, h, st = _gpu(engine_mod, scn, order, geo, **kw)
    ores, oh = _oracle(oracle_mod, scn, order)
    _same((scn.name, order, geo), res, h, ores, oh)
    return res, h, st


# ------------------------------------------------------------ the sweep fires
@functools.lru_cache(maxsize=None)
def _ring(n_nodes, n_replicas=70, launch_duration=T_KILL):
    return scenarios.token_ring(n_nodes=n_nodes, n_replicas=n_replicas, launch_duration=launch_duration,
                                drop_log2=3, link_depth=4)


@pytest.mark.parametrize("geo", SWEPT_GEOS)
@pytest.mark.parametrize("order", SWEPT_ORDERS)
@pytest.mark.parametrize("N", [4, 40])
def test_token_ring_teardown_is_swept(engine_mod, oracle_mod, N, order, geo):
    """N ring nodes and the observer each schedule a kill pair: N + 1 kill
    wakes and 2 (N + 1) victims per replica, no replica refused; the same
    outputs with the sweep switched off."""
    scn = _ring(N)
    R = scn.n_replicas
    res, h, st = _check(engine_mod, oracle_mod, scn, order, geo)
    assert st == {"killers": R * (N + 1), "victims": 2 * R * (N + 1), "refused_replicas": 0}
    res0, h0, st0 = _gpu(engine_mod, scn, order, geo, sweep_on=False)
    assert st0 == {"killers": 0, "victims": 0, "refused_replicas": 0}
    _same(("off", N, order, geo), res0, h0, res, h)


@pytest.mark.parametrize("geo", SWEPT_GEOS)
@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_one_throwto_stubs(engine_mod, oracle_mod, order, geo):
    """`throwTo r1; END` and `throwTo r2; END`: two kill wakes per unit."""
    K, R = 24, 64
    _r, _h, st = _check(engine_mod, oracle_mod, td_sweep(K, n_replicas=R, killer="one"), order, geo)
    assert st == {"killers": 2 * K * R, "victims": 2 * K * R, "refused_replicas": 0}


@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_two_killers_name_one_victim(engine_mod, oracle_mod, order):
    """Two kill pairs per unit: every victim is hit twice and dies once."""
    K, R = 24, 70
    _r, _h, st = _check(engine_mod, oracle_mod, td_sweep(K, n_replicas=R, killers=2), order, "dense")
    assert st == {"killers": 2 * K * R, "victims": 2 * K * R, "refused_replicas": 0}


@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_two_sweep_times(engine_mod, oracle_mod, order):
    """Even units kill at 40 s, odd ones at 20 s: two sweeps in one tw_run."""
    K, R = 24, 64
    _r, _h, st = _check(engine_mod, oracle_mod, td_sweep(K, n_replicas=R, two_sweeps=True), order, "dense")
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}


@functools.lru_cache(maxsize=None)
def prog(case, K=12, n_replicas=70):
    """main forks K units, one per node; a unit forks a sleeper (r1) and a
    second thread (r2) and schedules a kill pair on them at T_KILL.

    stale: r2 names a thread that ended at once (a stale ref: a no-op)
    finally: the sleeper sleeps inside a `timeout` (a finally frame)
    main: r2 is main's ref (main sleeps forever after its forks)
    chain: r2 is another kill wake of the same sweep
    """
    p = Program()
    c = p.function("main")
    if case == "main":
        c.my_thread_id(2)
    c.seti(0, 0).seti(3, K)
    loop = c.here()
    c.fork("unit", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 3, loop)
    if case == "main":
        c.sleep_forever()
    else:
        c.end()

    c = p.function("unit")
    c.fork("sleeper", ref=1)
    if case == "stale":
        c.fork("quick", ref=2)
    elif case == "chain":
        c.fork("stub_one", ref=2)
    elif case != "main":
        c.fork("sleeper2", ref=2)
    c.schedule(at(T_KILL), "kill_pair")
    c.end()

    c = p.function("kill_pair")
    c.kill_thread(1).kill_thread(2).end()
    c = p.function("stub_one")          # `schedule`'s stub, forked with a ref
    c.wait(at(T_KILL)).jmp("kill_one")
    c = p.function("kill_one")
    c.kill_thread(1).end()
    c = p.function("quick")
    c.end()
    c = p.function("sleeper")
    if case == "finally":
        c.timeout_begin(sec(1000), epoch_reg=3)
        c.wait(for_(sec(500)))
        c.timeout_end()
        c.end()
    else:
        c.sleep_forever()
    c = p.function("sleeper2")
    c.sleep_forever()

    img = p.finalize()
    topo = Topology.from_out_lists(K + 1, [[] for _ in range(K + 1)])
    return Scenario(name=f"sweep_prog_{case}_{K}", image=img, topo=topo, n_replicas=n_replicas,
                    main_pc=img.pc_of("main"), main_node=K, max_slots=8 * K + 16, queue_capacity=8 * K + 64,
                    run_capacity=256, max_frames=2, max_timeouts=2 * K + 4)


@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_stale_ref(engine_mod, oracle_mod, order):
    K = 12
    scn = prog("stale", K)
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order, "dense")
    assert st == {"killers": K * scn.n_replicas, "victims": K * scn.n_replicas, "refused_replicas": 0}


@pytest.mark.parametrize("geo", ["dense", "half"])
@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_t_end_at_the_sweep_and_split_runs(engine_mod, oracle_mod, order, geo):
    """t_end == T: the sweep runs and the run stops behind it, as the oracle
    cut there; t_end == T - 1: no sweep; a run in pieces around T."""
    K, R = 24, 70
    scn = td_sweep(K, n_replicas=R)
    o = oracle_mod.run(scn, replica=5, mode=ORACLE_MODE[order], t_end=T_KILL)
    res, h, st = _gpu(engine_mod, scn, order, geo, runs=({"t_end": T_KILL},))
    for f in FIELDS:
        assert (res[f] == o.result[f]).all(), (f, res[f][:4], o.result[f])
    assert (h == o.hashes[None, :]).all()
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}
    o = oracle_mod.run(scn, replica=5, mode=ORACLE_MODE[order], t_end=T_KILL - 1)
    res, h, st = _gpu(engine_mod, scn, order, geo, runs=({"t_end": T_KILL - 1},))
    for f in FIELDS:
        assert (res[f] == o.result[f]).all(), (f, res[f][:4], o.result[f])
    assert (h == o.hashes[None, :]).all()
    assert st == {"killers": 0, "victims": 0, "refused_replicas": 0}
    pieces = ({"t_end": sec(5)}, {"t_end": T_KILL - 1}, {"t_end": T_KILL - 1}, {"t_end": T_KILL}, {})
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order, geo, runs=pieces)
    assert st == {"killers": K * R, "victims": 2 * K * R, "refused_replicas": 0}


# ------------------------------------------------- refused, or not attempted
@pytest.mark.parametrize("geo", ["dense", "half"])
@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_victims_that_catch_are_refused_by_replica(engine_mod, oracle_mod, order, geo):
    """The sleepers of replicas with main register r3 = replica % 3 != 0 catch
    ThreadKilled: those replicas are refused, the others of the same wave swept."""
    K, R = 12, 70
    scn = td_sweep(K, n_replicas=R, victims="catch")
    swept = len([r for r in range(R) if r % 3 == 0])
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order, geo)
    assert st == {"killers": K * swept, "victims": 2 * K * swept, "refused_replicas": R - swept}


@pytest.mark.parametrize("case", ["finally", "main", "chain"])
@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_refused_victims(engine_mod, oracle_mod, order, case):
    """A victim inside a `timeout`, a victim that is main, a kill wake killed
    by another kill wake of the same sweep: every replica is refused."""
    scn = prog(case)
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order, "dense")
    assert st == {"killers": 0, "victims": 0, "refused_replicas": scn.n_replicas}


@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_self_victim_and_other_wakes_at_the_sweep(engine_mod, oracle_mod, order):
    """A stub whose second victim is the killer itself; a thread that is no
    kill stub waking at exactly T (odd units' far_waiter)."""
    for scn in (td_sweep(24, n_replicas=64, killer="self"), td_sweep(24, n_replicas=64, waiter=True)):
        _r, _h, st = _check(engine_mod, oracle_mod, scn, order, "dense")
        assert st == {"killers": 0, "victims": 0, "refused_replicas": 64}


@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_event_cap_inside_the_sweep(engine_mod, oracle_mod, order):
    """max_events falls among the kill wakes: the sweep is refused and the
    counts are the oracle's at the cap.  Then, resumed with victims whose
    exception is already pending: refused again, and the whole run matches."""
    K, R = 24, 64
    scn = td_sweep(K, n_replicas=R)
    ores, oh = _oracle(oracle_mod, scn, order)
    before = int(ores["events"][0]) - 3 * K
    cap = before + K // 2
    o = oracle_mod.run(scn, replica=2, mode=ORACLE_MODE[order], max_events=cap)
    res, h, st = _gpu(engine_mod, scn, order, "dense", runs=({"max_events": cap},))
    for f in FIELDS:
        assert (res[f] == o.result[f]).all(), (f, res[f][:4], o.result[f])
    assert (h == o.hashes[None, :]).all()
    assert st == {"killers": 0, "victims": 0, "refused_replicas": R}
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry="dense")
        e.set_tie_mode(order).set_sweep(False).reset()
        e.run(max_events=cap)   # sequential: K / 2 kill wakes done, their victims pending
        e.set_sweep(True)
        e.run()
        st = e.sweep_stats()
        _same((scn.name, order, "pending"), e.results(), e.hashes(), ores, oh)
    assert st["killers"] == 0 and st["victims"] == 0 and st["refused_replicas"] == R


@pytest.mark.parametrize("order", SWEPT_ORDERS)
def test_wakes_in_the_near_heap(engine_mod, oracle_mod, order):
    """launch_duration below the on-chip horizon: the kill wakes sit in the
    near heap, where a sweep does not reach."""
    scn = _ring(4, launch_duration=sec(5))
    _r, _h, st = _check(engine_mod, oracle_mod, scn, order, "dense")
    assert st["killers"] == 0 and st["victims"] == 0


@pytest.mark.parametrize("geo,order", [("dense", "lifo"), ("compact", "fifo"), ("sparse", "fifo"), ("wave", "fifo"),
                                       ("lpb", "fifo")])
def test_paths_without_sweeps(engine_mod, oracle_mod, geo, order):
    """LIFO and the geometries without far-run sweeps: nothing attempted."""
    scn = _ring(4, n_replicas=64)
    if geo == "lpb":
        with engine_mod.Engine(0) as e:
            e.load(scn, geometry="lpb")
            e.reset()
            e.run()
            res, h, st = e.results(), e.hashes(), e.sweep_stats()
    else:
        res, h, st = _gpu(engine_mod, scn, order, geo)
    ores, oh = _oracle(oracle_mod, scn, order)
    _same((geo, order), res, h, ores, oh)
    assert st == {"killers": 0, "victims": 0, "refused_replicas": 0}
