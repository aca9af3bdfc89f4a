"""Kill sweeps -- the shape of token-ring's teardown (`schedule (at
launchDuration) $ mapM_ killThread [wtid, stid]`, examples/token-ring/Main.hs:
124-127) -- against the oracle, every result field and node hash bit-exact.

K killers wake at one absolute time; each resumes at `throwTo r1; throwTo r2;
END` and kills two sleepers parked in `sleepForever`, one of which owns its
node's listener.  Every victim is re-stamped to (now, fresh seq), pops later
with its pending ThreadKilled and dies.  The cases pin the paths the run
geometries take through such a sweep:

* reap iterations: a wave none of whose lanes has a thread to run after the
  pop phase skips the step and its store tail -- alone (plain sweeps), mixed
  with ordinary iterations (token-ring with drops: lanes enter the teardown at
  different iterations) and with running lanes in the same wave (victims that
  catch the exception, by replica);
* re-stamps that change far runs: the run that took the lane's last re-stamp
  is full, empty, or its tail has moved past the key (a thread parked far
  ahead in between, LIFO's falling keys) -- the shapes a re-stamp hint would
  have to give up on (measured, not kept);
* cuts through the sweep: t_end, the event cap, a launch boundary;
* the 2^22-instruction step cap on a kill pair's second throwTo and on its END
  (the interpreter's count: no new code).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from timewarp import isa, scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.timeunits import at, for_, sec

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "lifo": 2, "forkfirst": 5}  # oracle MODE_CANONICAL, MODE_LIFO, MODE_FORKFIRST
ORDERS = ["fifo", "forkfirst", "lifo"]
T_KILL = sec(20)   # beyond the 10 s on-chip horizon: the kill wakes queue in the far runs
T_LATE = sec(40)
TK = isa.EXC_THREAD_KILLED


@functools.lru_cache(maxsize=None)
def sweep(K, n_replicas=64, killer="pair", victims="plain", killers=1, waiter=False, two_sweeps=False,
          run_capacity=256):
    """main forks K units, one per node; a unit forks a sleeper and a server
    (which owns the node's listener) and schedules its killer(s) at T_KILL.

    killer: "pair" (`throwTo r1; throwTo r2; END`), "one" (`throwTo r1; END`),
        "self" (the pair's second victim is the killer itself)
    victims: "plain", or "catch": the sleepers of replicas whose r3 (main's
        registers, replica % 3) is not 0 catch ThreadKilled, trace and end
    killers: killers per unit (2: every victim is re-stamped twice, the first
        re-stamp pops superseded)
    waiter: odd units also schedule, at T_KILL, a thread that parks 1,000 s
        ahead -- on the run the re-stamps go to, whose tail then lies past the
        next re-stamp's key
    two_sweeps: even units kill at T_LATE; the run that took the first sweep's
        re-stamps is empty when the second begins
    """
    p = Program()
    lset = p.listener_set({"ping": "on_ping"})
    c = p.function("main")
    c.seti(0, 0).seti(2, K)
    loop = c.here()
    c.fork("unit", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 2, loop)
    c.end()

    target = {"pair": "kill_pair", "one": "kill_one", "self": "kill_self"}[killer]
    c = p.function("unit")
    c.fork("sleeper", ref=1)
    c.fork("server", ref=2)
    late = c.label()
    if waiter or two_sweeps:
        c.mov(3, 0).modi(3, 2)
    if two_sweeps:
        c.jeqi(3, 0, late)
    if waiter:
        skip = c.label()
        c.jeqi(3, 0, skip)
        c.schedule(at(T_KILL), "far_waiter")
        c.bind(skip)
    for _ in range(killers):
        if killer == "self":
            c.fork_("self_stub")
        else:
            c.schedule(at(T_KILL), target)
    if killer != "pair":
        c.schedule(at(T_KILL), "kill_server")  # (the server must end too, or the run never does)
    c.end()
    c.bind(late)
    c.schedule(at(T_LATE), target)
    c.end()

    c = p.function("kill_pair")
    c.kill_thread(1).kill_thread(2).end()
    c = p.function("kill_one")
    c.kill_thread(1).end()
    c = p.function("kill_server")
    c.kill_thread(2).end()
    c = p.function("self_stub")        # `schedule`'s stub, with the killer's own ref in r3
    c.my_thread_id(3).wait(at(T_KILL)).jmp("kill_self")
    c = p.function("kill_self")
    c.kill_thread(1).kill_thread(3).end()
    c = p.function("far_waiter")
    c.wait(for_(sec(1000))).end()

    c = p.function("sleeper")
    plain = c.label()
    if victims == "catch":
        c.jeqi(3, 0, plain)
        c.catch_(1 << TK, "sleeper_h")
        c.sleep_forever()
    c.bind(plain)
    c.sleep_forever()
    c = p.function("sleeper_h")
    c.trace(7, 0).trace(8, 3).end()
    c = p.function("server")
    c.listen(lset, owned=True)
    c.sleep_forever()
    c = p.function("on_ping")
    c.end()

    img = p.finalize()
    topo = Topology.from_out_lists(K + 1, [[] for _ in range(K + 1)])
    regs = np.zeros((n_replicas, 4), np.int64)
    if victims == "catch":
        regs[:, 3] = np.arange(n_replicas) % 3
    return Scenario(name=f"sweep_{K}_{killer}_{victims}_{killers}_{int(waiter)}_{int(two_sweeps)}_{run_capacity}",
                    image=img, topo=topo, n_replicas=n_replicas, main_pc=img.pc_of("main"), main_node=K,
                    main_regs=regs, max_slots=6 * K + 16, queue_capacity=8 * K + 64, run_capacity=run_capacity,
                    max_frames=2)


_ORACLE = {}


def _oracle(oracle_mod, scn, order):
    """the oracle's full run of a scenario, computed once per (scenario name, order)"""
    key = (scn.name, scn.n_replicas, order)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


def _gpu(engine_mod, scn, order, geo, **run):
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry=geo)
        e.set_tie_mode(order).reset()
        e.run(**run)
        return e.results(), e.hashes()


def _same(tag, res, h, ores, oh):
    for f in FIELDS:
        assert np.array_equal(res[f], ores[f]), (tag, f, res[f][:6], ores[f][:6])
    assert np.array_equal(h, oh), tag


def _check(engine_mod, oracle_mod, scn, order, geo):
    res, h = _gpu(engine_mod, scn, order, geo)
    ores, oh = _oracle(oracle_mod, scn, order)
    _same((scn.name, order, geo), res, h, ores, oh)
    return res


@pytest.mark.parametrize("geo", ["dense", "narrow", "half", "sparse", "compact"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("K", [4, 40])
def test_kill_sweep(engine_mod, oracle_mod, K, order, geo):
    """K = 4: every re-stamp fits the on-chip queue; K = 40: 80 victims, most
    re-stamped into the far runs (the dense queue holds 16)."""
    res = _check(engine_mod, oracle_mod, sweep(K), order, geo)
    assert (res["final_t"] == T_KILL).all() and (res["threads"] == 1 + 4 * K).all()


@functools.lru_cache(maxsize=None)
def _ring():
    return scenarios.token_ring(n_nodes=16, n_replicas=128, drop_log2=2, link_depth=4)


@pytest.mark.parametrize("geo", ["dense", "narrow", "half"])
@pytest.mark.parametrize("order", ORDERS)
def test_mixed_waves(engine_mod, oracle_mod, order, geo):
    """token-ring with every fourth send dropped: the replicas of a wave reach
    the teardown at different iterations, so its waves alternate between reap
    and ordinary iterations."""
    res = _check(engine_mod, oracle_mod, _ring(), order, geo)
    assert res["dropped"].sum() > 0


@pytest.mark.parametrize("geo", ["dense", "half", "sparse"])
@pytest.mark.parametrize("order", ORDERS)
def test_victims_that_catch(engine_mod, oracle_mod, order, geo):
    """Two of three replicas' sleepers catch ThreadKilled and run a handler
    with a trace: dying lanes and running lanes share a wave."""
    _check(engine_mod, oracle_mod, sweep(24, n_replicas=128, victims="catch"), order, geo)


@pytest.mark.parametrize("geo", ["dense", "narrow"])
@pytest.mark.parametrize("order", ORDERS)
def test_victim_restamped_twice(engine_mod, oracle_mod, order, geo):
    """Two killers per unit: the second re-stamps victims that are still
    queued, and the first re-stamp's entry pops superseded during the sweep."""
    _check(engine_mod, oracle_mod, sweep(24, killers=2), order, geo)


@pytest.mark.parametrize("geo", ["dense", "narrow"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", ["full", "tail_moved", "empty"])
def test_restamp_run_changes(engine_mod, oracle_mod, case, order, geo):
    """(The shapes that would defeat a re-stamp hint -- "try the run of the
    last re-stamp first"; that change was measured and not kept, DESIGN 3j,
    and the shapes stay as sweeps whose re-stamps change runs.)
    The run that took the last re-stamp cannot take the next one: it is
    full (run_capacity below the victim count: re-stamps go on to other runs
    and the heap), its tail moved past the key (a thread parked 1,000 s ahead
    landed on it between two kills), or it is empty (a second sweep after the
    first one's run was popped out).

    How each case reaches its fallback (dense / narrow: 16 on-chip entries, a
    10 s on-chip horizon; fifo and forkfirst -- under lifo every re-stamp's
    key is below the last one's, so the hint misses from the second on):
    the first eight kill wakes fill the on-chip queue with their 16 victims,
    so the other 64 re-stamps are far pushes, and the kill wakes' own run
    (tail (T_KILL, older seq) <= every re-stamp key) takes the first and
    becomes the hint.
    full: a run holds 24 entries, fewer than the 40 kill wakes or the 64 far
    re-stamps, so whichever run is hinted reaches capacity during the sweep
    and the re-stamps move on to the other runs and, when those fill, the heap.
    tail_moved: an odd unit's far_waiter pops between two kill wakes and parks
    at T_KILL + 1,000 s, beyond the horizon: a far push whose best run (largest
    tail <= key) is the hinted one (the sleepers' run ends at 100,500 min); the
    next re-stamp's key (T_KILL, ..) is below that tail.
    empty: units alternate T_LATE / T_KILL, so startup builds one run per kill
    time; the T_KILL run takes the first sweep's re-stamps and is popped out by
    its end, and at T_LATE the hint still names it.
    The cases compare results with the oracle; they do not read the engine's
    push counters, so the derivation above is what ties them to their names."""
    scn = {"full": lambda: sweep(40, run_capacity=24),
           "tail_moved": lambda: sweep(40, waiter=True),
           "empty": lambda: sweep(40, two_sweeps=True)}[case]()
    _check(engine_mod, oracle_mod, scn, order, geo)


@pytest.mark.parametrize("killer", ["one", "self"])
@pytest.mark.parametrize("order", ORDERS)
def test_kill_stub_shapes(engine_mod, oracle_mod, order, killer):
    """A kill stub with one throwTo, and one whose second victim is the killer."""
    _check(engine_mod, oracle_mod, sweep(24, killer=killer), order, "dense")


@pytest.mark.parametrize("geo", ["dense", "half"])
@pytest.mark.parametrize("order", ["fifo", "forkfirst"])
def test_cut_by_t_end_and_event_cap(engine_mod, oracle_mod, order, geo):
    """A sweep runs at one timestamp, so t_end cuts before it, at it (the run
    stops with the sweep done) or not at all; inside it the run is cut by the
    event cap.  Each replica at t_end = T_KILL against the oracle cut there;
    then the run in pieces -- up to the sweep, into the middle of the killers,
    into the middle of the victims, to the end -- against the whole run."""
    K = 40
    scn = sweep(K)
    res, h = _gpu(engine_mod, scn, order, geo, t_end=T_KILL)
    o = oracle_mod.run(scn, replica=3, mode=ORACLE_MODE[order], t_end=T_KILL)
    for f in FIELDS:
        assert (res[f] == o.result[f]).all(), (f, res[f][:4], o.result[f])
    assert (h == o.hashes[None, :]).all()
    ores, oh = _oracle(oracle_mod, scn, order)
    total = int(ores["events"][0])
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry=geo)
        e.set_tie_mode(order).reset()
        e.run(t_end=T_KILL - 1)
        before = int(e.results()["events"][0])
        assert total - before == 3 * K  # the sweep: K kill wakes, 2K victims
        e.run(max_events=before + K // 2)
        e.run(max_events=before + K + K // 2 + 1)
        e.run(t_end=T_KILL - 1)  # nothing left before the sweep: no event
        assert int(e.results()["events"][0]) == before + K + K // 2 + 1
        e.run()
        _same((scn.name, order, geo, "pieces"), e.results(), e.hashes(), ores, oh)


_CHILD = """
import sys
import numpy as np
sys.path[:0] = {paths!r}
import test_gpu_teardown as T
from timewarp import engine
scn = T.sweep(40)
with engine.Engine(0) as e:
    e.load(scn, geometry={geo!r})
    e.set_tie_mode({order!r}).reset()
    st = e.run()
    res, h = e.results(), e.hashes()
np.savez({out!r}, res=res, h=h, launches=np.array([st.launches]))
"""


@pytest.mark.parametrize("geo,order", [("dense", "forkfirst"), ("narrow", "fifo")])
def test_launch_boundary_in_the_sweep(engine_mod, oracle_mod, monkeypatch, tmp_path, geo, order):
    """TW_LAUNCH_BUDGET = 50 iterations per launch: the 120 pops of the sweep
    span launches, so a launch ends and the next begins among reap iterations.
    (The library reads the budget once per process: a fresh one runs the case.)"""
    monkeypatch.setenv("TW_LAUNCH_BUDGET", "50")
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "r.npz")
    src = _CHILD.format(paths=[here] + [p for p in sys.path if p], geo=geo, order=order, out=out)
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(z["launches"][0]) > 4
    ores, oh = _oracle(oracle_mod, sweep(40), order)
    _same(("budget", geo, order), z["res"], z["h"], ores, oh)


def _cap_kill_prog(k, pad):
    """main forks two sleepers, then in one step counts to k and runs the kill
    pair: 3 + pad + 2k instructions before the first throwTo, so the
    2^22-instruction cap falls on the pair's second throwTo or on its END."""
    p = Program()
    c = p.function("main")
    c.fork("sleeper", ref=2).fork("sleeper", ref=3)
    c.wait(for_(10))
    c.seti(0, 0).seti(1, k)
    if pad:
        c.now(0).seti(0, 0)
    top = c.here()
    c.addi(0, 1).jlt(0, 1, top)
    c.kill_thread(2).kill_thread(3).end()
    c = p.function("sleeper")
    c.sleep_forever()
    img = p.finalize()
    topo = Topology.from_out_lists(1, [[]])
    return Scenario(name=f"cap_kill_{k}_{pad}", image=img, topo=topo, n_replicas=2, main_pc=img.pc_of("main"),
                    main_node=0, max_slots=8, queue_capacity=64, run_capacity=16)


@pytest.mark.parametrize("k,pad", [(2097149, 0), (2097150, 0), (2097148, 1), (2097149, 1)])
def test_step_cap_on_the_kill_pair(engine_mod, oracle_mod, k, pad):
    """throwTo at counts n, n + 1 and END at n + 2, n = 3 + 2 pad + 2k: the
    step fits under the cap of 2^22 with END on it, or the cap falls on END
    (pad 0) / on the second throwTo (pad 1).  The pair runs inside main's long
    step through the interpreter, on victims in the on-chip queue: this pins
    the cap's count on a kill pair for any engine (it covers no code of the
    reap iterations or the hinted append, and would cover a kill stub carried
    out at the pop only through the stub's flagging of `kill pair; END`)."""
    scn = _cap_kill_prog(k, pad)
    st, res, h = engine_mod.run_scenario(scn, geometry="dense")
    o = oracle_mod.run(scn)
    for f in FIELDS:
        assert res[f][0] == o.result[f], (k, pad, f, res[f][0], o.result[f])
    assert np.array_equal(h[0], o.hashes)
    n_end = 3 + 2 * pad + 2 * k + 2
    assert (int(o.result["status"]) == isa.REP_ERR_INSN) == (n_end > 1 << 22), (k, pad, o.result["status"])
