"""The send-free prefix against the oracle and against the same
context with the prefix switched off: every result field and every node hash
bit-exact, and tw_prefix_stats saying what each run did.

Until its first SEND a replica reads nothing of its own, so the first fresh
run that reaches T0 - 1 (T0: the load-time bound on the first send, 1 s for
the token ring) runs that stretch on one workgroup, snapshots replica 0 and
stores the snapshot to every replica (piloted); later reset / run pairs store
the cached snapshot (applied).  The rings drop one message in four
(drop_log2=2), so replicas really differ behind the prefix.  301 replicas are
more than one dense or half workgroup, 70 more than one narrow one, and
neither is a multiple of 4: rows of 4-byte arrays start unaligned.
"""
import functools

import numpy as np
import pytest

from timewarp import isa, scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.timeunits import for_, ms, sec

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "lifo": 2, "forkfirst": 5}
T_KILL = sec(20)
T0 = sec(1)  # node 0's `invoke (after 1 sec)`: tests/test_prefix_host.py
GEOS = [("dense", 301), ("narrow", 70), ("half", 301)]
ORDERS = ["fifo", "forkfirst"]

_ORACLE = {}


@functools.lru_cache(maxsize=None)
def _ring(n_nodes, n_replicas, link_depth=1):
    return scenarios.token_ring(n_nodes=n_nodes, n_replicas=n_replicas, launch_duration=T_KILL, drop_log2=2,
                                link_depth=link_depth)


def _oracle(oracle_mod, scn, order="fifo"):
    key = (id(scn), order)  # (the builders are cached: one object per scenario)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


def _oracle_cut(oracle_mod, scn, order, **kw):
    """one replica, cut at t_end / max_events"""
    key = (id(scn), order, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run(scn, mode=ORACLE_MODE[order], trace_cap=0, **kw)
    return _ORACLE[key]


def _same(tag, res, h, ores, oh):
    for f in FIELDS:
        assert np.array_equal(res[f], ores[f]), (tag, f, res[f][:6], ores[f][:6])
    assert np.array_equal(h, oh), tag


def _all_like(tag, res, h, o):
    """every replica equals the oracle's one run `o` (no send yet: replicas are alike)"""
    for f in FIELDS:
        assert (res[f] == o.result[f]).all(), (tag, f, res[f][:4], o.result[f])
    assert (h == o.hashes[None, :]).all(), tag


def _engine(engine_mod, scn, order, geo, prefix=True, sweep=True):
    e = engine_mod.Engine(0)
    e.load(scn, geometry=geo)
    e.set_tie_mode(order)
    if not prefix:
        e.set_prefix(False)
    if not sweep:
        e.set_sweep(False)
    return e


def _runs(e, runs=({},)):
    """reset, then the tw_run calls `runs`: results, hashes, what each run did with the prefix"""
    e.reset()
    did = []
    for kw in runs:
        e.run(**kw)
        did.append(e.prefix_stats()["last"])
    return e.results(), e.hashes(), did


def _snapshot_events(oracle_mod, scn, order):
    return int(_oracle_cut(oracle_mod, scn, order, replica=0, t_end=T0 - 1).result["events"])


# ------------------------------------------------------------- pilot and cache
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", [4, 40])
def test_pilot_then_cached_snapshot(engine_mod, oracle_mod, N, order, geo, R):
    scn = _ring(N, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        assert e.prefix_stats()["t0"] == T0
        for i, want in enumerate(["piloted", "applied", "applied"]):
            res, h, did = _runs(e)
            assert did == [want], (i, did)
            _same((N, order, geo, i), res, h, ores, oh)
            st = e.prefix_stats()
            assert st["t0"] == T0 and st["events"] == _snapshot_events(oracle_mod, scn, order)
            # at least the scalar block and main's and the nodes' thread records
            assert st["bytes"] >= 8 * 20 + 64 * (3 * N + 1)
    with _engine(engine_mod, scn, order, geo, prefix=False) as e:
        res0, h0, did = _runs(e)
        assert did == ["not_eligible"]
        _same(("off", N, order, geo), res0, h0, ores, oh)


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_link_depth(engine_mod, oracle_mod, order, geo, R):
    """link_depth 3: the pilot checks replica 0's send ordinals too"""
    scn = _ring(4, R, link_depth=3)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        for want in ("piloted", "applied"):
            res, h, did = _runs(e)
            assert did == [want]
            _same((order, geo, want), res, h, ores, oh)


# ------------------------------------------------------------ t_end around T0
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_t_end_around_t0(engine_mod, oracle_mod, order, geo, R):
    scn = _ring(4, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        # short of T0 - 1: not eligible; the run that goes on is not fresh
        res, h, did = _runs(e, ({"t_end": T0 - 2}, {}))
        assert did == ["not_eligible", "not_eligible"]
        _same((order, geo, "T0-2"), res, h, ores, oh)
        for t_end in (T0 - 1, T0):
            o = _oracle_cut(oracle_mod, scn, order, replica=0, t_end=t_end)
            for want in (("piloted" if t_end == T0 - 1 else "applied"), "applied"):
                res, h, did = _runs(e, ({"t_end": t_end},))
                assert did == [want], (t_end, did)
                _all_like((order, geo, t_end), res, h, o)
            e.run()  # ... and on to the end
            assert e.prefix_stats()["last"] == "not_eligible"
            _same((order, geo, t_end, "on"), e.results(), e.hashes(), ores, oh)


# --------------------------------------------------- max_events around the snapshot
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_max_events_around_the_snapshot(engine_mod, oracle_mod, order, geo, R):
    scn = _ring(4, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    n = _snapshot_events(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e, _engine(engine_mod, scn, order, geo, prefix=False) as e0:
        assert _runs(e)[2] == ["piloted"] and e.prefix_stats()["events"] == n
        for cap, want in ((n - 1, "not_eligible"), (n, "applied"), (n + 1, "applied")):
            res, h, did = _runs(e, ({"max_events": cap},))
            assert did == [want], (cap, did)
            assert (res["events"] == cap).all()
            res0, h0, _ = _runs(e0, ({"max_events": cap},))
            _same((order, geo, cap, "off"), res, h, res0, h0)
            for r in (0, 1, R - 1):  # (the event behind the snapshot may send: replicas differ)
                o = _oracle_cut(oracle_mod, scn, order, replica=r, max_events=cap)
                for f in FIELDS:
                    assert res[f][r] == o.result[f], (cap, r, f)
                assert (h[r] == o.hashes).all(), (cap, r)
            e.run()
            _same((order, geo, cap, "on"), e.results(), e.hashes(), ores, oh)


@pytest.mark.parametrize("order", ORDERS)
def test_pilot_at_the_event_cap_is_refused(engine_mod, oracle_mod, order):
    """the first fresh run's cap falls inside the prefix: its pilot is refused,
    and remembered as refused for the key"""
    scn = _ring(4, 301)
    ores, oh = _oracle(oracle_mod, scn, order)
    n = _snapshot_events(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, "dense") as e:
        res, h, did = _runs(e, ({"max_events": n - 2},))
        assert did == ["refused"]
        _all_like((order, "cap"), res, h, _oracle_cut(oracle_mod, scn, order, replica=0, max_events=n - 2))
        e.run()
        _same((order, "cap", "on"), e.results(), e.hashes(), ores, oh)
        res, h, did = _runs(e)
        assert did == ["refused"] and e.prefix_stats()["events"] == 0
        _same((order, "cap", "again"), res, h, ores, oh)
        e.set_tie_mode(order)  # drops what is cached for the key: the next fresh run pilots
        res, h, did = _runs(e)
        assert did == ["piloted"]
        _same((order, "cap", "piloted"), res, h, ores, oh)


# ------------------------------------------------------------- invalidation
@pytest.mark.parametrize("geo,R", GEOS)
def test_tie_mode_change_repilots(engine_mod, oracle_mod, geo, R):
    scn = _ring(4, R)
    with _engine(engine_mod, scn, "fifo", geo) as e:
        for order, want in (("fifo", "piloted"), ("fifo", "applied"), ("forkfirst", "piloted"),
                            ("forkfirst", "applied"), ("fifo", "piloted")):
            if want == "piloted":  # (the other steps keep the mode of the step before)
                e.set_tie_mode(order)
            res, h, did = _runs(e)
            assert did == [want], (order, did)
            _same((geo, order, want), res, h, *_oracle(oracle_mod, scn, order))


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_counter_base_repilots(engine_mod, oracle_mod, order, geo, R):
    scn = _ring(4, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e, _engine(engine_mod, scn, order, geo, prefix=False) as e0:
        assert _runs(e)[2] == ["piloted"]
        e.set_counter_base(1000, 77)
        e0.set_counter_base(1000, 77)
        res0, h0, _ = _runs(e0)
        for want in ("piloted", "applied"):
            res, h, did = _runs(e)
            assert did == [want]
            _same((order, geo, "base", want), res, h, res0, h0)
        e.set_counter_base(0, 1)
        res, h, did = _runs(e)
        assert did == ["piloted"]
        _same((order, geo, "base back"), res, h, ores, oh)


# ------------------------------------------------------------ with the sweeps
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_sweep_off_and_on_and_runs_in_pieces(engine_mod, oracle_mod, order, geo, R):
    scn = _ring(40, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    N = 40
    with _engine(engine_mod, scn, order, geo, sweep=False) as e:
        for want in ("piloted", "applied"):
            res, h, did = _runs(e)
            assert did == [want] and e.sweep_stats()["killers"] == 0
            _same((order, geo, "sweep off", want), res, h, ores, oh)
        e.set_sweep(True)
        res, h, did = _runs(e)
        assert did == ["applied"] and e.sweep_stats()["killers"] == R * (N + 1)
        _same((order, geo, "sweep on"), res, h, ores, oh)
        # in pieces across the sweep time: the first piece takes the prefix
        pieces = ({"t_end": sec(5)}, {"t_end": T_KILL - 1}, {"t_end": T_KILL - 1}, {"t_end": T_KILL}, {})
        res, h, did = _runs(e, pieces)
        assert did == ["applied"] + ["not_eligible"] * 4
        _same((order, geo, "pieces"), res, h, ores, oh)


# ------------------------------------------------------------------ not used
def _not_used(engine_mod, oracle_mod, scn, order, geo, trace=0):
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry=geo)
        if order != "fifo":
            e.set_tie_mode(order)
        if trace:
            e.set_trace(trace)
        for _ in range(2):
            res, h, did = _runs(e)
            assert did == ["not_eligible"], (scn.name, geo, order, did)
            assert e.prefix_stats()["events"] == 0 and e.prefix_stats()["bytes"] == 0
            _same((scn.name, geo, order), res, h, *_oracle(oracle_mod, scn, order))
        return e.prefix_stats()


@functools.lru_cache(maxsize=None)
def _ping_pong():
    return scenarios.ping_pong(n_replicas=70, round_trips=3)


@functools.lru_cache(maxsize=None)
def _socket_state():
    return scenarios.socket_state(n_replicas=70)


def test_not_used_ping_pong(engine_mod, oracle_mod):
    """70 replicas of ping-pong run a wavefront per replica (65,536 and more:
    the compact geometry); neither takes the prefix"""
    assert _not_used(engine_mod, oracle_mod, _ping_pong(), "fifo", None)["t0"] == sec(2)
    _not_used(engine_mod, oracle_mod, _ping_pong(), "fifo", "compact")


def test_not_used_main_regs(engine_mod, oracle_mod):
    """socket-state: main's registers differ by replica"""
    assert _socket_state().main_regs is not None
    assert _not_used(engine_mod, oracle_mod, _socket_state(), "fifo", "dense")["t0"] == sec(1)


def test_not_used_lifo_and_trace(engine_mod, oracle_mod):
    _not_used(engine_mod, oracle_mod, _ring(4, 70), "lifo", "dense")
    _not_used(engine_mod, oracle_mod, _ring(4, 70), "fifo", "dense", trace=64)


@pytest.mark.parametrize("geo", ["compact", "sparse", "wave", "lpb"])
def test_not_used_other_geometries(engine_mod, oracle_mod, geo):
    scn = _ring(4, 64)  # (lpb: a power-of-two replica count)
    _not_used(engine_mod, oracle_mod, scn, "fifo", geo)


def test_not_used_without_sends(engine_mod, oracle_mod):
    """an image that never sends would end inside its prefix: no prefix (tw_prefix_stats
    reports T0 = 0), and its kill wakes are still swept"""
    from test_gpu_sweep import prog

    scn = prog("stale", 12)
    assert _not_used(engine_mod, oracle_mod, scn, "fifo", "dense")["t0"] == 0
    with _engine(engine_mod, scn, "fifo", "dense") as e:
        _runs(e)
        assert e.sweep_stats()["killers"] == 12 * scn.n_replicas


# -------------------------------------------- other shapes of the same argument
@pytest.mark.parametrize("order", ORDERS)
def test_ping_pong_dense_takes_it(engine_mod, oracle_mod, order):
    """ping-pong under the dense geometry (no far runs): T0 = 2 s, the prefix is used"""
    scn = _ping_pong()
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, "dense") as e:
        for want in ("piloted", "applied"):
            res, h, did = _runs(e)
            assert did == [want] and e.prefix_stats()["t0"] == sec(2)
            _same(("ping-pong", order, want), res, h, ores, oh)


@functools.lru_cache(maxsize=None)
def _handler_sends_at_0(n_replicas=70):
    """tests/prefix_classify_main.cpp's image as a scenario: main forks `a` on
    node 0 and throws to it at once; a's handler sends, while a's only
    exception-free path to the handler sleeps 1 s.  T0 = 0: no prefix."""
    EXC = isa.EXC_USER0
    p = Program()
    K_MSG = p.kind("msg")
    rx = p.listener_set({"msg": "on_msg"})
    c = p.function("main")
    c.seti(0, 1).fork_("rx_main", node_reg=0)
    c.seti(0, 0).fork("a", ref=1, node_reg=0)
    c.throw_to(1, EXC, 0).end()
    c = p.function("a")
    c.catch_(1 << EXC, "handler")
    c.wait(for_(sec(1)))
    c.uncatch()
    c = p.function("handler")
    c.link(1, 0).send(1, K_MSG, 0)
    c.end()
    c = p.function("rx_main")
    c.listen(rx)
    c.end()
    c = p.function("on_msg")
    c.trace(1, 0)
    c.end()
    img = p.finalize()
    topo = Topology.from_out_lists(3, [[1], [], []])
    table = scenarios.draw_table(1, n_replicas, [0], np.array([ms(1)]), np.array([ms(5)]), drop_log2=2)
    return Scenario(name="handler_sends_at_0", image=img, topo=topo, n_replicas=n_replicas,
                    main_pc=img.pc_of("main"), main_node=2, link_table=table, max_slots=16, queue_capacity=64,
                    run_capacity=16, near_horizon_us=sec(10))


@pytest.mark.parametrize("order", ORDERS)
def test_handler_sends_at_t0(engine_mod, oracle_mod, order):
    scn = _handler_sends_at_0()
    ores, oh = _oracle(oracle_mod, scn, order)
    assert (ores["delivered"] + ores["dropped"] >= 1).all()  # the handler sent
    st = _not_used(engine_mod, oracle_mod, scn, order, "narrow")
    assert st["t0"] == 0
