"""What a tw_load leaves of the load before it.

One context, loads in sequence: batched LP with tracing on, then a replica
load of another scenario, then batched LP again.  After each load the context
must compute what a fresh context computes and say what a fresh context says:
the trace off, the sweeps, the prefix and the tie order back at their
defaults.  What outlives a load by design is pinned too: the counter bases
(tw_set_counter_base) and the last run's sweep counts.

A refused descriptor or argument keeps the previous load runnable; a load
refused behind that point (two-phase windows that would need a third phase, an
image too large for LDS) leaves the context unloaded (the state error) and a
later load works.  Every refusal here is a host-side status.

Shapes: the token ring of test_gpu_prefix.py (4 nodes, 70 replicas, dense) and
a hotspot of 8 senders over 8 replicas for the batched mode."""
import functools

import pytest

from timewarp import isa, scenarios
from timewarp.program import Program
import progs
from test_gpu_prefix import FIELDS, _all_like, _oracle, _ring, _same
from progs import single

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

ERR_INVALID, ERR_STATE = -1, -5
LDS_LIMIT = 160 * 1024


@functools.lru_cache(maxsize=None)
def _spot(n_replicas=8):
    return scenarios.hotspot(n_senders=8, n_replicas=n_replicas, msg_num=10)


def _code(call):
    with pytest.raises(Exception) as ei:
        call()
    return getattr(ei.value, "code", None)


def _run_same(tag, e, oracle_mod, scn):
    e.reset()
    st = e.run()
    _same(tag, e.results(), e.hashes(), *_oracle(oracle_mod, scn))
    return st


def _says(e):
    px = e.prefix_stats()
    del px["apply_ms"]
    return e.sweep_stats(), px, e.prefix_clean_stats()


def test_lpb_then_replica_then_lpb(engine_mod, oracle_mod):
    spot, ring = _spot(), _ring(4, 70)
    with engine_mod.Engine(0) as e, engine_mod.Engine(0) as fresh:
        e.load(spot, geometry="lpb")
        e.set_trace(256)
        _run_same("lpb traced", e, oracle_mod, spot)
        assert e.lpb_windows()[0] > 0 and e.lpb_batch()[0] == 0
        assert e.trace(0)[1] > 0

        e.load(ring, geometry="dense")
        fresh.load(ring, geometry="dense")
        assert e.geometry() == "dense"
        assert _says(e) == _says(fresh)
        # the trace is off: a replica context with tracing off answers the state error
        assert _code(lambda: e.measure(1, 2)) == ERR_STATE
        assert e.trace(0)[0].size == 0
        assert _code(e.lpb_windows) == ERR_STATE and _code(e.lpb_batch) == ERR_STATE
        for i, want in enumerate(["piloted", "applied"]):
            _run_same(("dense", i), e, oracle_mod, ring)
            _run_same(("fresh", i), fresh, oracle_mod, ring)
            says = _says(e)
            print("dense", i, says)
            assert says == _says(fresh)
            assert says[1]["last"] == want and says[0]["killers"] > 0

        e.load(spot, geometry="lpb")
        assert e.geometry() == "lpb"
        assert _code(lambda: e.measure(1, 2)) == ERR_INVALID  # (batched LP, tracing off)
        _run_same("lpb again", e, oracle_mod, spot)
        assert e.lpb_windows()[0] > 0 and e.trace(0)[1] == 0


def test_load_restores_the_switches(engine_mod, oracle_mod):
    ring = _ring(4, 70)
    with engine_mod.Engine(0) as e:
        e.load(ring, geometry="dense")
        e.set_sweep(False).set_prefix(False).set_tie_mode("forkfirst")
        e.reset().run()
        assert e.prefix_stats()["last"] == "not_eligible" and e.sweep_stats()["killers"] == 0
        e.load(ring, geometry="dense")
        _run_same("defaults", e, oracle_mod, ring)  # (the fifo oracle)
        assert e.prefix_stats()["last"] == "piloted" and e.sweep_stats()["killers"] > 0
        # (the ring's results are the same under both orders: a program whose results differ)
        scn = progs.random_program(3)
        fifo, ff = (oracle_mod.run(scn, replica=0, mode=m, t_end=3000) for m in (0, 5))
        assert any(fifo.result[f] != ff.result[f] for f in FIELDS) or (fifo.hashes != ff.hashes).any()
        e.load(scn, geometry="dense").set_tie_mode("forkfirst").reset().run(3000)
        _all_like("forkfirst", e.results(), e.hashes(), ff)
        e.load(scn, geometry="dense").run(3000)
        _all_like("fifo again", e.results(), e.hashes(), fifo)


def test_what_outlives_a_load(engine_mod, oracle_mod):
    ring = _ring(4, 70)
    with engine_mod.Engine(0) as e:
        e.load(ring, geometry="dense")
        _run_same("first", e, oracle_mod, ring)
        sw = e.sweep_stats()
        assert sw["killers"] > 0
        # the counter bases are the context's, not the load's
        e.set_counter_base(0xFFFFFFFF - 50, 1)
        e.load(ring, geometry="dense")
        # ... and so are the last run's counts, until the next run
        assert e.sweep_stats() == sw and e.prefix_stats()["last"] == "piloted"
        assert e.prefix_stats()["events"] == 0 and e.prefix_clean_stats()["claimed_slots"] == 0
        e.run()
        assert (e.results()["status"] == isa.REP_ERR_COUNTER).all()
        e.set_counter_base(0, 1)
        e.load(ring, geometry="dense")
        _run_same("base back", e, oracle_mod, ring)
        # the last batched run's windows and ticks, likewise
        spot = _spot()
        e.load(spot, geometry="lpb")
        _run_same("lpb", e, oracle_mod, spot)
        w = e.lpb_windows()
        assert w[0] > 0
        e.load(spot, geometry="lpb")
        assert e.lpb_windows() == w


def test_refused_descriptor_keeps_the_load(engine_mod, oracle_mod):
    spot = _spot()
    with engine_mod.Engine(0) as e:
        e.load(spot, geometry="lpb")
        _run_same("before", e, oracle_mod, spot)
        # batched LP takes a power-of-two replica count
        assert _code(lambda: e.load(_spot(6), geometry="lpb")) == ERR_INVALID
        assert _code(lambda: e.load_lpb(spot, lookahead_us=0)) == ERR_INVALID
        assert e.scn is spot  # (the wrapper records a scenario only behind a load that succeeded)
        assert e.geometry() == "lpb"
        _run_same("after", e, oracle_mod, spot)


def _short_link_out_of_phase1():
    """test_gpu_lpb.py's test_lpb_rejects_short_link_out_of_phase1"""
    scn = scenarios.gossip(n_nodes=64, fanout=2)
    lt = scn.link_table.copy()
    l_ab = int(scn.topo.out_off[0])
    l_bc = int(scn.topo.out_off[int(scn.topo.dst[l_ab])])
    lt[l_ab] = 0
    lt[l_bc] = 0
    scn.link_table = lt
    return scn


def _too_large_for_lds():
    p = Program()
    c = p.function("main")
    for _ in range(LDS_LIMIT // 16 + 8):
        c._e(isa.OP_NOP)
    c.end()
    return single(p, "nops", n_replicas=70)


@pytest.mark.parametrize("refused", ["two_phase", "lds"])
def test_refusal_behind_the_unload(engine_mod, oracle_mod, refused):
    ring, spot = _ring(4, 70), _spot()
    with engine_mod.Engine(0) as e:
        e.load(ring, geometry="dense")
        _run_same("before", e, oracle_mod, ring)
        if refused == "two_phase":
            bad = _short_link_out_of_phase1()
            assert _code(lambda: e.load_lpb(bad, lookahead_us=1000)) == ERR_INVALID
        else:
            bad = _too_large_for_lds()
            assert 16 * bad.desc().n_insns > LDS_LIMIT
            assert _code(lambda: e.load(bad, geometry="dense")) == ERR_INVALID
        for call in (e.reset, e.run, e.geometry, e.sweep_stats, e.prefix_stats):
            assert _code(call) == ERR_STATE, call
        e.load(spot, geometry="lpb")
        _run_same("lpb after", e, oracle_mod, spot)
        e.load(ring, geometry="dense")
        _run_same("dense after", e, oracle_mod, ring)
