"""Live delays on the GPU (tw_set_live_delays): a per-replica StdGen stepped at
each send, against `oracle.run(scn, replica=r, mode=m, live_seed=seed_base + r)`
field by field and node hash by node hash (integer outputs, no tolerances).

  1  config 1 native: the golden file's run without a table and without the oracle
  2  the seed batch: 300 rings, every replica its own generator; live_stats
  3  net soup made live: kinds over {0, 1, 2}, five ranges, lanes that never draw
  4  runs cut at a time and at an event count, continued; reset and re-run
  5  the send-free prefix and the sweeps, on and off
  6  two shards seed by the replica's index in the whole batch
  7  the tie audit re-seeds every probe run
  8  refusals, and off again

What the inputs reach is guarded on the CPU by tests/test_live_oracle.py; the
inputs and references are tests/livesoup.py's.  Every failure names the
replica and its generator's seed."""
import copy
import functools
import json
import os

import numpy as np
import pytest

import livesoup
from livesoup import LIVE_SEEDS, SEED_BASE, TABLE_SEED, live_ring, live_soup, recorded, ref, same
from netsoup import GPU_REPLICAS
from timewarp import isa, scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.measures import trace_tuples

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "token_ring_c1.json")))
RING = ("ring", GPU_REPLICAS)
ERR_INVALID, ERR_STATE = -1, -5


def _live_engine(engine_mod, scn, seed_base=SEED_BASE, geometry=None, **kw):
    e = engine_mod.Engine(**kw)
    e.load(scn, geometry=geometry)
    e.set_live_delays(scn, seed_base=seed_base)
    return e


# ------------------------------------------------------------ 1. config 1, native
@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", ["wave", "narrow"])
def test_config1_native(engine_mod, geo):
    """BASELINE config 1 -- one ring under mkStdGen 0, the draws in send order --
    from the engine alone: no table, no oracle."""
    scn = scenarios.token_ring(16, 1, launch_duration=20_000_000, live=True)
    assert scn.link_table is None
    with engine_mod.Engine() as e:
        e.load(scn, geometry=geo)
        assert e.geometry() == geo
        e.set_trace(64).set_live_delays(scn, seed_base=0).reset()
        e.run()
        res, h = e.results(), e.hashes()
        recs, n = e.trace(0)
        draws = e.live_stats()
    for f in RESULT_FIELDS:
        assert int(res[f][0]) == GOLD["result"][f], (geo, f, "seed 0, replica 0", int(res[f][0]), GOLD["result"][f])
    assert [f"{int(x):016x}" for x in h[0]] == GOLD["hashes"], (geo, "seed 0, replica 0: hashes")
    assert n == len(GOLD["traces"]) and [list(t) for t in trace_tuples(recs)] == GOLD["traces"], (geo, "TRACE list")
    # one draw per token sent: the recorded table's ring-link entries
    tab = np.array(GOLD["recorded_table"], dtype=np.uint32)
    assert draws == int((tab[scn.live_kind == 2] != 0).sum()), (geo, draws)


# ------------------------------------------------------------------ 2. seed batch
@functools.lru_cache(maxsize=None)
def _ring_draws():
    scn = live_ring(GPU_REPLICAS)
    return sum(livesoup.draws_of(scn, recorded(scn, r, SEED_BASE + r)[1]) for r in range(GPU_REPLICAS))


def test_seed_batch(engine_mod, oracle_mod):
    """300 rings (a full dense workgroup and a 44-lane tail), replica r under
    mkStdGen(7 + r), under every replica geometry."""
    scn = live_ring(GPU_REPLICAS)
    ores, oh = ref(RING)
    with _live_engine(engine_mod, scn) as e:
        st = e.run()
        same(scn, e.results(), e.hashes(), ores, oh, "seed batch")
        assert e.live_stats() == _ring_draws(), (e.live_stats(), _ring_draws(), f"seed_base {SEED_BASE}")
        assert st.events == int(ores["events"].sum())
        e.reset()                    # re-seeded: the same batch again
        e.run()
        same(scn, e.results(), e.hashes(), ores, oh, "seed batch, after reset")
        assert e.live_stats() == _ring_draws()
    assert len({x.tobytes() for x in oh}) > GPU_REPLICAS // 2     # (the generators differ: so do the rings' traces)


# ----------------------------------------------------------------- 3. net soup, live
@pytest.mark.parametrize("seed", LIVE_SEEDS)
def test_soup_canonical(engine_mod, oracle_mod, seed):
    scn = live_soup(seed)
    ores, oh = ref(("soup", seed, "regs"))
    with _live_engine(engine_mod, scn) as e:
        e.run()
        same(scn, e.results(), e.hashes(), ores, oh, "canonical")


@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", ["dense", "compact"])
@pytest.mark.parametrize("order,mode", [("lifo", 2), ("forkfirst", 5)])
@pytest.mark.parametrize("seed", LIVE_SEEDS)
def test_soup_tie_orders(engine_mod, oracle_mod, seed, order, mode, geo):
    scn = live_soup(seed)
    ores, oh = ref(("soup", seed, "regs"), mode=mode)
    with _live_engine(engine_mod, scn, geometry=geo) as e:
        assert e.geometry() == geo
        e.set_tie_mode(order).reset()
        e.run()
        same(scn, e.results(), e.hashes(), ores, oh, f"{order}, {geo}", mode=mode)


@pytest.mark.one_geometry
@pytest.mark.parametrize("seed", LIVE_SEEDS)
def test_soup_pqueue_wave(engine_mod, oracle_mod, seed):
    scn = copy.copy(live_soup(seed))
    scn.queue_capacity = 8192            # (covers every pending event: tw_set_tie_mode)
    ores, oh = livesoup.oracle_batch(scn, mode=1)
    with _live_engine(engine_mod, scn, geometry="wave") as e:
        e.set_tie_mode("pqueue").reset()
        e.run()
        same(scn, e.results(), e.hashes(), ores, oh, "pqueue, wave", mode=1)


# -------------------------------------------------------------------------- 4. cuts
MSG_TERMS = (isa.KIND_RECV >> 16, isa.KIND_DROP >> 16, isa.KIND_UNDELIV >> 16)


@functools.lru_cache(maxsize=None)
def _cut_ref(name):
    """T1 and E0 from the oracle's term log, as test_gpu_netsoup.py derives
    them: T1 is the median over the replicas of the time of the message term
    a third of the way through the replica's message terms; E0 is half the
    lower quartile of the replicas' event totals.  Returns them with the share
    of replicas that still have a draw to come at each cut."""
    scn = livesoup.scenario(name)
    ores, _ = ref(name)
    thirds, total = [], np.zeros(scn.n_replicas, np.int64)
    for r in range(scn.n_replicas):
        _res, sends, _rec, terms = recorded(scn, r, SEED_BASE + r, term_cap=1 << 14)
        total[r] = livesoup.draws_of(scn, sends)
        times = sorted(t for t, _n, kind, _v in terms if kind >> 16 in MSG_TERMS)
        if times:
            thirds.append(times[len(times) // 3])
    t1 = int(np.median(thirds))
    ev0 = max(1, int(np.percentile(ores["events"].astype(np.int64), 25)) // 2)
    at_t1 = np.array([livesoup.draws_of(scn, recorded(scn, r, SEED_BASE + r, t_end=t1)[1])
                      for r in range(scn.n_replicas)])
    at_e0 = np.array([livesoup.draws_of(scn, recorded(scn, r, SEED_BASE + r, max_events=ev0)[1])
                      for r in range(scn.n_replicas)])
    return t1, ev0, float((at_t1 < total).mean()), float((at_e0 < total).mean())


@pytest.mark.parametrize("name", [("soup", LIVE_SEEDS[1], "regs"), RING], ids=["soup", "ring"])
def test_cuts_and_rerun(engine_mod, oracle_mod, name):
    scn = livesoup.scenario(name)
    ores, oh = ref(name)
    t1, ev0, to_come_t1, to_come_e0 = _cut_ref(name)
    print(f"{scn.name}: T1 {t1} us, E0 {ev0}; a draw still to come at T1 {to_come_t1:.2f}, at E0 {to_come_e0:.2f}")
    # (the oracle's figures, before the engine runs: the generators are mid-sequence at the cuts)
    assert to_come_t1 >= 0.5 and to_come_e0 >= 0.5, (name, t1, ev0, to_come_t1, to_come_e0)
    with _live_engine(engine_mod, scn) as e:
        e.run(t_end=t1)
        assert (e.results()["status"] == isa.REP_RUNNING).mean() >= 0.5
        e.run()
        same(scn, e.results(), e.hashes(), ores, oh, f"cut at t_end={t1}, continued")
        e.reset()
        e.run(max_events=ev0)
        res = e.results()
        assert (res["status"] == isa.REP_RUNNING).mean() >= 0.5 and (res["events"] <= ores["events"]).all()
        e.run()
        same(scn, e.results(), e.hashes(), ores, oh, f"cut at max_events={ev0}, continued")
        e.reset()
        st = e.run()
        same(scn, e.results(), e.hashes(), ores, oh, "reset, whole")
        assert st.events == int(ores["events"].sum())


# ------------------------------------------------------------- 5. prefix and sweep
@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", ["dense", "narrow", "half"])
@pytest.mark.parametrize("name", [RING, ("soup", TABLE_SEED, "table")], ids=["ring", "table_soup"])
def test_prefix_and_sweep(engine_mod, oracle_mod, name, geo):
    """The prefix ends before the first send, so no generator has moved when
    its snapshot is taken or applied; the sweeps kill and never send."""
    scn = livesoup.scenario(name)
    assert scn.main_regs is None
    ores, oh = ref(name)
    with _live_engine(engine_mod, scn, geometry=geo) as e:
        assert e.geometry() == geo
        t0 = e.prefix_stats()["t0"]
        assert t0 >= 1, (name, t0)
        for on in (True, False):
            e.set_prefix(on)
            used = []
            for i in range(3):
                e.reset()
                e.run()
                used.append(e.prefix_stats()["last"])
                same(scn, e.results(), e.hashes(), ores, oh, f"prefix {on}, pair {i} ({used[-1]}), {geo}")
            print(name, geo, "prefix", on, used)
            if on:
                assert used[0] in ("piloted", "applied") and used[1:] == ["applied", "applied"], (name, geo, used)
            else:
                assert used == ["not_eligible"] * 3, (name, geo, used)
        e.set_prefix(True)
        swept = []
        for on in (True, False):
            e.set_sweep(on)
            for i in range(3):
                e.reset()
                e.run()
                sw = e.sweep_stats()
                swept.append(sw["victims"])
                same(scn, e.results(), e.hashes(), ores, oh, f"sweep {on}, pair {i}, {geo}")
        assert swept[3:] == [0, 0, 0], (name, geo, swept)
        if name == RING:     # (its kill_pair at launch_duration is what the sweeps serve; the soups have none)
            assert min(swept[:3]) > 0, (name, geo, swept)


# --------------------------------------------------------------------- 6. two shards
@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", [None, "dense"])
def test_two_shards_seed_by_global_index(engine_mod, oracle_mod, geo):
    import oracle

    scn = live_soup(LIVE_SEEDS[0])
    ores, oh = ref(("soup", LIVE_SEEDS[0], "regs"))
    # replica 150 is the second shard's first: seeded by its index within the
    # shard it would draw from SEED_BASE + 0 -- which the oracle tells apart
    local = oracle.run(live_ring(GPU_REPLICAS), replica=150, live_seed=SEED_BASE)
    rres, rh = ref(RING)
    assert any(local.result[f] != rres[f][150] for f in RESULT_FIELDS) or not np.array_equal(local.hashes, rh[150])
    for s, o_res, o_h in ((scn, ores, oh), (live_ring(GPU_REPLICAS), rres, rh)):
        with _live_engine(engine_mod, s, geometry=geo) as one:
            one.run()
            r1, h1 = one.results(), one.hashes()
        with _live_engine(engine_mod, s, geometry=geo, devices=[0, 0]) as two:
            assert two.info()[0] == 2
            two.run()
            r2, h2 = two.results(), two.hashes()
            draws2 = two.live_stats()
        same(s, r2, h2, o_res, o_h, f"two shards, {geo}")
        same(s, r1, h1, o_res, o_h, f"one device, {geo}")
        for f in RESULT_FIELDS:
            assert np.array_equal(r1[f], r2[f]), (f, "one device against two shards")
        assert np.array_equal(h1, h2)
        if s is not scn:
            assert draws2 == _ring_draws(), (draws2, "live_stats summed over the shards")


# ---------------------------------------------------------------------- 7. tie audit
@pytest.mark.one_geometry
def test_tie_audit_reseeds_every_probe(engine_mod, oracle_mod):
    seed = LIVE_SEEDS[0]
    scn = live_soup(seed)
    name = ("soup", seed, "regs")
    (r0, h0), (r2, h2), (r3, h3) = ref(name), ref(name, mode=2), ref(name, mode=3)

    def differs(ra, ha):
        d = (ha != h0).any(axis=1)
        for f in RESULT_FIELDS:
            d |= ra[f] != r0[f]
        return d

    want = 1 | (differs(r2, h2).astype(np.uint32) << 1) | (differs(r3, h3).astype(np.uint32) << 2)
    with _live_engine(engine_mod, scn) as e:
        e.tie_audit(probes=2)
        res, h = e.results(), e.hashes()
    same(scn, res, h, r0, h0, "tie audit: the canonical run stays loaded")
    bad = np.flatnonzero(res["tie_flags"] != want)
    assert bad.size == 0, (f"seed {seed}, replica {bad[0]}, live seed {SEED_BASE + bad[0]}: tie_flags "
                           f"{res['tie_flags'][bad[0]]} != oracle {want[bad[0]]} ({bad.size} replicas)")


# ----------------------------------------------------------------------- 8. refusals
@pytest.mark.one_geometry
def test_refusals_and_off_again(engine_mod, oracle_mod):
    def code(fn):
        with pytest.raises(engine_mod.EngineError) as ei:
            fn()
        return ei.value.code

    ring = scenarios.token_ring(16, 64, launch_duration=5_000_000)
    with engine_mod.Engine() as e:                       # before a load
        assert code(lambda: e.set_live_delays(ring)) == ERR_STATE
        assert code(e.live_stats) == ERR_STATE
        e.load_lpb(ring)                                 # batched logical processes
        assert code(lambda: e.set_live_delays(ring)) == ERR_INVALID
        assert code(lambda: e.set_live_delays(None)) == ERR_INVALID
    small = scenarios.gossip(n_nodes=64, fanout=2)
    lp = engine_mod.LPEngine(engine_mod.lp_scenario(small), 0, small.n_nodes, int(small.meta["lookahead_us"]))
    try:
        k = np.zeros(small.topo.n_links, np.uint32)
        assert code(lambda: lp.set_live_delays((k, k.astype(np.int64), k.astype(np.int64)))) == ERR_INVALID
    finally:
        lp.close()
    # a bad spec leaves the context as it was; off again reproduces the table run
    tres, th = oracle_mod.run_batch(ring)
    with engine_mod.Engine() as e:
        e.load(ring)
        bad_kind = ring.live_kind.copy()
        bad_kind[0] = 3
        assert code(lambda: e.set_live_delays((bad_kind, ring.live_lo, ring.live_hi))) == ERR_INVALID
        assert code(lambda: e.set_live_delays((ring.live_kind, ring.live_lo, ring.live_hi + (1 << 31)))) == ERR_INVALID
        assert code(lambda: e.set_live_delays((ring.live_kind, ring.live_lo, ring.live_lo + 2147483))) == ERR_INVALID
        assert e.live_stats() == 0
        e.run()
        for f in RESULT_FIELDS:
            assert np.array_equal(e.results()[f], tres[f]), (f, "after refused specs: the table run")
        e.set_live_delays(ring, seed_base=3).reset()
        e.run()
        live_res = e.results()
        assert e.live_stats() > 0
        assert any(not np.array_equal(live_res[f], tres[f]) for f in RESULT_FIELDS) or \
            not np.array_equal(e.hashes(), th)
        e.set_live_delays(None).reset()
        e.run()
        assert e.live_stats() == 0
        for f in RESULT_FIELDS:
            assert np.array_equal(e.results()[f], tres[f]), (f, "live delays off again: the table run")
        assert np.array_equal(e.hashes(), th)
