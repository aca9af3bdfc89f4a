"""Random networked programs with divergent replicas (tests/netsoup.py), the
engine against the oracle: every RESULT_FIELD and every node hash bit-exact
(integer outputs, no tolerances).

  a  canonical order under every replica geometry, 300 replicas a seed
  b  runs cut at a time and at an event count, continued, then reset and re-run
  c  TW_TIE_LIFO / TW_TIE_FORKFIRST under five geometries, TW_TIE_PQUEUE under wave
  d  the send-free prefix and its refusals on images nobody wrote by hand
  e  TRACE records, record for record
  g  fused instruction pairs against the two-instruction form

(f, the profile="lp" soup under tw_lpb_load, is not here: see DESIGN.md, net soup.)

What the seeds cover is guarded on the CPU by tests/test_netsoup_oracle.py.
Every failure names seed, replica and field and the command that replays the
replica through the oracle without a GPU."""
import functools

import numpy as np
import pytest

import netsoup
import progs
from netsoup import GPU_REPLICAS, SEEDS, net_soup, reducer_command
from timewarp import isa
from timewarp.abi import RESULT_FIELDS
from timewarp.measures import trace_tuples

pytestmark = pytest.mark.gpu

QUARTER = SEEDS[::4]
TIE = {"lifo": 2, "forkfirst": 5, "pqueue": 1}      # oracle modes


# ------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def _scn(seed, diverge="regs"):
    return net_soup(seed, GPU_REPLICAS, diverge=diverge)


@functools.lru_cache(maxsize=None)
def _ref(seed, diverge="regs", mode=0):
    """The oracle's whole run of a seed's batch (computed once, never written to)."""
    import oracle

    res, h = oracle.run_batch(_scn(seed, diverge), mode=mode, threads=8)
    res.setflags(write=False)
    h.setflags(write=False)
    return res, h


def _same(scn, res, h, ores, oh, what, mode=0, only=None):
    """Every field and node hash of every replica (of `only`, a mask) equal."""
    rows = np.arange(scn.n_replicas) if only is None else np.flatnonzero(only)
    for f in RESULT_FIELDS:
        bad = rows[res[f][rows] != ores[f][rows]]
        assert bad.size == 0, (f"{scn.name} [{what}]: seed {scn.meta['seed']}, replica {bad[0]}, field {f}: "
                               f"gpu {res[f][bad[0]]} != oracle {ores[f][bad[0]]} ({bad.size} replicas differ); "
                               f"{reducer_command(scn, int(bad[0]), mode)}")
    bad = rows[(h[rows] != oh[rows]).any(axis=1)]
    if bad.size:
        nodes = np.flatnonzero(h[bad[0]] != oh[bad[0]]).tolist()
        raise AssertionError(f"{scn.name} [{what}]: seed {scn.meta['seed']}, replica {bad[0]}, field hashes "
                             f"(nodes {nodes}; {bad.size} replicas differ); {reducer_command(scn, int(bad[0]), mode)}")


# ------------------------------------------------- a. canonical, every geometry
@pytest.mark.parametrize("seed", SEEDS)
def test_canonical(engine_mod, oracle_mod, seed):
    scn = _scn(seed)
    ores, oh = _ref(seed)
    st, res, h = engine_mod.run_scenario(scn)
    _same(scn, res, h, ores, oh, "canonical")
    assert st.events == int(ores["events"].sum()), (seed, "stats.events")
    assert st.replicas_error == int((ores["status"] >= isa.REP_ERR_SLOTS).sum()), (seed, "stats.replicas_error")


def test_owned_listener_two_owners(engine_mod, oracle_mod):
    """progs.owned_listener_two_owners, what seeds 7 and 12 reduced to: a dying
    thread that once owned its node's listener releases nothing when another
    thread has bound the node since; the message after both deaths finds the
    port closed, under every geometry."""
    scn, want = progs.owned_listener_two_owners()
    o = oracle_mod.run(scn)
    st, res, h = engine_mod.run_scenario(scn)
    for f in RESULT_FIELDS:
        assert res[f][0] == o.result[f], (f, res[f][0], o.result[f])
    assert np.array_equal(h[0], o.hashes)
    assert res["undeliverable"][0] == want["undeliverable"] and res["delivered"][0] == want["delivered"]


# ---------------------------------------------------------------------- b. cuts
MSG_TERMS = (isa.KIND_RECV >> 16, isa.KIND_DROP >> 16, isa.KIND_UNDELIV >> 16)


@functools.lru_cache(maxsize=None)
def _cut_ref(seed):
    """T1 and E from the traffic itself, not from the run's end (a daemon's
    closing wait of up to 3 ms outlasts the messages by far).  A replica's
    message terms (RECV, DROP, UNDELIV) are sorted by time; T1 is the median
    over the replicas of the time of the term a third of the way through, so
    most replicas are cut with messages still to come.  E lies halfway
    between a replica's event count at the T1 cut and its final one (median
    over the replicas), so the event cap bites after the time cut, not before;
    the replicas' totals differ up to fourfold (1-4 rounds), so one E is
    mid-run for about half of them.  E0, for an event cut on a fresh reset, is
    half the lower quartile of the totals: it stops three replicas in four.
    Returns T1, E, E0, the oracle's per-replica state at the T1 cut, and the
    shares of replicas that are mid-traffic at T1, stopped by E between T1 and
    their end, and stopped by E0 with messages still to come."""
    import oracle

    scn = _scn(seed)
    ores, _ = _ref(seed)
    thirds = []
    for r in range(scn.n_replicas):
        o = oracle.run(scn, replica=r, term_cap=1 << 13)
        assert len(o.terms) < 1 << 13
        times = sorted(t for t, _n, kind, _v in o.terms if kind >> 16 in MSG_TERMS)
        if times:
            thirds.append(times[len(times) // 3])
    t1 = int(np.median(thirds))
    cut = [oracle.run(scn, replica=r, t_end=t1) for r in range(scn.n_replicas)]
    msgs = ores["delivered"] + ores["dropped"] + ores["undeliverable"]
    cut_msgs = np.array([o.result["delivered"] + o.result["dropped"] + o.result["undeliverable"] for o in cut])
    cut_ev = np.array([o.result["events"] for o in cut], np.int64)
    tot_ev = ores["events"].astype(np.int64)
    ev = int(np.median((cut_ev + tot_ev) // 2))
    in_flight = float((cut_msgs < msgs).mean())          # replicas with messages still to come at T1
    capped = float(((cut_ev < ev) & (ev < tot_ev)).mean())   # replicas the event cap stops after T1, before their end
    ev0 = max(1, int(np.percentile(tot_ev, 25)) // 2)
    at0 = [oracle.run(scn, replica=r, max_events=ev0).result for r in range(scn.n_replicas)]
    msgs0 = np.array([o["delivered"] + o["dropped"] + o["undeliverable"] for o in at0])
    capped0 = float(((tot_ev > ev0) & (msgs0 < msgs)).mean())
    return t1, ev, ev0, cut, in_flight, capped, capped0


@pytest.mark.parametrize("seed", QUARTER)
def test_cuts_and_rerun(engine_mod, oracle_mod, seed):
    scn = _scn(seed)
    ores, oh = _ref(seed)
    t1, ev, ev0, cut, in_flight, capped, capped0 = _cut_ref(seed)
    print(f"seed {seed}: T1 {t1} us, E {ev}, E0 {ev0}; mid-traffic at T1 {in_flight:.2f}, stopped by E {capped:.2f}, "
          f"by E0 with messages to come {capped0:.2f}")
    # the cuts fall mid-traffic (the oracle's figures, not the engine's): most
    # replicas at T1 and at E0, and a third at least at E after T1
    assert in_flight > 0.5 and capped0 > 0.5 and capped > 1 / 3, (seed, t1, ev, ev0, in_flight, capped, capped0)
    with engine_mod.Engine() as e:
        e.load(scn).reset()
        e.run(t_end=t1)
        res, h = e.results(), e.hashes()
        for r, o in enumerate(cut):
            for f in RESULT_FIELDS:
                assert res[f][r] == o.result[f], (f"seed {seed}, replica {r}, field {f} at t_end={t1}: gpu "
                                                  f"{res[f][r]} != oracle {o.result[f]}; {reducer_command(scn, r)}")
            assert np.array_equal(h[r], o.hashes), (f"seed {seed}, replica {r}, field hashes at t_end={t1}; "
                                                    f"{reducer_command(scn, r)}")
        e.run(max_events=ev)
        res = e.results()
        running = res["status"] == isa.REP_RUNNING
        assert running.mean() > 1 / 3, (seed, "the event cap stopped too few replicas", running.mean())
        assert (res["events"][running] >= ev).all(), (seed, "event cap: a running replica below it")
        assert (res["events"][running] < ores["events"][running]).all(), (seed, "event cap: running at its end")
        assert (res["events"] <= ores["events"]).all(), (seed, "event cap: more events than the whole run")
        e.run()
        _same(scn, e.results(), e.hashes(), ores, oh, "in pieces")
        e.reset()                                   # the event cut first, from a fresh start
        e.run(max_events=ev0)
        res = e.results()
        running = res["status"] == isa.REP_RUNNING
        assert running.mean() > 0.5, (seed, "E0 stopped too few replicas", running.mean())
        assert (res["events"][running] >= ev0).all() and (res["events"] <= ores["events"]).all(), (seed, "E0")
        assert (res["events"][running] < ores["events"][running]).all(), (seed, "E0: running at its end")
        e.run()
        _same(scn, e.results(), e.hashes(), ores, oh, "event cut first")
        e.reset()
        st = e.run()
        _same(scn, e.results(), e.hashes(), ores, oh, "reset, whole")
        assert st.events == int(ores["events"].sum())


# ---------------------------------------------------------------- c. tie orders
@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", ["dense", "narrow", "sparse", "compact", "half"])
@pytest.mark.parametrize("order", ["lifo", "forkfirst"])
@pytest.mark.parametrize("seed", QUARTER)
def test_tie_orders(engine_mod, oracle_mod, seed, order, geo):
    scn = _scn(seed)
    ores, oh = _ref(seed, mode=TIE[order])
    with engine_mod.Engine() as e:
        e.load(scn, geometry=geo)
        # (sparse, and sparse alone, falls back to dense when the image does not fit its LDS)
        assert e.geometry() == geo or (geo == "sparse" and e.geometry() == "dense")
        e.set_tie_mode(order).reset()
        e.run()
        _same(scn, e.results(), e.hashes(), ores, oh, f"{order}, {geo}", mode=TIE[order])


@pytest.mark.one_geometry
@pytest.mark.parametrize("seed", [1, 6, 13])
def test_pqueue_order_wave(engine_mod, oracle_mod, seed):
    """TimedT's own equal-time order (wave geometry) against the oracle's
    pqueue transcription; queue_capacity covers every pending event."""
    import copy

    scn = copy.copy(_scn(seed))
    scn.queue_capacity = 8192
    ores, oh = _ref(seed, mode=TIE["pqueue"])
    with engine_mod.Engine() as e:
        e.load(scn, geometry="wave")
        e.set_tie_mode("pqueue").reset()
        e.run()
        _same(scn, e.results(), e.hashes(), ores, oh, "pqueue, wave", mode=TIE["pqueue"])


# ------------------------------------------------------- d. prefix and sweep paths
@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", ["dense", "narrow", "half"])
@pytest.mark.parametrize("seed", SEEDS)
def test_prefix_on_random_images(engine_mod, oracle_mod, seed, geo):
    scn = _scn(seed, "table")
    assert scn.main_regs is None
    ores, oh = _ref(seed, "table")
    with engine_mod.Engine() as e:
        e.load(scn, geometry=geo)
        t0 = e.prefix_stats()["t0"]
        used = []
        for i in range(3):
            e.reset()
            e.run()
            used.append(e.prefix_stats()["last"])
            _same(scn, e.results(), e.hashes(), ores, oh, f"prefix pair {i} ({used[-1]}), {geo}, T0 {t0}")
        if t0 >= 1:
            assert used[1] in ("applied", "refused"), (seed, geo, t0, used)
        else:
            assert used == ["not_eligible"] * 3, (seed, geo, t0, used)
        e.set_prefix(False).reset()
        e.run()
        assert e.prefix_stats()["last"] == "not_eligible"
        _same(scn, e.results(), e.hashes(), ores, oh, f"prefix off, {geo}")


@pytest.mark.one_geometry
def test_prefix_seeds_have_a_prefix(engine_mod):
    """(d) is not vacuous: some table-mode image has T0 >= 1."""
    t0s = []
    with engine_mod.Engine() as e:
        for seed in QUARTER + [SEEDS[1]]:
            e.load(_scn(seed, "table"), geometry="dense")
            t0s.append(e.prefix_stats()["t0"])
    assert max(t0s) >= 1, t0s


# -------------------------------------------------------------- e. trace records
@functools.lru_cache(maxsize=None)
def _trace_ref(seed):
    import oracle

    scn = _scn(seed)
    logs = [tuple(trace_tuples(oracle.run(scn, replica=r, trace_cap=1 << 12).traces)) for r in range(scn.n_replicas)]
    assert max(len(t) for t in logs) < 1 << 12
    return logs


@pytest.mark.parametrize("seed", SEEDS[1::4])
def test_trace_records(engine_mod, oracle_mod, seed):
    scn = _scn(seed)
    logs = _trace_ref(seed)
    cap = max(len(t) for t in logs) + 1
    assert cap > 6
    some = (0, 277, GPU_REPLICAS - 1)          # first, one of the tail workgroup, last
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(cap).reset()
        e.run()
        _same(scn, e.results(), e.hashes(), *_ref(seed), "traced")
        for r in some:
            recs, n = e.trace(r)
            assert n == len(logs[r]), f"seed {seed}, replica {r}, field n_emitted; {reducer_command(scn, r)}"
            assert tuple(trace_tuples(recs)) == logs[r], f"seed {seed}, replica {r}, field trace; " \
                                                         f"{reducer_command(scn, r)}"
        e.set_trace(5).reset()
        e.run()
        for r in range(scn.n_replicas):
            recs, n = e.trace(r)
            assert n == len(logs[r]), f"seed {seed}, replica {r}, field n_emitted (cap 5); {reducer_command(scn, r)}"
            if r in some:
                assert tuple(trace_tuples(recs)) == logs[r][:5], f"seed {seed}, replica {r}, field trace (cap 5)"


# ---------------------------------------------------------- g. fused vs unfused
@pytest.mark.one_geometry
@pytest.mark.parametrize("geo", ["dense", "compact"])
@pytest.mark.parametrize("seed", [0, 3, 10, 14])
def test_fused_against_unfused(engine_mod, oracle_mod, monkeypatch, seed, geo):
    import oracle

    fused = _scn(seed)
    monkeypatch.setenv("TW_FUSE_PAIRS", "0")
    plain = net_soup(seed, GPU_REPLICAS)
    monkeypatch.delenv("TW_FUSE_PAIRS")
    assert netsoup.fused_flags(fused.image.insns) and not netsoup.fused_flags(plain.image.insns)
    assert fused.image.insns.shape == plain.image.insns.shape
    ores, oh = _ref(seed)
    pres, ph = oracle.run_batch(plain, threads=8)
    _same(plain, pres, ph, ores, oh, "oracle: unfused image against fused")
    for scn, what in ((fused, "fused"), (plain, "unfused")):
        with engine_mod.Engine() as e:
            e.load(scn, geometry=geo).reset()
            e.run()
            _same(scn, e.results(), e.hashes(), ores, oh, f"{what}, {geo}")
