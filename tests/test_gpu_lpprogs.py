"""The batched logical-process kernels (tw_lpb_load, geometry "lpb") against
the oracle on the hand-written feature programs of tests/lpprogs.py: every
RESULT_FIELD but tie_flags and every node hash bit-exact (integer outputs, no
tolerances), on the replicas whose oracle outputs do not depend on the order
of equal-time events (netsoup.lp_compared -- the documented contract of
tw_lpb_load); the others must end DONE with the oracle's message count.

One test per program, so a failure or a time limit names its feature:
timeouts, throws, listen / unlisten from handlers, a second owner of an owned
binding, listenR, kinds without a handler, link_depth wrap-around, a handler
that waits between a node-variable update and its reply and forks a local
child, NLOADX / NSTOREX on the own node, per-replica main_regs in spawn
records, a heavy inbox with batchable and non-batchable handlers mixed.  Each
program also runs a second time in the same context (lane state reset),
some under the other window modes, two shards and with TRACE records, and
each once through the replica kernel with no mask, so that a mismatch in the
LP run is known to be the LP path's.  heavy_mixed with TW_LP_BATCH=0 found a
window that never completed (a due run on a lane with no thread left);
test_due_run_on_an_idle_lane is its reduced case.

What the programs reach is guarded on the CPU by tests/test_lpprogs_oracle.py.
A failure names program, replica and field; `python tests/lpprogs.py --program
P --replica r [--mode M]` replays the replica through the oracle without a GPU."""
import functools

import numpy as np
import pytest

import lpprogs
from lpprogs import NAMES, WINDOW_MODE_PROGRAMS
from timewarp import isa
from timewarp.abi import RESULT_FIELDS
from timewarp.measures import trace_tuples

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

SHARD_PROGRAMS = ("timeout_handler", "throw_handler")
TRACE_PROGRAMS = ("timeout_handler", "throw_handler", "raw_gate")


# ------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def _ref(name):
    """The program, the oracle's canonical run of its batch and the replicas
    compared (computed once, never written to)."""
    import netsoup
    import oracle

    scn = lpprogs.program(name)
    res, h = oracle.run_batch(scn, threads=8)
    keep = netsoup.lp_compared(scn, res, h)
    for a in (res, h, keep):
        a.setflags(write=False)
    return scn, res, h, keep


@functools.lru_cache(maxsize=None)
def _trace_ref(name):
    import oracle

    scn = _ref(name)[0]
    logs = [tuple(sorted(trace_tuples(oracle.run(scn, replica=r, trace_cap=1 << 12).traces)))
            for r in range(scn.n_replicas)]
    assert max(len(t) for t in logs) < 1 << 12
    return logs


def _same(name, res, h, ores, oh, what, only=None):
    """Every field and node hash of every replica (of `only`, a mask) equal."""
    rows = np.arange(len(ores)) if only is None else np.flatnonzero(only)
    for f in RESULT_FIELDS:
        if f == "tie_flags":
            continue
        bad = rows[res[f][rows] != ores[f][rows]]
        assert bad.size == 0, (f"{name} [{what}]: replica {bad[0]}, field {f}: gpu {res[f][bad[0]]} != oracle "
                               f"{ores[f][bad[0]]} ({bad.size} replicas differ); "
                               f"python tests/lpprogs.py --program {name} --replica {bad[0]}")
    bad = rows[(h[rows] != oh[rows]).any(axis=1)]
    if bad.size:
        nodes = np.flatnonzero(h[bad[0]] != oh[bad[0]]).tolist()
        raise AssertionError(f"{name} [{what}]: replica {bad[0]}, field hashes (nodes {nodes}; {bad.size} replicas "
                             f"differ); python tests/lpprogs.py --program {name} --replica {bad[0]}")


def _check_lp(name, e, what):
    """An LP run against the oracle: bit-exact on the compared replicas; the
    others (their outputs depend on the tie order) end DONE with the oracle's
    message count, which does not (tests/test_lpprogs_oracle.py)."""
    scn, ores, oh, keep = _ref(name)
    res, h = e.results(), e.hashes()
    _same(name, res, h, ores, oh, what, only=keep)
    for r in np.flatnonzero(~keep):
        assert res["status"][r] == isa.REP_DONE, f"{name} [{what}]: replica {r} (not compared), field status: " \
                                                 f"gpu {res['status'][r]}"
        got = int(res["delivered"][r]) + int(res["dropped"][r]) + int(res["undeliverable"][r])
        want = int(ores["delivered"][r]) + int(ores["dropped"][r]) + int(ores["undeliverable"][r])
        assert got == want, f"{name} [{what}]: replica {r} (not compared), delivered + dropped + undeliverable: " \
                            f"gpu {got} != oracle {want}"
    return res, h


def _load_lp(e, scn):
    e.load(scn, geometry="lpb")
    assert e.geometry() == "lpb"
    return e


# ------------------------------------------- the replica kernel, with no mask
@pytest.mark.parametrize("name", NAMES)
def test_replica_kernel(engine_mod, oracle_mod, name):
    """The default replica geometry on all replicas against the canonical
    oracle: the program itself is within what the engine runs bit-exact."""
    scn, ores, oh, _keep = _ref(name)
    st, res, h = engine_mod.run_scenario(scn)
    _same(name, res, h, ores, oh, "replica kernel")
    assert st.events == int(ores["events"].sum())


# ------------------------------------------------------------- the LP kernels
@pytest.mark.parametrize("name", NAMES)
def test_lp_kernel(engine_mod, oracle_mod, name):
    scn, ores, oh, keep = _ref(name)
    with engine_mod.Engine(0) as e:
        _load_lp(e, scn).reset()
        e.run()
        res, h = _check_lp(name, e, "lpb")
        windows, ticks = e.lpb_windows()
        assert windows > 1 and ticks >= windows, (name, windows, ticks)
        if name == "heavy_mixed":
            # the due run's batchable prefix is closed by a non-batchable record
            batched, due = e.lpb_batch()
            assert due > 0 and 0 < batched < due, (batched, due)
        # lane state reset: the watchdog table and epoch counters, the cached
        # bindings and owners, spawn counts
        e.reset()
        e.run()
        res2, h2 = _check_lp(name, e, "lpb, second run")
        for f in RESULT_FIELDS:
            if f != "tie_flags":
                assert np.array_equal(res[f], res2[f]), f"{name}: second run, field {f} differs from the first"
        assert np.array_equal(h, h2), f"{name}: second run, node hashes differ from the first"
    if name.startswith("two_owners_lp"):
        want = scn.meta["want"]
        assert (res["delivered"] == want["delivered"]).all() and (res["undeliverable"] == want["undeliverable"]).all()


def test_heavy_mixed_without_the_batch(engine_mod, oracle_mod, monkeypatch):
    """TW_LP_BATCH=0: every due record on the receiver's chain; same outputs.
    (The run that found the hang of DESIGN.md, section 2, feature programs: the
    second burst comes as a due run to a receiver without a thread left.)"""
    monkeypatch.setenv("TW_LP_BATCH", "0")
    scn = _ref("heavy_mixed")[0]
    with engine_mod.Engine(0) as e:
        _load_lp(e, scn).reset()
        e.run()
        _check_lp("heavy_mixed", e, "lpb, TW_LP_BATCH=0")
        batched, due = e.lpb_batch()
        assert batched == 0 and due > 0, (batched, due)


@pytest.mark.parametrize("windows", ["per_replica", "global"])
def test_due_run_on_an_idle_lane(engine_mod, oracle_mod, monkeypatch, windows):
    """lpprogs.due_run_on_an_idle_lane, what the run above reduced to: a due run
    whose lane has no thread left, handlers that tw_lp_batch does not take.
    The lane must pop its run all the same; both window modes, twice each."""
    if windows == "global":
        monkeypatch.setenv("TW_LPB_GLOBAL", "1")
    name = "due_run_on_an_idle_lane"
    scn = _ref(name)[0]
    with engine_mod.Engine(0) as e:
        _load_lp(e, scn).reset()
        e.run()
        _check_lp(name, e, f"lpb, {windows}")
        batched, due = e.lpb_batch()
        assert batched == 0 and due == 12 * scn.n_replicas, (batched, due)
        e.reset()
        e.run()
        _check_lp(name, e, f"lpb, {windows}, second run")


@pytest.mark.parametrize("mode", ["global", "grid3", "grid_stride"])
@pytest.mark.parametrize("name", WINDOW_MODE_PROGRAMS)
def test_window_modes(engine_mod, oracle_mod, monkeypatch, name, mode):
    """One window for the whole batch (TW_LPB_GLOBAL=1); TW_LP_GRID=3, which at
    these contexts' three workgroups of lanes is still the plain launch; and
    TW_LP_GRID=1, under which one workgroup walks every window's work list
    grid-stride (the launch takes that form only for a context of more
    workgroups than the grid)."""
    env = {"global": ("TW_LPB_GLOBAL", "1"), "grid3": ("TW_LP_GRID", "3"),
           "grid_stride": ("TW_LP_GRID", str(lpprogs.GRID_STRIDE))}[mode]
    monkeypatch.setenv(*env)
    scn = _ref(name)[0]
    if mode == "grid_stride":
        assert lpprogs.lp_workgroups(scn) > lpprogs.GRID_STRIDE
    with engine_mod.Engine(0) as e:
        _load_lp(e, scn).reset()
        e.run()
        _check_lp(name, e, f"lpb, {mode}")
        windows, ticks = e.lpb_windows()
        assert windows > 1 and ticks >= windows, (name, mode, windows, ticks)


@pytest.mark.parametrize("name", SHARD_PROGRAMS)
def test_two_shards_of_one_gpu(engine_mod, oracle_mod, name):
    """Two shards of 32 replicas each on one device."""
    scn = _ref(name)[0]
    with engine_mod.Engine(devices=[0, 0]) as e:
        _load_lp(e, scn).reset()
        e.run()
        _check_lp(name, e, "lpb, two shards")


@pytest.mark.parametrize("name", TRACE_PROGRAMS)
def test_trace_records(engine_mod, oracle_mod, name):
    """TRACE records of an LP run: n_emitted and tw_read_trace's canonical
    order (t, node, tag, val) against the oracle's log sorted by the same key."""
    scn, _ores, _oh, keep = _ref(name)
    logs = _trace_ref(name)
    cap = max(len(t) for t in logs) + 1
    some = (0, 31, 63)
    assert all(keep[r] for r in some)
    with engine_mod.Engine(0) as e:
        _load_lp(e, scn).set_trace(cap).reset()
        e.run()
        _check_lp(name, e, "lpb, traced")
        for r in some:
            recs, n = e.trace(r)
            assert n == len(logs[r]), f"{name} [traced]: replica {r}, field n_emitted: gpu {n} != oracle {len(logs[r])}"
            assert tuple(trace_tuples(recs)) == logs[r], f"{name} [traced]: replica {r}, field trace; " \
                                                         f"python tests/lpprogs.py --program {name} --replica {r}"
