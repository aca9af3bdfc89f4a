"""What the batched-LP feature programs (tests/lpprogs.py) reach, from the
oracle alone (CPU; nothing here calls the engine).

tests/test_gpu_lpprogs.py compares the LP kernels with the oracle on these
programs; this module keeps that comparison meaningful: every program stays
inside tw_lpb_load's contract and its declared lane capacities, few or no
replicas depend on the order of equal-time events (those are left out of the
GPU comparison), and the feature each program is named after actually occurs.
The figures are in profiles/lpprogs/oracle_reach.txt (python tests/lpprogs.py
--reach)."""
import functools

import numpy as np
import pytest

import lpprogs
from lpprogs import ALL_COMPARED, NAMES, THROW_CODES
from timewarp import isa


@functools.lru_cache(maxsize=None)
def _reach(name):
    scn = lpprogs.program(name)
    return scn, lpprogs.reach(scn)


@pytest.fixture
def reach(oracle_mod, request):
    return _reach(request.param)


def _for(*names):
    return pytest.mark.parametrize("reach", names, indirect=True)


def test_programs_are_deterministic_and_named():
    progs = lpprogs.lp_programs()
    assert list(progs) == NAMES and len(NAMES) == 11          # the ten features and two_owners_lp's twin
    again = lpprogs.lp_programs()
    for name, scn in progs.items():
        assert np.array_equal(scn.image.insns, again[name].image.insns), name
        assert np.array_equal(scn.link_table, again[name].link_table), name
        assert scn.n_replicas == (32 if name == "heavy_mixed" else 64), name
        if name != "heavy_mixed":
            assert 3 <= scn.n_nodes - 1 <= 6, name
        has_links = scn.topo.out_off[scn.main_node + 1] > scn.topo.out_off[scn.main_node]
        assert has_links == name.startswith("two_owners_lp"), name     # (the probe's link)
        assert (scn.main_regs is not None) == (name == "spawn_regs"), name
        for key in ("lp_inbox_cap", "lp_max_slots", "lp_queue_capacity", "lp_outbox_cap"):
            assert key in scn.meta, (name, key)


@_for(*NAMES)
def test_contract_and_capacities(reach):
    scn, f = reach
    name = f["name"]
    # every link delay >= the lookahead (the table's smallest delay, itself >= 50 µs): no phase-1 nodes
    assert f["min_delay"] >= f["lookahead"] >= lpprogs.LO, (name, f["lookahead"], f["min_delay"])
    assert f["short_dst"] == [], (name, f["short_dst"])
    assert (f["res"]["status"] == isa.REP_DONE).all(), (name, np.unique(f["res"]["status"]))
    for o in f["runs"]:
        assert o.result["status"] not in lpprogs.CAPACITY_ERRORS, name
    # sufficient bounds, not peaks: every message term a node ever hashes fits
    # its inbox, and every thread it ever had (per message term a deliverer, a
    # handler and a watchdog or child; plus the daemon and its own forks) its slots
    assert f["over_inbox"] == 0, (name, f["max_node_msgs"], scn.meta["lp_inbox_cap"])
    assert f["over_slots"] == 0, (name, f["max_node_msgs"], scn.meta["lp_max_slots"])
    assert scn.meta["lp_queue_capacity"] >= scn.meta["lp_max_slots"], name
    # (the watchdog epochs of a whole replica, hence of each of its lanes)
    begins = sum(1 for w in scn.image.insns[:, 0].tolist() if (w & 0xFF) == isa.OP_TMO_BEGIN)
    if begins:
        assert scn.max_timeouts >= int((f["res"]["delivered"]).max()), name


@_for(*NAMES)
def test_tie_orders(reach):
    """The replicas the GPU comparison keeps (netsoup.lp_compared: equal
    outputs under the canonical, LIFO, SCRAMBLE and FORKFIRST orders): a
    condition on the programs, not a measurement."""
    scn, f = reach
    kept, R = int(f["compared"].sum()), scn.n_replicas
    assert kept >= (29 if f["name"] == "heavy_mixed" else 58), (f["name"], kept, R)
    if f["name"] in ALL_COMPARED:
        assert kept == R, (f["name"], kept)
    if f["name"] == "slow_handler":
        assert kept < R, "slow_handler: no replica is left out, so the mask is never exercised"


@_for("timeout_handler")
def test_reach_timeout_handler(reach):
    scn, f = reach
    handlers = int(f["res"]["delivered"].sum())           # one handler per delivered message
    assert f["fired"] + f["completed"] == handlers
    assert 4 * f["fired"] >= handlers and 4 * f["completed"] >= handlers, (f["fired"], f["completed"], handlers)
    assert f["overlap"] > 0                                # two timeouts open at once on one node


@_for("throw_handler")
def test_reach_throw_handler(reach):
    scn, f = reach
    assert f["sites"] == {0, 1, 2, 3}, f["sites"]
    assert f["codes"] == set(THROW_CODES), f["codes"]      # (the codes the caught sites' handlers received)
    assert f["after_inline_throw"] > 0
    # the bare sites' throws leave no term (the thread just dies), but a handler
    # that did not throw on an odd payload would have replied: per replica the
    # 4 x 2 x 5 originals and one reply to each with an even payload, no more
    assert (f["res"]["delivered"] == 40 + 16).all() and (f["res"]["undeliverable"] == 0).all()


@_for("rebind_handler")
def test_reach_rebind_handler(reach):
    scn, f = reach
    assert f["owned"] > 0 and f["not_owned"] > 0
    assert (f["res"]["undeliverable"] > 0).all()


@_for("two_owners_lp", "two_owners_lp_twin")
def test_reach_two_owners(reach):
    scn, f = reach
    want = scn.meta["want"]
    assert (f["res"]["delivered"] == want["delivered"]).all() and want["delivered"] == (f["name"] != "two_owners_lp")
    assert (f["res"]["undeliverable"] == want["undeliverable"]).all()
    assert want["delivered"] + want["undeliverable"] == 1


@_for("raw_gate")
def test_reach_raw_gate(reach):
    scn, f = reach
    assert f["turned_away"] > 0 and f["accepted"] > 0


@_for("kinds_sets")
def test_reach_kinds_sets(reach):
    scn, f = reach
    # (reach() itself asserts that every UNDELIV term is of the kind its node's set lacks)
    assert f["missing_kind"] > 0 and f["missing_kind"] == int(f["res"]["undeliverable"].sum())
    assert f["inline_recv"] > 0 and f["forked_recv"] > 0 and f["stub_recv"] > 0
    ls = scn.image.listener_pc
    assert (ls[0] != isa.PC_NONE).all() and (ls[1:] == isa.PC_NONE).sum() == 2
    assert (ls[0] & isa.LPC_INLINE != 0).sum() == 1        # set 0: A inline, B forked


@_for("depth_wrap")
def test_reach_depth_wrap(reach):
    scn, f = reach
    assert scn.link_depth == 3 and scn.meta["drop_log2"] == 2
    # every daemon sends 8 originals over each of its links (the program's own
    # loop: no branch skips a send), so every link's ordinal wraps at least twice
    assert scn.meta["sends_per_link"] > 2 * scn.link_depth
    # and from the oracle's terms, per link (the payload names it): the fewest
    # messages any link of any replica carried
    assert f["min_link_msgs"] > 2 * scn.link_depth, f["min_link_msgs"]
    assert f["min_link_msgs"] >= scn.meta["sends_per_link"]
    assert (f["res"]["dropped"] > 0).all() and (f["res"]["delivered"] > 0).all()
    assert f["drop_kinds"] == {0, 1}                       # originals and replies


@_for("slow_handler")
def test_reach_slow_handler(reach):
    scn, f = reach
    assert 4 * f["recv_inside"] >= scn.n_replicas, f["recv_inside"]


@_for("spawn_regs")
def test_reach_spawn_regs(reach):
    scn, f = reach
    assert f["distinct"] >= 16, f["distinct"]
    assert set(scn.main_regs[:, 0].tolist()) == set(range(8)) and set(scn.main_regs[:, 1].tolist()) == {1, 2, 3, 4}


@_for("heavy_mixed")
def test_reach_heavy_mixed(reach):
    scn, f = reach
    assert min(f["window_peak"]) > 32, f["window_peak"]    # in every replica: the tw_lp_due path
    assert int(scn.meta["lp_inbox_cap"][scn.meta["receiver"]]) > 32
    assert f["recv_kinds"] == {0, 1}                       # Ping and Count both delivered
    assert f["undeliv_after_unlisten"] == scn.n_replicas
    assert scn.link_depth == 1                             # (classify_batch's condition)


def test_excluded_replicas_keep_their_message_count(oracle_mod):
    """The GPU test checks delivered + dropped + undeliverable on the replicas
    it leaves out: in these programs that sum does not depend on the tie order."""
    import oracle

    for name in NAMES:
        scn, f = _reach(name)
        if f["compared"].all():
            continue
        want = f["res"]["delivered"] + f["res"]["dropped"] + f["res"]["undeliverable"]
        for mode in (oracle.MODE_LIFO, oracle.MODE_SCRAMBLE, oracle.MODE_FORKFIRST):
            r2, _h = oracle.run_batch(scn, mode=mode, threads=8)
            assert np.array_equal(r2["delivered"] + r2["dropped"] + r2["undeliverable"], want), (name, mode)


def test_due_run_on_an_idle_lane(oracle_mod):
    """The reduced case of the hang heavy_mixed found (TW_LP_BATCH=0): every
    message reaches a heavy inbox after the last thread of its node has ended,
    and its handler is not batchable."""
    scn = lpprogs.due_run_on_an_idle_lane()
    f = lpprogs.reach(scn)
    assert (f["res"]["status"] == isa.REP_DONE).all() and f["compared"].all()
    assert f["over_inbox"] == 0 and f["over_slots"] == 0 and f["short_dst"] == []
    assert (np.asarray(scn.meta["lp_inbox_cap"])[:-1] > 32).all()         # heavy lanes: tw_lp_due
    assert (f["res"]["delivered"] == 12).all() and (f["res"]["undeliverable"] == 0).all()
    fused = [w for w in scn.image.insns[:, 0].tolist() if (w & 0xFF) == isa.OP_ADDI and (w >> 16) & isa.ALU_NSTORE]
    assert fused                                                         # the handler stores: not batchable
    for o in f["runs"]:
        # a node's daemon ends (its last RESUME term) before its first message arrives
        for node in range(scn.meta["n_daemons"]):
            own = [t for t, n, kind, _v in o.terms if n == node and kind >> 16 == isa.KIND_RESUME >> 16]
            first = min(t for t, n, kind, _v in o.terms if n == node and kind >> 16 == isa.KIND_RECV >> 16)
            assert min(own) < 10 and first >= lpprogs.LO


def test_window_mode_programs_are_grid_stride():
    """TW_LP_GRID = GRID_STRIDE makes these contexts' work lists grid-stride:
    they have more workgroups of lanes than that (the launch's condition), and
    the workgroup size here is the kernel's."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(__file__), "..", "time-warp_amd", "csrc", "engine_dev.hpp")).read()
    assert int(re.search(r"#define TW_WG_LP (\d+)", src).group(1)) == lpprogs.LP_WORKGROUP_LANES
    for name in lpprogs.WINDOW_MODE_PROGRAMS:
        assert lpprogs.lp_workgroups(lpprogs.program(name)) > lpprogs.GRID_STRIDE, name
