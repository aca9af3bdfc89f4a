"""What the net soup's committed seed lists cover, from the oracle alone (CPU).

tests/test_gpu_netsoup.py compares the engine with the oracle on these seeds;
this module keeps that comparison from quietly becoming vacuous: every class
of behaviour the soup exists for must occur in some seed, the replicas of a
batch must diverge, and the capacities must be generous enough that no
replica stops for want of room.  The figures themselves are in
profiles/netsoup/oracle_coverage.txt (python tests/netsoup.py --coverage)."""
import numpy as np
import pytest

import netsoup
import progs
from netsoup import FUSED_FLAGS, GPU_REPLICAS, LP_REPLICAS, LP_SEEDS, SEEDS
from timewarp import isa

CAPACITY_ERRORS = (isa.REP_ERR_SLOTS, isa.REP_ERR_QUEUE, isa.REP_ERR_FRAMES, isa.REP_ERR_COUNTER)


@pytest.fixture(scope="module")
def cov(oracle_mod):
    return netsoup.coverage(SEEDS, GPU_REPLICAS, "replica", "regs")


@pytest.fixture(scope="module")
def cov_table(oracle_mod):
    return netsoup.coverage(SEEDS, GPU_REPLICAS, "replica", "table", term_replicas=0)


@pytest.fixture(scope="module")
def cov_lp(oracle_mod):
    return netsoup.coverage(LP_SEEDS, LP_REPLICAS, "lp", "regs", term_replicas=0)


def test_generator_is_deterministic():
    a, b = netsoup.net_soup(5, 8), netsoup.net_soup(5, 8)
    assert np.array_equal(a.image.insns, b.image.insns) and np.array_equal(a.link_table, b.link_table)
    assert np.array_equal(a.main_regs, b.main_regs) and np.array_equal(a.topo.dst, b.topo.dst)
    c = netsoup.net_soup(6, 8)
    assert a.image.insns.shape != c.image.insns.shape or not np.array_equal(a.image.insns, c.image.insns)
    # a replica's inputs do not depend on the size of the batch it is drawn in
    big = netsoup.net_soup(5, 40)
    assert np.array_equal(big.link_table[:, :, :8], a.link_table)


def test_message_counters_are_exercised(cov):
    for f in ("delivered", "dropped", "undeliverable"):
        hit = sum(1 for row in cov if row["res"][f].sum() > 0)
        assert 2 * hit >= len(cov), (f, hit)


def test_error_and_done_within_one_batch(cov):
    mixed = [row["seed"] for row in cov
             if row["status"].get(isa.REP_ERR_INSN, 0) and row["status"].get(isa.REP_DONE, 0)]
    assert mixed


def test_kill_of_a_bound_daemon(cov):
    """main killThreads a daemon that owns its listener (the binding is
    released with the thread), and one with a delivery still in flight: the
    term log has TW_KIND_EXC at its node and a TW_KIND_UNDELIV there later."""
    assert sum(row["killed_owned"] for row in cov) > 0
    assert sum(row["killed_pending"] for row in cov) > 0


def test_inline_handler_throws_uncaught(cov):
    assert sum(row["inline_uncaught_throw"] for row in cov) > 0


def test_handler_rebinds_its_node(cov):
    assert sum(row["rebinds"] for row in cov) > 0


def test_link_depth_wraps(cov):
    """Some replica attempts more sends than links x link_depth: some link's
    ordinal then passed its depth (pigeonhole)."""
    assert sum(row["wraps"] for row in cov) > 0
    assert {row["scn"].link_depth for row in cov} == {1, 2, 3}


def test_transmission_time_and_far_queue_seeds(cov):
    assert any(row["scn"].msg_bytes is not None for row in cov)
    assert any(row["scn"].meta["hi"] == 0 for row in cov)            # tie-heavy
    assert any(not row["scn"].meta["symmetric"] for row in cov)      # RLINK without a reverse link
    assert any(row["scn"].meta["raw"] for row in cov)                # a listenR set
    assert {row["scn"].near_horizon_us for row in cov} == {64, 10_000_000}


def test_every_fused_flag_occurs(cov):
    seen = set().union(*(row["flags"] for row in cov))
    assert seen == set(FUSED_FLAGS)
    # each of SETI, ADDI, NOW and NODE with the NSTORE after it
    ops = set().union(*(netsoup.fused_nstore_ops(row["scn"].image.insns) for row in cov))
    assert ops >= {isa.OP_SETI, isa.OP_ADDI, isa.OP_NOW, isa.OP_NODE}, ops


def test_no_fused_flag_without_fusion(monkeypatch):
    monkeypatch.setenv("TW_FUSE_PAIRS", "0")
    for seed in SEEDS:
        assert not netsoup.fused_flags(netsoup.net_soup(seed, 4).image.insns), seed


def test_a_jump_targets_the_second_half_of_a_fused_pair(cov):
    hit = 0
    for row in cov:
        ins = row["scn"].image.insns
        fused = {pc + 1 for pc, w in enumerate(ins[:, 0].tolist())
                 if ((w & 0xFF) == isa.OP_SEND and (w >> 16) & (isa.SEND_VIA_LINK | isa.SEND_VIA_RLINK))
                 or ((w & 0xFF) == isa.OP_TRACE and (w >> 16) & isa.TRACE_PAIR)}
        jumps = {int(imm) for w, imm in ins.tolist() if isa.OP_JMP <= (w & 0xFF) <= isa.OP_JNEI}
        hit += bool(fused & jumps)
    assert hit > 0


@pytest.mark.parametrize("which", ["regs", "table", "lp"])
def test_statuses(which, cov, cov_table, cov_lp):
    rows = dict(regs=cov, table=cov_table, lp=cov_lp)[which]
    status = np.concatenate([row["res"]["status"] for row in rows])
    assert not np.isin(status, CAPACITY_ERRORS).any()
    assert np.isin(status, (isa.REP_DONE, isa.REP_ERR_INSN)).mean() >= 0.9


def test_lanes_diverge(cov, cov_table, cov_lp):
    """(events, hash sum) takes at least R / 4 values within every seed whose
    replicas have registers of their own; replicas that differ by their
    link-table column alone diverge that much in at least half of the seeds
    (a deliberate deviation from "within every seed", DESIGN section 2: with
    equal registers, a small topology and few drops there are not 75 different
    outcomes to reach), and every one of them in more than one way."""
    for row in cov + cov_lp:
        assert 4 * row["distinct"] >= row["scn"].n_replicas, (row["seed"], row["distinct"])
    assert 2 * sum(4 * row["distinct"] >= GPU_REPLICAS for row in cov_table) >= len(cov_table)
    assert all(row["scn"].main_regs is None for row in cov_table)
    assert all(row["distinct"] > 1 for row in cov_table)


def test_lp_exclusions_are_few(cov_lp):
    """Replicas left out of the batched-LP comparison (tie-order dependent or
    not DONE): at most 10 % over the seed list, at most half of any seed."""
    ex = [row["excluded"] for row in cov_lp]
    assert sum(ex) <= 0.10 * LP_REPLICAS * len(cov_lp), ex
    assert max(ex) <= LP_REPLICAS // 2, ex
    assert any(row["scn"].meta["fan_in"] for row in cov_lp)
    caps = [int(row["scn"].meta["lp_inbox_cap"][0]) for row in cov_lp]
    assert min(caps) <= 32 < max(caps)      # light inboxes and heavy ones


def test_reducer_prints_a_replica(oracle_mod):
    scn = netsoup.net_soup(3, 8)
    text = netsoup.describe(scn, 5)
    assert "daemon0:" in text and "== term log" in text and "link  0:" in text
    assert netsoup.reducer_command(scn, 5).startswith("python tests/netsoup.py --seed 3 --replica 5 ")


def test_owned_listener_two_owners(oracle_mod):
    """The case the soup's seed 12 reduced to, on the oracle: a former owner's
    death does not reopen a port its current owner's death closed."""
    scn, want = progs.owned_listener_two_owners()
    for mode in (0, 1, 2, 3, 5):
        o = oracle_mod.run(scn, mode=mode)
        assert o.result["status"] == isa.REP_DONE
        for f in ("delivered", "undeliverable", "final_t"):
            assert o.result[f] == want[f], (mode, f)
        assert [v for _t, _n, tag, v in o.traces if tag == progs.TAG_CP] == want["cps"]
