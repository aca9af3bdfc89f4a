"""What the inputs of tests/test_gpu_live.py reach, stated on the oracle alone
(CPU), so that the GPU tests cannot pass vacuously.  The seeds of
tests/livesoup.py were chosen here: `python tests/livesoup.py --search N`
prints coverage() of seeds 0 .. N-1.

For every soup seed, with the live arrays drawn from it:
  * links of kind 1 and of kind 2 are sent over;
  * some replica makes no draw at all;
  * some replica draws after one of its daemons was killed;
  * a link with range [0, 0], one with [0, 2] and one with [1000, 5000] are
    drawn from;
  * at least a quarter of the 300 replicas are pairwise distinct in outcome;
  * no capacity status occurs anywhere.
The diverge="table" soup of the prefix test runs one program in every
replica, so every replica draws: it is held to everything but the second
point, and its kill is followed by draws in every replica."""
import numpy as np
import pytest

import livesoup
from livesoup import CAPACITY, LIVE_SEEDS, SEED_BASE, TABLE_SEED, coverage, live_ring, live_soup, recorded
from netsoup import GPU_REPLICAS
from timewarp import scenarios


@pytest.mark.parametrize("seed", LIVE_SEEDS)
def test_soup_seed_reaches_what_the_gpu_tests_need(oracle_mod, seed):
    c = coverage(seed)
    print(c)
    assert c["kind1_sends"] > 0 and c["kind2_sends"] > 0, c
    assert c["kind0_links"] > 0, c                       # (kinds over {0, 1, 2}: the table is still read)
    assert c["no_draw"] > 0, c
    assert c["after_kill"] > 0, c
    assert {(0, 0), (0, 2), (1000, 5000)} <= c["drawn_ranges"], c
    assert c["distinct"] >= GPU_REPLICAS // 4, c
    assert not (c["statuses"] & set(CAPACITY)), c
    assert livesoup.meets(c)


def test_table_soup_reaches_what_the_prefix_test_needs(oracle_mod):
    c = coverage(TABLE_SEED, "table")
    print(c)
    assert live_soup(TABLE_SEED, "table").main_regs is None      # the send-free prefix's condition
    assert c["kind1_sends"] > 0 and c["kind2_sends"] > 0 and c["kind0_links"] > 0, c
    assert c["after_kill"] == GPU_REPLICAS, c
    assert {(0, 0), (0, 2), (1000, 5000)} <= c["drawn_ranges"], c
    assert c["distinct"] >= GPU_REPLICAS // 4, c
    assert not (c["statuses"] & set(CAPACITY)), c
    assert livesoup.meets(c, table_mode=True)


def test_a_reversed_range_is_drawn_from_somewhere(oracle_mod):
    """Every input's kinds cover {0, 1, 2}; a reversed range (randomR swaps
    it) is drawn from in at least one of them."""
    rev = [r for r in livesoup.RANGES if r[0] > r[1]]
    assert rev
    hit = []
    for seed, diverge in [(s, "regs") for s in LIVE_SEEDS] + [(TABLE_SEED, "table")]:
        scn = live_soup(seed, diverge)
        assert set(np.unique(scn.live_kind).tolist()) == {0, 1, 2}, seed
        hit += [seed for r in rev if r in coverage(seed, diverge)["drawn_ranges"]]
    assert hit


def test_ring_draws_once_per_token_and_replicas_differ(oracle_mod):
    """The seed batch of the GPU tests: the ring's kind-2 links are the ring
    links, one draw per token sent; the replicas' generators differ, so do
    most outcomes; the live scenario carries no table."""
    scn = live_ring(GPU_REPLICAS)
    assert scn.link_table is None and scn.link_depth == 1
    tabled = scenarios.token_ring(16, 2, launch_duration=20_000_000)
    assert tabled.link_table is not None
    for a, b in ((scn.live_kind, tabled.live_kind), (scn.live_lo, tabled.live_lo), (scn.live_hi, tabled.live_hi)):
        assert np.array_equal(a, b)
    assert np.array_equal(scn.image.insns, tabled.image.insns)
    outcomes, draws = set(), 0
    for r in range(0, GPU_REPLICAS, 7):
        res, sends, rec, _ = recorded(scn, r, SEED_BASE + r)
        k2 = scn.live_kind == 2
        assert sends[k2].sum() > 0 and sends[scn.live_kind == 1].sum() > 0
        ent = rec[k2][rec[k2] != livesoup.SENTINEL]
        assert ((ent >= 1000) & (ent <= 5000)).all(), r
        draws += livesoup.draws_of(scn, sends)
        outcomes.add(tuple(ent.tolist()))          # (the drawn delays themselves: the counts are the same)
        assert res["status"] not in CAPACITY
    assert draws > 0 and len(outcomes) > 1


def test_ping_pong_and_hotspot_carry_live_arrays(oracle_mod):
    pp = scenarios.ping_pong(n_replicas=2, network_delay=(1000, 5000))
    assert pp.live_kind.tolist() == [2, 2] and pp.live_lo.tolist() == [1000, 1000] and pp.live_hi.tolist() == [5000, 5000]
    hs = scenarios.hotspot(n_senders=4, n_replicas=2, msg_num=3, network_delay=(1000, 5000))
    L = hs.topo.n_links
    assert hs.live_kind.tolist() == [2] * L and hs.live_lo.tolist() == [1000] * L and hs.live_hi.tolist() == [5000] * L
    for scn in (pp, hs):   # the oracle runs them live: every delivery a draw
        o = oracle_mod.run(scn, replica=1, live_seed=5)
        assert o.result["status"] == 1 and o.result["delivered"] > 0
