"""Live delays for the tests: the soups of tests/netsoup.py (imported, not
edited) and the token ring made live, their oracle references, and what the
oracle alone says the inputs reach (tests/test_live_oracle.py).

A soup's live arrays are drawn from its seed: every link gets a kind from
{0, 1, 2} and a range from RANGES.  Replica r of a batch draws from
mkStdGen(seed_base + r), so its reference is
`oracle.run(scn, replica=r, mode=m, live_seed=seed_base + r)`.

Replay one replica through the oracle without a GPU:
    python tests/livesoup.py --seed S --replica r [--mode M] [--diverge table]
"""
import ctypes as C
import functools

import numpy as np

from netsoup import GPU_REPLICAS, net_soup
from timewarp import isa, scenarios
from timewarp.abi import RESULT_DTYPE, RESULT_FIELDS, TwReplicaResult

# the ranges a soup's links draw from; the last one is reversed (randomR swaps it)
RANGES = ((0, 0), (0, 2), (0, 5), (1000, 5000), (40, 7))
# soup seeds of the GPU tests, chosen on the CPU so that the oracle meets every
# requirement of test_live_oracle.py (coverage(); `python tests/livesoup.py --search`)
LIVE_SEEDS = (381, 1057)
TABLE_SEED = 17          # the diverge="table" soup of the prefix / sweep test
SEED_BASE = 7            # replica r draws from mkStdGen(SEED_BASE + r)
SENTINEL = 0xFFFFFFFF    # a record entry no send wrote (a live entry has bit 31 clear)
CAPACITY = (isa.REP_ERR_SLOTS, isa.REP_ERR_QUEUE, isa.REP_ERR_FRAMES, isa.REP_ERR_COUNTER)


def live_arrays(topo, seed: int):
    """(kind, lo, hi) of a soup's links, from its seed.  Kinds are over
    {0, 1, 2}: every source node draws a dominant kind, which each of its
    out-links takes with probability 0.8 (else any kind) -- a replica makes no
    draw at all only when every drawn link it would send over belongs to
    daemons that never get to send in it (killed before their first period is
    over), which uniform kinds per link practically never leave room for.
    The kind-2 links take the RANGES in turn, from a shuffled start (a soup
    with five of them draws from every range), the others any."""
    rng = np.random.default_rng([int(seed), 0x6c697665])
    n_links = topo.n_links
    dominant = rng.integers(0, 3, size=topo.n_nodes)[topo.src_of()] if n_links else np.zeros(0, np.int64)
    kind = np.where(rng.random(n_links) < 0.8, dominant, rng.integers(0, 3, size=n_links)).astype(np.uint32)
    pick = rng.integers(0, len(RANGES), size=n_links)
    order = rng.permutation(len(RANGES))
    two = np.flatnonzero(kind == 2)
    pick[two] = order[np.arange(two.size) % len(RANGES)]
    lo = np.array([RANGES[i][0] for i in pick], np.int64)
    hi = np.array([RANGES[i][1] for i in pick], np.int64)
    return kind, lo, hi


@functools.lru_cache(maxsize=None)
def live_soup(seed: int, diverge: str = "regs", n_replicas: int = GPU_REPLICAS):
    scn = net_soup(seed, n_replicas, "replica", diverge)
    scn.live_kind, scn.live_lo, scn.live_hi = live_arrays(scn.topo, seed)
    return scn


@functools.lru_cache(maxsize=None)
def live_ring(n_replicas: int):
    """BASELINE config 1's ring (16 nodes, 20 s) without a table."""
    return scenarios.token_ring(16, n_replicas, launch_duration=20_000_000, live=True)


def oracle_batch(scn, seed_base: int = SEED_BASE, mode: int = 0, **kw):
    """Every replica's oracle run under live delays: (results, hashes)."""
    import oracle

    res = np.zeros(scn.n_replicas, RESULT_DTYPE)
    h = np.zeros((scn.n_replicas, scn.n_nodes), np.uint64)
    for r in range(scn.n_replicas):
        o = oracle.run(scn, replica=r, mode=mode, live_seed=seed_base + r, trace_cap=1, **kw)
        for f in RESULT_FIELDS:
            res[f][r] = o.result[f]
        h[r] = o.hashes
    res.setflags(write=False)
    h.setflags(write=False)
    return res, h


@functools.lru_cache(maxsize=None)
def ref(name, seed_base: int = SEED_BASE, mode: int = 0):
    """oracle_batch of a named input: ("soup", seed, diverge) or ("ring", n_replicas)."""
    return oracle_batch(scenario(name), seed_base, mode)


def scenario(name):
    return live_soup(name[1], name[2]) if name[0] == "soup" else live_ring(name[1])


def same(scn, res, h, ores, oh, what, seed_base: int = SEED_BASE, mode: int = 0):
    """Every field and node hash of every replica equal; the message names the
    replica, its generator's seed and the command that replays it."""
    def where(r):
        m = scn.meta
        cmd = (f"python tests/livesoup.py --seed {m['seed']} --replica {r} --diverge {m['diverge']} --mode {mode} "
               f"--seed-base {seed_base}") if m.get("config") == "net_soup" else "the ring"
        return f"{scn.name} [{what}]: replica {r}, live seed {seed_base + r} (seed_base {seed_base}); {cmd}"

    for f in RESULT_FIELDS:
        bad = np.flatnonzero(res[f] != ores[f])
        assert bad.size == 0, (f"{where(int(bad[0]))}: field {f}: gpu {res[f][bad[0]]} != oracle {ores[f][bad[0]]} "
                               f"({bad.size} replicas differ)")
    bad = np.flatnonzero((h != oh).any(axis=1))
    if bad.size:
        nodes = np.flatnonzero(h[bad[0]] != oh[bad[0]]).tolist()
        raise AssertionError(f"{where(int(bad[0]))}: node hashes {nodes} ({bad.size} replicas differ)")


# ------------------------------------------------------- what the oracle reaches
def recorded(scn, replica: int, live_seed: int, t_end: int = 1 << 62, depth: int = 256, term_cap: int = 0,
             max_events: int = 0):
    """One live oracle run with the record buffer pre-filled with SENTINEL:
    (result dict, sends per link over live links, the recorded entries
    [n_links][depth], terms).  oracle.run zero-fills its buffer, which hides a
    send whose delay is 0; this calls the same entry point with its own."""
    import oracle

    L = oracle.lib()
    d = scn.desc()
    o = oracle.TwoOpts()
    o.mode, o.t_end, o.max_events = 0, t_end, max_events
    terms = None
    if term_cap:
        terms = (oracle.TwoTerm * term_cap)()
        o.terms = C.cast(terms, C.POINTER(oracle.TwoTerm))
        o.terms_cap = term_cap
    kind = np.ascontiguousarray(scn.live_kind, np.uint32)
    lo = np.ascontiguousarray(scn.live_lo, np.int64)
    hi = np.ascontiguousarray(scn.live_hi, np.int64)
    rec = np.full((scn.topo.n_links, depth), SENTINEL, np.uint32)
    live = oracle.TwoLiveDelays(kind=kind.ctypes.data, lo=lo.ctypes.data, hi=hi.ctypes.data, seed=live_seed,
                                record=rec.ctypes.data, record_depth=depth, record_overflow=0)
    o.live = C.pointer(live)
    res = TwReplicaResult()
    hashes = np.zeros(scn.n_nodes, np.uint64)
    rc = L.two_run(C.addressof(d), replica, C.byref(o), C.byref(res), hashes.ctypes.data)
    assert rc == 0 and not live.record_overflow, (rc, live.record_overflow)
    tm = [(terms[i].t, terms[i].node, terms[i].kind, terms[i].val) for i in range(min(o.terms_n, term_cap))] \
        if terms is not None else []
    assert not term_cap or o.terms_n < term_cap
    return {f: getattr(res, f) for f in RESULT_FIELDS}, (rec != SENTINEL).sum(axis=1), rec, tm


def draws_of(scn, sends) -> int:
    """generator steps of a replica: its sends over kind-2 links"""
    return int(sends[np.asarray(scn.live_kind) == 2].sum())


def coverage(seed: int, diverge: str = "regs", seed_base: int = SEED_BASE, n_replicas: int = GPU_REPLICAS) -> dict:
    """What a live soup reaches, from the oracle alone."""
    scn = live_soup(seed, diverge, n_replicas)
    kind, lo, hi = (np.asarray(a) for a in (scn.live_kind, scn.live_lo, scn.live_hi))
    kn = scn.meta["kill_node"]
    exc_tk = isa.KIND_EXC | isa.EXC_THREAD_KILLED
    tot = np.zeros(scn.topo.n_links, np.int64)
    draws = np.zeros(n_replicas, np.int64)
    after_kill = 0
    outcomes = set()
    statuses = set()
    for r in range(n_replicas):
        res, sends, _rec, terms = recorded(scn, r, seed_base + r, term_cap=1 << 14)
        tot += sends
        draws[r] = draws_of(scn, sends)
        statuses.add(int(res["status"]))
        outcomes.add(tuple(int(res[f]) for f in RESULT_FIELDS))
        if kn is not None and draws[r]:
            at = [t for t, node, k, _v in terms if node == kn and k == exc_tk]
            if at:
                _res, before, _rec, _t = recorded(scn, r, seed_base + r, t_end=at[0])
                after_kill += draws_of(scn, before) < draws[r]
    drawn = {(int(lo[l]), int(hi[l])) for l in range(len(kind)) if kind[l] == 2 and tot[l]}
    return dict(seed=seed, kind1_sends=int(tot[kind == 1].sum()), kind2_sends=int(tot[kind == 2].sum()),
                kind0_links=int((kind == 0).sum()), no_draw=int((draws == 0).sum()), after_kill=int(after_kill),
                drawn_ranges=drawn, distinct=len(outcomes), statuses=statuses, draws=int(draws.sum()))


def meets(c: dict, table_mode: bool = False) -> bool:
    need = {(0, 0), (0, 2), (1000, 5000)}
    return (c["kind1_sends"] > 0 and c["kind2_sends"] > 0 and need <= c["drawn_ranges"]
            and c["distinct"] >= GPU_REPLICAS // 4 and not (c["statuses"] & set(CAPACITY))
            and (table_mode or (c["no_draw"] > 0 and c["after_kill"] > 0)))


def _main(argv=None):
    import argparse

    import oracle

    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=LIVE_SEEDS[0])
    ap.add_argument("--replica", type=int, default=0)
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--diverge", default="regs", choices=["regs", "table"])
    ap.add_argument("--seed-base", type=int, default=SEED_BASE)
    ap.add_argument("--search", type=int, default=0, help="report coverage() of seeds 0 .. N-1")
    a = ap.parse_args(argv)
    if a.search:
        for s in range(a.search):
            try:
                c = coverage(s, a.diverge)
            except AssertionError as e:  # (a log or record buffer too small for this seed)
                print(False, s, "skipped:", e, flush=True)
                continue
            print(meets(c, a.diverge == "table"), c, flush=True)
        return
    scn = live_soup(a.seed, a.diverge)
    print("kind", scn.live_kind.tolist(), "lo", scn.live_lo.tolist(), "hi", scn.live_hi.tolist())
    o = oracle.run(scn, replica=a.replica, mode=a.mode, live_seed=a.seed_base + a.replica, term_cap=1 << 14)
    print(o.result)
    print("hashes", o.hashes.tolist())
    for t in o.terms:
        print(t)


if __name__ == "__main__":
    _main()
