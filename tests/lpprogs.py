"""Hand-written feature programs for the batched logical-process kernels
(tw_lpb_load, geometry "lpb"): one small named program per feature that the
LP path has code of its own for (`if constexpr (LP)`, `c.lpb`, the lane's
cached binding words DW_BSET / DW_BOWN, the per-lane watchdog counter CW_TMO,
spawn records, tw_lp_due / tw_lp_batch), each inside tw_lpb_load's documented
contract and compared bit-exact with the oracle.

`lp_programs()` returns name -> Scenario.  Shared by tests/test_lpprogs_oracle.py
(CPU: what the programs reach, from the oracle alone) and
tests/test_gpu_lpprogs.py (GPU).  Run as a script it prints the figures of
profiles/lpprogs/oracle_reach.txt:

    python tests/lpprogs.py --reach

The common shape (net soup's, tests/netsoup.py).  Nodes 0..N-1 carry one daemon
each; node N hosts `main`, which forks the daemons -- spawn records under the
LP kernel -- and ends.  Nobody uses a ref to a thread on another node, nobody
touches another node's variables, a handler sends at most once and a daemon at
most twice per round.  Link tables come from `scenarios.draw_table` over
[50, 50 + hi] µs, so the lookahead is at least 50 µs; the replicas differ by their
table column (in `spawn_regs` also by `main_regs`).  A message's payload is
its hop budget: a handler replies with payload - 1 only while it is > 0.

`meta` carries the per-lane capacities of Engine.load_lpb as sufficient
bounds, not peaks: `lp_inbox_cap[n]` is at least every message term (RECV,
DROP, UNDELIV) node n ever hashes, `lp_max_slots` at least every thread a node
ever had (`lp_threads_per_msg` per message term -- deliverer, handler and a
watchdog or a local child -- plus `lp_threads_extra` for the daemon and its
own forks); tests/test_lpprogs_oracle.py checks both against the oracle's term
logs.  `max_timeouts` bounds the TMO_BEGINs of a whole replica, hence of each
of its lanes (the LP kernel counts watchdog epochs per lane).

Handler registers (include/timewarp.h TW_OP_DELIVER): r0 payload, r1 incoming
link, r2 sender node, r3 kind."""
from __future__ import annotations

import os
import sys
from collections import OrderedDict

import numpy as np

try:
    from timewarp import isa
except ImportError:  # run as a script: no conftest has set the path
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_ROOT, "time-warp_amd"), os.path.join(_ROOT, "oracle")]
    from timewarp import isa
from timewarp.program import Program
from timewarp.scenario import Scenario, Topology
from timewarp.scenarios import draw_table
from timewarp.timeunits import for_

ALL = isa.MASK_ALL
TK, ARITH, USER0, TIMEOUT = isa.EXC_THREAD_KILLED, isa.EXC_ARITH, isa.EXC_USER0, isa.EXC_TIMEOUT
LO = 50                  # every table's lower bound: the lookahead is at least this
REPLICAS = 64            # a power of two: one wave of 64 replicas per node
HEAVY_REPLICAS = 32

TAG_T = 200              # a handler's plain trace: TAG_T + handler id, the payload
TAG_CAUGHT = 400         # a catch_(ALL) handler ran: r3, the exception code
TAG_RAW = 401            # the raw (listenR) listener saw a message: the payload
TAG_REBIND = 402         # a handler is about to listen: the payload (even: owned)
TAG_UNLISTEN = 403       # a handler is about to unlisten
TAG_OPEN = 404           # a handler has begun a timeout: the payload
TAG_DONE = 405           # ... and ended it in time: the payload
TAG_STORE = 406          # slow_handler: the node counter as just stored
TAG_XVAR = 407           # slow_handler: NLOADX of what NSTOREX wrote on the own node
TAG_CHILD = 408          # slow_handler's local child: the counter its parent saw
TAG_REPLY = 409          # slow_handler: about to reply (the counter it stored)
TAG_COUNT = 410          # heavy_mixed's receiver: its Count counter at the unlisten
TAG_THROW = 500          # TAG_THROW + handler id: about to throw (the payload)

MSG_TERMS = (isa.KIND_RECV >> 16, isa.KIND_DROP >> 16, isa.KIND_UNDELIV >> 16)

# timeout_handler: (T, W) by payload mod 4 -- 0 and 3 fire (W >= T + 2), 1 and
# 2 complete (W <= T - 2); the watchdog is itself a fork (+1 µs), so T = W + 1
# would be decided by the order of equal-time events and never occurs
TIMEOUTS = ((3, 6), (5, 2), (8, 6), (2, 4))
# throw_handler: handler id -> (kind, inline, caught); odd payloads throw
THROW_SITES = {0: ("FC", False, True), 1: ("FB", False, False), 2: ("IC", True, True), 3: ("IB", True, False)}
THROW_CODES = (ARITH, USER0, TK)        # by payload mod 3


# ------------------------------------------------------------------ pieces
def _ring(N: int):
    """Node n's out-list: its two ring neighbours (link 0 forward, link 1
    back), so every link has a reverse; the main node N has no links."""
    return [[(n + 1) % N, (n - 1) % N] for n in range(N)] + [[]]


def _main(p: Program, N: int, regs=None, waits=None):
    """`main`: set the registers the daemons inherit (r0 period, r1 rounds),
    fork one daemon per node, end."""
    c = p.function("main")
    if regs is not None:
        c.seti(0, regs[0]).seti(1, regs[1])
    for n in range(N):
        c.seti(2, n).fork_(f"daemon{n}", node_reg=2, scratch=3)
        if waits is not None and waits[n]:
            c.wait(for_(waits[n]))
    c.end()


def _reply(c, kind, link_reg: int = 2):
    """Reply over the incoming link's reverse while the hop budget lasts."""
    skip = c.label()
    c.jeqi(0, 0, skip).addi(0, -1)
    c.reply_link(link_reg, 1).send(link_reg, kind, 0)
    c.bind(skip)


def _scenario(name, p, out, hi, msgs, n_replicas=REPLICAS, depth=1, drop_log2=0, seed_base=0, main_regs=None,
              max_timeouts=8, threads_per_msg=3, threads_extra=4, inbox_cap=None, table=None, **extra) -> Scenario:
    """`msgs`: an upper bound on the message terms of one node (of the whole
    replica where that is simpler); the lane capacities follow from it."""
    img = p.finalize()
    topo = Topology.from_out_lists(len(out), out)
    L = topo.n_links
    if table is None:
        table = draw_table(L, n_replicas, np.arange(L), LO, LO + hi, link_depth=depth, drop_log2=drop_log2,
                           seed_base=seed_base)
    N = len(out) - 1
    if inbox_cap is None:
        assert msgs <= 32
        inbox_cap = np.array([32] * N + [4], np.uint32)      # every inbox light: drained in the event kernel
    slots = threads_per_msg * int(max(inbox_cap)) + threads_extra
    meta = dict(config="lpprog", program=name, hi=hi, n_daemons=N, out=out, link_depth=depth, drop_log2=drop_log2,
                lp_inbox_cap=inbox_cap, lp_max_slots=slots, lp_queue_capacity=slots + 16,
                lp_outbox_cap=int((int(np.sum(inbox_cap)) + 2 * (N + 1) + 64) * n_replicas),
                lp_threads_per_msg=threads_per_msg, lp_threads_extra=threads_extra, **extra)
    return Scenario(
        name=f"lpprog_{name}", image=img, topo=topo, n_replicas=n_replicas, main_pc=img.pc_of("main"), main_node=N,
        link_table=table, main_regs=main_regs, max_slots=max(256, slots), queue_capacity=4096, run_capacity=512,
        max_timeouts=max_timeouts, max_frames=4, meta=meta)


# ---------------------------------------------------------------- programs
def timeout_handler() -> Scenario:
    """TMO_BEGIN / TMO_END / TMO_FIRE in a forked handler, under catch_(ALL):
    `timeout T (wait W)` with (T, W) = TIMEOUTS[payload mod 4]; a timeout that
    fires is caught (the code is traced) and the handler ends without a reply.
    The epoch register r3 holds the lane's watchdog count under the LP kernel
    and the replica's on the oracle: it is cleared before anything reads it
    (the catch handler finds the exception code there instead).  A daemon sends
    the same payload twice over one link, 1 µs apart (one table entry, so the
    same delay): the two handlers' timeouts overlap on the receiving node and
    claim consecutive epochs of its lane."""
    N, rounds = 4, 4
    p = Program()
    p.kind("A")
    p.listener_set({"A": "on_a"})
    _main(p, N, regs=(400, rounds))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(1 + 3 * n)).listen(0)
        loop = c.here()
        c.wait_reg(0)
        c.link(2, 0).send(2, "A", 1)
        c.link(3, 0).send(3, "A", 1)
        c.addi(1, -1).jnei(1, 0, loop)
        c.end()
    c = p.function("on_a")
    caught, done = c.label(), c.label()
    arms = [c.label() for _ in TIMEOUTS]
    c.catch_(ALL, caught)
    c.mov(2, 0).modi(2, 4)
    for k in range(1, len(TIMEOUTS)):
        c.jeqi(2, k, arms[k])
    for k, (t, w) in enumerate(TIMEOUTS):
        c.bind(arms[k])
        c.timeout_begin(t, epoch_reg=3)
        c.trace(TAG_OPEN, 0)
        c.wait(for_(w))
        c.timeout_end()
        c.jmp(done)
    c.bind(done)
    c.seti(3, 0)
    c.uncatch()
    c.trace(TAG_DONE, 0)
    _reply(c, "A")
    c.end()
    c.bind(caught)
    c.trace(TAG_CAUGHT, 3)
    c.end()
    # a daemon's 2 x 4 originals and the replies of those that complete: 14 messages
    return _scenario("timeout_handler", p, _ring(N), hi=2000, msgs=28, seed_base=11_000, max_timeouts=64)


def throw_handler() -> Scenario:
    """THROW in a forked and in an inline handler, each under catch_(ALL) and
    bare (THROW_SITES).  A handler traces, throws on odd payloads
    (THROW_CODES[payload mod 3]) and otherwise replies with the next site's
    kind.  An uncaught throw in an inline handler kills the deliverer it runs
    in; the messages after it still arrive."""
    N, rounds = 4, 5
    p = Program()
    kinds = [THROW_SITES[h][0] for h in range(4)]
    for k in kinds:
        p.kind(k)
    p.listener_set({k: f"on_{k}" for k in kinds}, inline=[THROW_SITES[h][0] for h in range(4) if THROW_SITES[h][1]])
    _main(p, N, regs=(300, rounds))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(1 + 2 * n)).listen(0)
        loop = c.here()
        c.wait_reg(0)
        c.link(2, 0).send(2, kinds[n], 1)
        c.link(3, 1).send(3, kinds[(n + 2) % 4], 1)
        c.addi(1, -1).jnei(1, 0, loop)
        c.end()
    for hid in range(4):
        kind, _inline, is_caught = THROW_SITES[hid]
        c = p.function(f"on_{kind}")
        caught = c.label()
        if is_caught:
            c.catch_(ALL, caught)
        c.trace(TAG_T + hid, 0)
        even = c.label()
        arms = [c.label() for _ in THROW_CODES]
        c.mov(2, 0).modi(2, 2).jeqi(2, 0, even)
        c.trace(TAG_THROW + hid, 0)
        c.mov(2, 0).modi(2, 3)
        for k in range(1, 3):
            c.jeqi(2, k, arms[k])
        for k, code in enumerate(THROW_CODES):
            c.bind(arms[k])
            c.throw(code, 0)
        c.bind(even)
        _reply(c, kinds[(hid + 1) % 4])
        if is_caught:
            c.uncatch()
        c.end()
        if is_caught:
            c.bind(caught)
            c.trace(TAG_CAUGHT, 3)
            c.end()
    # a daemon's 2 x 5 originals, and one reply to each of its even ones (4, 2)
    return _scenario("throw_handler", p, _ring(N), hi=2000, msgs=28, seed_base=12_000)


def rebind_handler() -> Scenario:
    """LISTEN / UNLISTEN issued from handlers.  A daemon binds its node to set 0,
    owned.  An `R` message's handler re-binds the node to the other set, owned
    on even payloads -- the handler then stays for 700 µs, and its end releases
    the node -- and not owned on odd ones.  The daemon ends at about 5 ms, as
    a former owner: some handler has bound its node since, so its death must
    release nothing.  Then its neighbour's `U` arrives (its handler calls
    `unlisten`), and the `A` sent 10 µs after it over the same link is
    undeliverable."""
    N, rounds = 4, 4
    p = Program()
    for k in ("A", "R", "U"):
        p.kind(k)
    p.listener_set({"A": "on_a0", "R": "on_r0", "U": "on_u"})
    p.listener_set({"A": "on_a1", "R": "on_r1", "U": "on_u"})
    _main(p, N, regs=(400, rounds))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(1 + 3 * n)).listen(0, owned=True)
        loop = c.here()
        c.wait_reg(0)
        c.link(2, 0).send(2, "A", 1)
        c.link(3, 1).send(3, "R", 1)
        c.addi(1, -1).jnei(1, 0, loop)
        # every R has arrived by 4 x 400 + 2050 µs; the U and the A after it
        c.wait(for_(3000))
        c.seti(1, 0)
        c.link(2, 0).send(2, "U", 1)
        c.wait(for_(10))
        c.link(2, 0).send(2, "A", 1)
        c.end()
    for s in (0, 1):
        c = p.function(f"on_a{s}")
        c.trace(TAG_T + s, 0)
        if s == 0:
            _reply(c, "A")
        c.end()
        c = p.function(f"on_r{s}")
        odd = c.label()
        c.trace(TAG_REBIND, 0)
        c.mov(2, 0).modi(2, 2).jeqi(2, 1, odd)
        c.listen(1 - s, owned=True).wait(for_(700)).end()
        c.bind(odd)
        c.listen(1 - s, owned=False).end()
    c = p.function("on_u")
    c.trace(TAG_UNLISTEN, 0).unlisten().end()
    # per node: 4 R, 4 + 2 originals from the ring's other side, and the hops of
    # the A chains (budget 4, 3, 2, 1: at most 10 hops, shared with a neighbour)
    return _scenario("rebind_handler", p, _ring(N), hi=2000, msgs=32, seed_base=13_000)


def two_owners_lp(second_outlives: bool = False) -> Scenario:
    """progs.owned_listener_two_owners under the contract: `first` and `second`
    are local forks of node 0's daemon.  `first` binds the node owned, `second`
    binds it again over that, owned too, and dies at about 200 µs -- the port
    is closed.  `first` dies at 500 µs owning nothing: its death must change
    nothing (Lane::rel_bind's non-owner path under the LP kernel, where the
    owner word is the lane's cached DW_BOWN).  main's probe, sent at 1 ms over
    its constant 50 µs link, finds no listener: undeliverable = 1, delivered =
    0.  The twin (`second_outlives`): `second` lives until 2 ms, so the probe
    is delivered.  The other daemons do the same on their nodes, unprobed."""
    N = 3
    p = Program()
    K = p.kind("msg")
    lset = p.listener_set({"msg": "on_msg"})
    c = p.function("main")
    for n in range(N):
        c.seti(2, n).fork_(f"daemon{n}", node_reg=2, scratch=3)
    c.wait(for_(1000))
    c.seti(0, 7).link(1, 0).send(1, K, 0)
    c.end()
    for n in range(N):
        p.function(f"daemon{n}").fork_("first").end()
    c = p.function("first")
    c.listen(lset, owned=True).fork_("second").wait(for_(500)).end()
    c = p.function("second")
    c.listen(lset, owned=True).wait(for_(2000 if second_outlives else 200)).end()
    c = p.function("on_msg")
    c.trace(TAG_T, 0).end()
    out = _ring(N)
    out[N] = [0]                     # the probe's link: main's only one
    name = "two_owners_lp_twin" if second_outlives else "two_owners_lp"
    topo = Topology.from_out_lists(N + 1, out)
    table = draw_table(topo.n_links, REPLICAS, np.arange(topo.n_links - 1), LO, LO + 2000, seed_base=14_000)
    assert (table[topo.n_links - 1] == LO).all()          # undrawn: the constant 50 µs
    return _scenario(name, p, out, hi=2000, msgs=1, table=table, threads_extra=8,
                     want=dict(delivered=int(second_outlives), undeliverable=int(not second_outlives)))


def raw_gate() -> Scenario:
    """`listenR`: the last listener set has a raw listener, which traces every
    message and turns away payloads that are 0 mod 3 (the thread ends); the
    typed handlers behind it reply.  Odd nodes bind that set, even nodes the
    plain one."""
    N, rounds = 4, 3
    p = Program()
    for k in ("A", "B"):
        p.kind(k)

    def raw(c, accept):
        c.trace(TAG_RAW, 0)
        c.mov(2, 0).modi(2, 3)
        c.jnei(2, 0, accept)

    p.listener_set({"A": "on_a", "B": "on_b"})
    p.listener_set({"A": "on_a", "B": "on_b"}, raw=raw)
    _main(p, N, regs=(300, rounds))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(1 + 2 * n)).listen(n % 2)
        loop = c.here()
        c.wait_reg(0)
        c.link(2, 0).send(2, "A", 1)
        c.link(3, 1).send(3, "B", 1)
        c.addi(1, -1).jnei(1, 0, loop)
        c.end()
    for hid, (k, other) in enumerate((("a", "B"), ("b", "A"))):
        c = p.function(f"on_{k}")
        c.trace(TAG_T + hid, 0)
        _reply(c, other)
        c.end()
    # a daemon's 2 x 3 originals with budgets 3, 2, 1: at most 2 x (4 + 3 + 2) = 18
    # messages, every chain shared between two nodes and cut short by the gate
    return _scenario("raw_gate", p, _ring(N), hi=2000, msgs=32, seed_base=15_000)


def kinds_sets() -> Scenario:
    """Three kinds, three listener sets over different pairs of them, node n
    bound to set n mod 3, and every daemon sends all three kinds (two per
    round, rotating).  Set 0 dispatches A inline and B forked.  A kind a set
    lacks: under set 0 (no C) it is what the assembler lowers `listen` to, a
    handler thread that finds "No listener with name" and ends
    (MonadDialog.hs:240-244), so the message counts as delivered; under sets 1
    and 2 the entry is TW_PC_NONE, the ABI's "no listener" -- the assembler
    itself never leaves one in a bound set, so these two entries are written
    into the finalized listener table here -- and the message is undeliverable
    although the node is bound."""
    N = 5
    p = Program()
    for k in ("A", "B", "C"):
        p.kind(k)
    p.listener_set({"A": "on_0a", "B": "on_0b"}, inline=["A"])
    p.listener_set({"B": "on_1b", "C": "on_1c"})
    p.listener_set({"C": "on_2c", "A": "on_2a"}, inline=["C"])
    lacks = {0: "C", 1: "A", 2: "B"}
    _main(p, N, regs=(300, 3))
    pairs = (("A", "B"), ("C", "A"), ("B", "C"))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(1 + 2 * n)).listen(n % 3)
        for i in range(3):
            a, b = pairs[(i + n) % 3]
            c.wait_reg(0)
            c.link(2, 0).send(2, a, 1)
            c.link(3, 1).send(3, b, 1)
            c.addi(1, -1)
        c.end()
    for hid, (name, other) in enumerate((("0a", "B"), ("0b", "C"), ("1b", "C"), ("1c", "A"), ("2c", "A"), ("2a", "B"))):
        c = p.function(f"on_{name}")
        c.trace(TAG_T + hid, 0)
        _reply(c, other)
        c.end()
    scn = _scenario("kinds_sets", p, _ring(N), hi=2000, msgs=32, seed_base=16_000, lacks=lacks)
    for s in (1, 2):
        scn.image.listener_pc[s, p.msg_kinds[lacks[s]]] = isa.PC_NONE
    return scn


def depth_wrap() -> Scenario:
    """`link_depth = 3` with drop bits (2^-2): a daemon sends 8 originals over
    each of its two links, so every link's ordinal wraps at least twice, and
    drops hit originals (kind O) and replies (kind R, to the originals of the
    last round) alike.  An original's payload names its link (round + 16 x link
    id) and the reply carries it back unchanged, so the oracle's terms can be
    counted per link."""
    N, rounds = 3, 8
    p = Program()
    for k in ("O", "R"):
        p.kind(k)
    p.listener_set({"O": "on_o", "R": "on_r"})
    _main(p, N, regs=(250, rounds))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(1 + 2 * n)).listen(0)
        loop = c.here()
        c.wait_reg(0)
        for k in range(2):         # payload: the round + 16 x the link's id (n's links are 2 n and 2 n + 1)
            c.mov(3, 1).addi(3, 16 * (2 * n + k))
            c.link(2, k).send(2, "O", 3)
        c.addi(1, -1).jnei(1, 0, loop)
        c.end()
    c = p.function("on_o")
    skip = c.label()
    c.trace(TAG_T, 0)
    c.mov(2, 0).modi(2, 8).jnei(2, 1, skip)
    c.reply_link(2, 1).send(2, "R", 0)
    c.bind(skip)
    c.end()
    c = p.function("on_r")
    c.trace(TAG_T + 1, 0).end()
    # per node: 16 originals in, 2 replies in, and the DROP terms of its own 16 + 2 sends
    return _scenario("depth_wrap", p, _ring(N), hi=2000, msgs=32, depth=3, drop_log2=2, seed_base=17_000,
                     sends_per_link=rounds)


def slow_handler() -> Scenario:
    """A handler that waits between a node-variable update and its reply:
    NLOAD / ADDI / NSTORE on the node's counter, `wait (payload mod 4 µs)`,
    NSTOREX / NLOADX on its own node, a fork_ of a local child that traces the
    counter its parent saw, then the reply.  A daemon sends twice over one
    link, 1 µs apart, so the second message arrives inside the first handler's
    wait; with delays of 50-55 µs the two neighbours' messages meet too, and
    the handlers of equal-time arrivals read the counter in the order of the
    tie: this program has replicas left out of the comparison."""
    N, rounds = 3, 2
    p = Program()
    p.kind("A")
    p.listener_set({"A": "on_a"})
    _main(p, N, regs=(200, rounds))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.wait(for_(10 + 25 * n)).listen(0)
        loop = c.here()
        c.wait_reg(0)
        c.link(2, 0).send(2, "A", 1)
        c.link(3, 0).send(3, "A", 1)
        c.addi(1, -1).jnei(1, 0, loop)
        c.end()
    c = p.function("on_a")                 # r2: the counter as this handler stored it
    c.nload(2, 0).addi(2, 1).nstore(2, 0)
    c.trace(TAG_STORE, 2)
    c.mov(3, 0).modi(3, 4).wait_reg(3)
    c.node(3).nstorex(2, 1, 3).nloadx(3, 1, 3).trace(TAG_XVAR, 3)
    c.fork_("child", scratch=3)
    c.trace(TAG_REPLY, 2)
    _reply(c, "A", link_reg=3)
    c.end()
    c = p.function("child")
    c.trace(TAG_CHILD, 2).end()
    # a daemon's 2 x 2 originals with budgets 2 and 1: 2 x (3 + 2) = 10 messages
    return _scenario("slow_handler", p, _ring(N), hi=5, msgs=30, seed_base=18_000, threads_per_msg=4)


def spawn_regs() -> Scenario:
    """Per-replica `main_regs`: every replica has its own period (0-7 µs) and
    rounds (1-4), which the daemons inherit through the spawn record's register
    copy.  main waits 0-2 µs between its forks, so the spawns spread over
    several ticks of the first window."""
    N = 5
    p = Program()
    p.kind("A")
    p.listener_set({"A": "on_a"})
    _main(p, N, waits=[0, 1, 2, 0, 2])
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.listen(0)
        loop = c.here()
        c.wait_reg(0)
        c.link(2, 0).send(2, "A", 1)
        c.link(3, 1).send(3, "A", 1)
        c.addi(1, -1).jnei(1, 0, loop)
        c.end()
    c = p.function("on_a")
    c.trace(TAG_T, 0)
    _reply(c, "A")
    c.end()
    g = np.random.default_rng([19, 0x72656773])
    regs = np.zeros((REPLICAS, 4), np.int64)
    regs[:, 0] = g.integers(0, 8, size=REPLICAS)
    regs[:, 1] = g.integers(1, 5, size=REPLICAS)
    # a daemon's 2 x 4 originals with budgets 4..1: 2 x (5 + 4 + 3 + 2) = 28 messages,
    # every chain shared between two nodes
    return _scenario("spawn_regs", p, _ring(N), hi=2000, msgs=32, seed_base=19_000, main_regs=regs)


def heavy_mixed() -> Scenario:
    """A heavy inbox whose due run mixes batchable and non-batchable handlers
    (tw_lp_due, classify_batch): 48 senders onto one receiver, 32 replicas,
    delays of 50-100 µs.  Every sender sends Ping, Count, waits 230 µs and
    sends Ping, Count again, so the receiver's 96 messages of the first burst
    arrive within about 150 µs: more than 32 in one window.  Its set has a pure
    `Ping` handler (trace, reply: batchable) and a `Count` handler that counts
    in a node variable (NSTORE: not batchable).  The receiver traces its
    counter and calls `unlisten` at 250 µs -- between the bursts' arrivals, so
    that no message meets the unlisten in the same microsecond -- when the
    first senders' second bursts are in flight: all of those are
    undeliverable.  Node i < 48 is sender i, node 48 the receiver, node 49
    hosts main."""
    S, rounds = 48, 4
    RECV = S
    p = Program()
    for k in ("Ping", "Count", "Pong"):
        p.kind(k)
    recv_set = p.listener_set({"Ping": "on_ping", "Count": "on_count"})
    send_set = p.listener_set({"Pong": "on_pong"})
    c = p.function("main")
    c.seti(0, RECV).fork_("receiver", node_reg=0, scratch=3)
    c.seti(0, 0).seti(2, S)
    loop = c.here()
    c.fork("sender", ref=1, node_reg=0)
    c.addi(0, 1).jlt(0, 2, loop)
    c.end()
    c = p.function("receiver")
    c.listen(recv_set)
    c.wait(for_(249))
    c.nload(2, 0).trace(TAG_COUNT, 2)
    c.unlisten()
    c.end()
    c = p.function("sender")
    c.listen(send_set)
    c.seti(1, rounds)
    for i in range(rounds):
        c.wait(for_(230 if i == 2 else 3))
        c.link(2, 0).send(2, "Ping" if i % 2 == 0 else "Count", 1)
        c.addi(1, -1)
    c.end()
    c = p.function("on_ping")
    c.trace(TAG_T, 0)
    c.reply_link(2, 1).send(2, "Pong", 0)
    c.end()
    c = p.function("on_count")
    c.nload(2, 0).addi(2, 1).nstore(2, 0)
    c.end()
    c = p.function("on_pong")
    c.trace(TAG_T + 1, 0).end()
    out = [[RECV] for _ in range(S)] + [list(range(S)), []]
    # the receiver's inbox as scenarios.hotspot sizes it: every sender's
    # messages in flight (all 4 of them) + 2, + 64
    caps = np.array([32] * S + [S * (rounds + 2) + 64, 4], np.uint32)
    return _scenario("heavy_mixed", p, out, hi=50, msgs=S * rounds, n_replicas=HEAVY_REPLICAS, seed_base=20_000,
                     inbox_cap=caps, receiver=RECV, n_senders=S)


def due_run_on_an_idle_lane() -> Scenario:
    """What heavy_mixed with TW_LP_BATCH=0 reduced to (not one of lp_programs():
    found by them).  Every daemon binds its node, sends two `Count` messages
    and ends at about 5 µs; the inboxes are heavy by their capacity (64 > 32),
    so the messages, 50 µs later, come as a due run (tw_lp_due) to a lane none
    of whose threads is left, and the handler stores a node variable, so
    tw_lp_batch leaves the run to the lane's chain.  An event kernel that stops
    a lane at `live == 0` without looking at its due run never pops these
    records: the window never completes and tw_run does not return (DESIGN.md,
    section 2, feature programs: the due run's records now count as live)."""
    N = 3
    p = Program()
    p.kind("Count")
    p.listener_set({"Count": "on_count"})
    _main(p, N, regs=(0, 1))
    for n in range(N):
        c = p.function(f"daemon{n}")
        c.listen(0)
        c.link(2, 0).send(2, "Count", 1)
        c.link(3, 1).send(3, "Count", 1)
        c.end()
    c = p.function("on_count")
    c.nload(2, 0).addi(2, 1).nstore(2, 0)
    c.trace(TAG_T, 0)
    _reply(c, "Count")
    c.end()
    # per node: 2 originals and 2 replies
    return _scenario("due_run_on_an_idle_lane", p, _ring(N), hi=2000, msgs=4, seed_base=21_000,
                     inbox_cap=np.array([64] * N + [4], np.uint32))


_BUILDERS = OrderedDict([
    ("timeout_handler", timeout_handler), ("throw_handler", throw_handler), ("rebind_handler", rebind_handler),
    ("two_owners_lp", two_owners_lp), ("two_owners_lp_twin", lambda: two_owners_lp(True)), ("raw_gate", raw_gate),
    ("kinds_sets", kinds_sets), ("depth_wrap", depth_wrap), ("slow_handler", slow_handler),
    ("spawn_regs", spawn_regs), ("heavy_mixed", heavy_mixed)])
NAMES = list(_BUILDERS)
# the programs also run under the other window modes, and the grid that makes
# their work lists grid-stride: the LP event kernel takes its grid-stride form
# only when a context has more workgroups of LP_WORKGROUP_LANES lanes (TW_WG_LP,
# csrc/engine_dev.hpp; a lane is a (node, replica) pair) than TW_LP_GRID
WINDOW_MODE_PROGRAMS = ("spawn_regs", "rebind_handler", "timeout_handler")
LP_WORKGROUP_LANES = 128
GRID_STRIDE = 1


def lp_workgroups(scn: Scenario) -> int:
    return -(-scn.n_nodes * scn.n_replicas // LP_WORKGROUP_LANES)


# the programs in which no replica may be left out of the batched-LP comparison
ALL_COMPARED = ("two_owners_lp", "two_owners_lp_twin", "raw_gate", "kinds_sets", "depth_wrap")


def lp_programs() -> "OrderedDict[str, Scenario]":
    return OrderedDict((name, build()) for name, build in _BUILDERS.items())


def program(name: str) -> Scenario:
    return due_run_on_an_idle_lane() if name == "due_run_on_an_idle_lane" else _BUILDERS[name]()


# ------------------------------------------------------------------- reach
CAPACITY_ERRORS = (isa.REP_ERR_SLOTS, isa.REP_ERR_QUEUE, isa.REP_ERR_FRAMES, isa.REP_ERR_COUNTER)


def _max_open(traces, open_tag, close):
    """The most timeouts open at once on one node: +1 at a TAG_OPEN, -1 at the
    trace that closes one; at equal times the closes count first."""
    ev = {}
    for t, node, tag, val in traces:
        if tag == open_tag:
            ev.setdefault(node, []).append((t, 1))
        elif close(tag, val):
            ev.setdefault(node, []).append((t, -1))
    best = 0
    for lst in ev.values():
        depth = 0
        for _t, d in sorted(lst):
            depth += d
            best = max(best, depth)
    return best


def _recv_inside(o):
    """slow_handler: does some node get a RECV after a handler's TAG_STORE and
    not after the same handler's TAG_REPLY (paired by node and counter value,
    in log order)?"""
    open_ = {}
    spans = []
    for t, node, tag, val in o.traces:
        if tag == TAG_STORE:
            open_.setdefault((node, val), []).append(t)
        elif tag == TAG_REPLY and open_.get((node, val)):
            spans.append((node, open_[(node, val)].pop(0), t))
    recv = [(t, node) for t, node, kind, _v in o.terms if kind >> 16 == isa.KIND_RECV >> 16]
    return any(n == node and t0 < t <= t1 for node, t0, t1 in spans for t, n in recv)


def reach(scn: Scenario, threads: int = 8) -> dict:
    """What one program reaches, from the oracle alone: the figures
    tests/test_lpprogs_oracle.py asserts and profiles/lpprogs/oracle_reach.txt
    lists.  `res`, `hashes` and `compared` are what the GPU test compares with."""
    import netsoup
    import oracle
    from timewarp.engine import lpb_lookahead, lpb_short_link_destinations

    m, R, name = scn.meta, scn.n_replicas, scn.meta["program"]
    res, h = oracle.run_batch(scn, threads=threads)
    look = lpb_lookahead(scn)
    f = dict(name=name, res=res, hashes=h, compared=netsoup.lp_compared(scn, res, h), lookahead=look,
             min_delay=int((scn.link_table & np.uint32(0x7FFFFFFF)).min()),
             short_dst=lpb_short_link_destinations(scn, look).tolist(),
             distinct=len(set(zip(res["events"].tolist(), h.sum(axis=1).tolist()))),
             max_node_msgs=0, max_traces=0, over_inbox=0, over_slots=0, runs=[])
    caps = np.broadcast_to(np.asarray(m["lp_inbox_cap"], np.int64), (scn.n_nodes,))
    x = dict(fired=0, completed=0, overlap=0, sites=set(), codes=set(), after_inline_throw=0, owned=0, not_owned=0,
             turned_away=0, accepted=0, missing_kind=0, inline_recv=0, forked_recv=0, stub_recv=0, drop_kinds=set(),
             recv_inside=0, window_peak=[], recv_kinds=set(), undeliv_after_unlisten=0, min_link_msgs=1 << 30)
    for r in range(R):
        o = oracle.run(scn, replica=r, term_cap=1 << 13, trace_cap=1 << 12)
        assert len(o.terms) < 1 << 13 and len(o.traces) < 1 << 12
        f["runs"].append(o)
        f["max_traces"] = max(f["max_traces"], len(o.traces))
        per_node = np.zeros(scn.n_nodes, np.int64)
        for _t, node, kind, _v in o.terms:
            if kind >> 16 in MSG_TERMS:
                per_node[node] += 1
        f["max_node_msgs"] = max(f["max_node_msgs"], int(per_node.max()))
        f["over_inbox"] += int((per_node > caps).sum())
        f["over_slots"] += int((m["lp_threads_per_msg"] * per_node + m["lp_threads_extra"] > m["lp_max_slots"]).sum())
        tags = [(tag, val) for _t, _n, tag, val in o.traces]
        if name == "timeout_handler":
            x["fired"] += sum(1 for tag, val in tags if tag == TAG_CAUGHT and val == TIMEOUT)
            x["completed"] += sum(1 for tag, _v in tags if tag == TAG_DONE)
            x["overlap"] += _max_open(o.traces, TAG_OPEN, lambda tag, val: tag == TAG_DONE or tag == TAG_CAUGHT) >= 2
        elif name == "throw_handler":
            x["sites"] |= {tag - TAG_THROW for tag, _v in tags if TAG_THROW <= tag < TAG_THROW + 4}
            x["codes"] |= {val for tag, val in tags if tag == TAG_CAUGHT}      # as caught: the code really raised
            bare = [(t, n) for t, n, tag, _v in o.traces if tag == TAG_THROW + 3]
            x["after_inline_throw"] += any(kind >> 16 == isa.KIND_RECV >> 16 and node == n and t > t0
                                           for t0, n in bare for t, node, kind, _v in o.terms)
        elif name == "rebind_handler":
            x["owned"] += sum(1 for tag, val in tags if tag == TAG_REBIND and val % 2 == 0)
            x["not_owned"] += sum(1 for tag, val in tags if tag == TAG_REBIND and val % 2 == 1)
        elif name == "raw_gate":
            x["turned_away"] += sum(1 for tag, val in tags if tag == TAG_RAW and val % 3 == 0)
            x["accepted"] += sum(1 for tag, val in tags if tag == TAG_RAW and val % 3 != 0)
        elif name == "kinds_sets":
            kid = {"A": 0, "B": 1, "C": 2}
            for _t, node, kind, _v in o.terms:
                if node >= m["n_daemons"]:
                    continue
                s, k = node % 3, kind & 0xFFFF
                if kind >> 16 == isa.KIND_UNDELIV >> 16:
                    assert s in (1, 2) and k == kid[m["lacks"][s]], (r, node, k)
                    x["missing_kind"] += 1
                elif kind >> 16 == isa.KIND_RECV >> 16:
                    x["stub_recv"] += s == 0 and k == kid["C"]
                    x["inline_recv"] += s == 0 and k == kid["A"]
                    x["forked_recv"] += s == 0 and k == kid["B"]
        elif name == "depth_wrap":
            x["drop_kinds"] |= {kind & 0xFFFF for _t, _n, kind, _v in o.terms if kind >> 16 == isa.KIND_DROP >> 16}
            # per link: an O term's payload names the link it went over, an R
            # term's the link it answers (it goes over that link's reverse)
            per_link = np.zeros(scn.topo.n_links, np.int64)
            for _t, _n, kind, val in o.terms:
                if kind >> 16 in MSG_TERMS:
                    l = int(val) // 16
                    per_link[l if kind & 0xFFFF == 0 else int(scn.topo.rev[l])] += 1
            x["min_link_msgs"] = min(x["min_link_msgs"], int(per_link.min()))
        elif name == "slow_handler":
            x["recv_inside"] += _recv_inside(o)
        elif name == "heavy_mixed":
            at = [t for t, node, kind, _v in o.terms
                  if node == m["receiver"] and kind >> 16 in (isa.KIND_RECV >> 16, isa.KIND_UNDELIV >> 16)]
            x["window_peak"].append(int(np.bincount(np.asarray(at) // look).max()))
            x["recv_kinds"] |= {kind & 0xFFFF for _t, node, kind, _v in o.terms
                                if node == m["receiver"] and kind >> 16 == isa.KIND_RECV >> 16}
            t_un = [t for t, _n, tag, _v in o.traces if tag == TAG_COUNT]
            x["undeliv_after_unlisten"] += any(node == m["receiver"] and kind >> 16 == isa.KIND_UNDELIV >> 16
                                               and t >= t_un[0] for t, node, kind, _v in o.terms)
    f.update(x)
    return f


def reach_report() -> str:
    out = ["batched-LP feature programs: what each reaches, from the oracle alone (python tests/lpprogs.py --reach)",
           "name                 R nodes links  compared excluded distinct  delivered dropped undeliv  max_ev "
           "node_msgs(cap) slots  figures"]
    for name, scn in lp_programs().items():
        f = reach(scn)
        res, m = f["res"], scn.meta
        skip = ("name", "res", "hashes", "compared", "runs", "lookahead", "min_delay", "short_dst", "distinct",
                "max_node_msgs", "max_traces", "over_inbox", "over_slots")
        fig = {k: (sorted(v) if isinstance(v, set) else v) for k, v in f.items()
               if k not in skip and v not in (0, [], set(), 1 << 30)}
        if "window_peak" in fig:
            fig["window_peak"] = f"{min(fig['window_peak'])}..{max(fig['window_peak'])}"
        out.append(f"{name:<20} {scn.n_replicas:2d} {scn.n_nodes:5d} {scn.topo.n_links:5d} {int(f['compared'].sum()):9d} "
                   f"{int((~f['compared']).sum()):8d} {f['distinct']:8d} {int(res['delivered'].sum()):10d} "
                   f"{int(res['dropped'].sum()):7d} {int(res['undeliverable'].sum()):7d} {int(res['events'].max()):7d} "
                   f"{f['max_node_msgs']:9d}({int(max(m['lp_inbox_cap']))}) {m['lp_max_slots']:5d}  "
                   + ", ".join(f"{k}={v}" for k, v in fig.items()))
    return "\n".join(out)


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser(description="batched-LP feature programs: reach figures, or one replica's oracle run")
    ap.add_argument("--reach", action="store_true")
    ap.add_argument("--program", default=NAMES[0], choices=NAMES + ["due_run_on_an_idle_lane"])
    ap.add_argument("--replica", type=int, default=0)
    ap.add_argument("--mode", type=int, default=0, help="oracle tie mode: 0 canonical, 2 lifo, 3 scramble, 5 forkfirst")
    a = ap.parse_args()
    if a.reach:
        print(reach_report())
    else:
        import netsoup

        print(netsoup.describe(program(a.program), a.replica, a.mode))
