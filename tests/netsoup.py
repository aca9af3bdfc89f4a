"""Random networked programs ("net soup") for differential GPU-vs-oracle tests
of the MonadDialog half of the engine: LINK / RLINK / SEND and their fused
forms, DELIVER, LISTEN (owned and not) / UNLISTEN, NLOADX / NSTOREX, forks onto
other nodes, inline (`TW_LPC_INLINE`) handlers, `link_depth` wrap-around, drop
bits, transmission time, undeliverable messages and RLINK without a reverse
link -- with every replica of a batch on its own control flow.

`net_soup(seed, n_replicas, profile, diverge)` is deterministic in `seed`.
Shared by tests/test_netsoup_oracle.py (CPU: what the seed list covers) and
tests/test_gpu_netsoup.py (GPU).  Run as a script it is the CPU-only reducer
of a GPU mismatch:

    python tests/netsoup.py --seed S --replica r [--profile lp] [--diverge table] [--mode M]

prints the program listing, the topology, that replica's link-table column
and the oracle's result, node hashes and term log.

Program shape.  `main` (on its own node) forks one daemon per node, keeps the
refs in its node variables and -- in about 60 % of the seeds -- later
killThreads one of them.  A daemon binds listener set `node mod nsets` (owned
or not), then `rounds` times waits `period` µs and sends 1-2 messages with the
loop counter as payload: the payload is the hop budget, a handler replies or
forwards only while it is > 0, which bounds the traffic.  A handler is 2-5
random pieces (HANDLER PIECES below), optionally under `catch_(ALL)`.

Handler registers (include/timewarp.h TW_OP_DELIVER): r0 payload, r1 incoming
link, r2 sender node, r3 kind; the pieces keep r0 and r1 and use r2 / r3 as
scratch."""
from __future__ import annotations

import os
import sys

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

# the committed seed list: what the CPU coverage test guards and the GPU tests run
SEEDS = list(range(16))
GPU_REPLICAS = 300       # one full 256-replica workgroup + a 44-lane tail; no multiple of 64
LP_REPLICAS = 256        # tw_lpb_load wants a power of two
# profile="lp" runs the same list but for seed 2, every replica of which depends
# on the order of equal-time events (nothing of it would be compared), plus one
LP_SEEDS = [s for s in range(17) if s != 2]

ALL = isa.MASK_ALL
TK, OVERFLOW, USER0 = isa.EXC_THREAD_KILLED, isa.EXC_ARITH, isa.EXC_USER0
KINDS = ("A", "B", "C")

TAG_T = 200              # plain handler traces: TAG_T + handler id
TAG_T2 = 300             # the second of a trace pair
TAG_CAUGHT = 400         # a catch_(ALL) handler ran: traces r3, the exception code
TAG_RAW = 401            # the raw (listenR) listener saw a message
TAG_REBIND = 402         # a handler is about to listen / unlisten on its node
TAG_XNODE = 403          # the value read back from another node's variable
TAG_THROW = 500          # TAG_THROW + handler id: the handler is about to throw

FUSED_FLAGS = ("TW_SEND_VIA_LINK", "TW_SEND_VIA_RLINK", "TW_ALU_NSTORE", "TW_TRACE_PAIR")
_ALU_NSTORE_OPS = (isa.OP_SETI, isa.OP_SETK, isa.OP_ADDI, isa.OP_MULI, isa.OP_NOW, isa.OP_NODE)


def fused_nstore_ops(insns: np.ndarray) -> set:
    """The opcodes (isa.OP_*) that occur fused with the NSTORE after them."""
    return {w & 0xFF for w in insns[:, 0].tolist() if (w & 0xFF) in _ALU_NSTORE_OPS and (w >> 16) & isa.ALU_NSTORE}


def fused_flags(insns: np.ndarray) -> set:
    """The fused-pair flags (include/timewarp.h) that occur in a finalized image."""
    out = set()
    for w in insns[:, 0].tolist():
        op, b = w & 0xFF, w >> 16
        if op == isa.OP_SEND and b & isa.SEND_VIA_LINK:
            out.add("TW_SEND_VIA_LINK")
        if op == isa.OP_SEND and b & isa.SEND_VIA_RLINK:
            out.add("TW_SEND_VIA_RLINK")
        if op in _ALU_NSTORE_OPS and b & isa.ALU_NSTORE:
            out.add("TW_ALU_NSTORE")
        if op == isa.OP_TRACE and b & isa.TRACE_PAIR:
            out.add("TW_TRACE_PAIR")
    return out


# ------------------------------------------------------------------ topology
def _topology(rng, N: int, symmetric: bool, fan_in: bool):
    """Out-lists of nodes 0..N-1 (1-3 distinct peers each) plus the main node N
    (no links).  `symmetric` adds every missing reverse link, so `link_rev` has
    no TW_PC_NONE; `fan_in` points every node's link 0 at node 0."""
    out = []
    for n in range(N):
        peers = [m for m in range(N) if m != n]
        k = int(rng.integers(1, min(3, len(peers)) + 1))
        lst = [int(x) for x in rng.choice(peers, size=k, replace=False)]
        if fan_in and n != 0:
            lst = [0] + [m for m in lst if m != 0]
        out.append(lst)
    if symmetric:
        for n in range(N):
            for m in list(out[n]):
                if n not in out[m]:
                    out[m].append(n)
    out.append([])
    return out


# ------------------------------------------------------------ handler pieces
class _Gen:
    """One seed's draws and the facts the coverage test reads back (meta)."""

    def __init__(self, rng, profile, N, nsets, min_deg):
        self.rng, self.lp, self.N, self.nsets, self.min_deg = rng, profile == "lp", N, nsets, min_deg
        self.throw_sites = {}    # TAG_THROW + hid -> dict(inline=.., caught=..)
        self.rebind_handlers = 0

    def _send_guard(self, c):
        """Reply / forward only while the hop budget lasts; the message carries budget - 1."""
        skip = c.label()
        c.jeqi(0, 0, skip).addi(0, -1)
        return skip

    def trace(self, c, hid):
        r = self.rng
        a = int(r.integers(0, 4))
        if r.random() < 0.4:       # TRACE ; TRACE, sometimes with a jump to the pair's second half
            if r.random() < 0.5:
                second = c.label()
                c.jeqi(0, 1, second).trace(TAG_T + hid, a)
                c.bind(second)
                c.trace(TAG_T2 + hid, int(r.integers(0, 4)))
            else:
                c.trace(TAG_T + hid, a).trace(TAG_T2 + hid, int(r.integers(0, 4)))
        else:
            c.trace(TAG_T + hid, a)

    def counter(self, c, hid):
        r = self.rng
        v = int(r.integers(0, 4))
        how = int(r.integers(0, 4))
        if how == 0:               # ADDI ; NSTORE
            c.nload(2, v).addi(2, 1).nstore(2, v)
        elif how == 1:             # NOW ; NSTORE
            c.now(3).nstore(3, v)
        elif how == 2:             # NODE ; NSTORE, then the counter the long way round
            c.node(2).nstore(2, v).nload(3, v).add(3, 0).nstore(3, (v + 1) % 4)
        else:                      # SETI ; NSTORE
            c.seti(2, int(r.integers(-5, 1000))).nstore(2, v)

    def reply(self, c, hid):
        r = self.rng
        skip = self._send_guard(c)
        kind = KINDS[int(r.integers(0, 3))]
        if r.random() < 0.5:
            c.reply_link(2, 1).send(2, kind, 0)            # RLINK ; SEND
        else:
            # the incoming link parked in r3 and r1 overwritten: the fused
            # SEND's register field is 3, not the usual 1
            c.mov(3, 1).now(1).reply_link(2, 3).send(2, kind, 0).mov(1, 3)
        c.bind(skip)

    def forward(self, c, hid):
        r = self.rng
        skip = self._send_guard(c)
        k = int(r.integers(0, self.min_deg))
        if not self.lp and r.random() < 0.1:
            k = int(r.integers(0, 4))      # maybe past this node's out-list: a neighbour's link, or none
        c.link(2, k).send(2, KINDS[int(r.integers(0, 3))], 0)   # LINK ; SEND
        c.bind(skip)

    def wait(self, c, hid):
        c.wait(for_(int(self.rng.integers(0, 4))))

    def throw(self, c, hid, inline, caught):
        r = self.rng
        skip = c.label()
        c.mov(2, 0).modi(2, 2).jeqi(2, int(r.integers(0, 2)), skip)
        c.trace(TAG_THROW + hid, 0)
        c.throw(int(r.choice([TK, OVERFLOW, USER0])), int(r.integers(0, 4)))
        c.bind(skip)
        self.throw_sites[TAG_THROW + hid] = dict(inline=inline, caught=caught)

    def rebind(self, c, hid, own_set):
        r = self.rng
        c.trace(TAG_REBIND, 0)
        if r.random() < 0.7:
            other = (own_set + 1 + int(r.integers(0, self.nsets - 1))) % self.nsets if self.nsets > 1 else own_set
            c.listen(other, owned=bool(r.random() < 0.5))
        else:
            c.unlisten()
        self.rebind_handlers += 1

    def timeout(self, c, hid):
        r = self.rng
        c.timeout_begin(int(r.integers(0, 5)), epoch_reg=3)
        c.wait(for_(int(r.integers(0, 5))))
        c.timeout_end()
        if self.lp:
            c.seti(3, 0)    # (the epoch number: counted per lane there, per replica by the oracle)

    def xnode(self, c, hid):
        r = self.rng
        v = int(r.integers(0, 4))
        if self.lp:
            c.node(2)                       # batched-LP contract: a node touches its own variables only
        else:
            c.mov(2, 0).modi(2, self.N)     # node `payload mod N`
        c.nstorex(0, v, 2).nloadx(3, (v + int(r.integers(0, 2))) % 4, 2).trace(TAG_XNODE, 3)

    def handler(self, c, hid, own_set, inline, pure):
        """One listener: 2-5 pieces.  `pure` handlers are the shape the batched
        delivery of tw_lpb_load admits (classify_batch): traces, a node-variable
        read, at most one send with END right after it."""
        r = self.rng
        if pure:
            for _ in range(int(r.integers(1, 3))):
                self.trace(c, hid)
            if r.random() < 0.5:
                c.nload(3, int(r.integers(0, 4))).trace(TAG_T + hid, 3)
            (self.reply if r.random() < 0.7 else self.forward)(c, hid)
            c.end()
            return
        caught = bool(r.random() < 0.5)
        if caught:
            h = c.label()
            c.catch_(ALL, h)
        names = ["trace", "counter", "reply", "forward", "wait", "throw", "rebind", "timeout", "xnode"]
        prob = np.array([0.20, 0.14, 0.15, 0.15, 0.08, 0.08, 0.06, 0.07, 0.07])
        sends, max_sends = 0, 1 if self.lp else 2
        for _ in range(int(r.integers(2, 6))):
            piece = names[int(r.choice(len(names), p=prob))]
            if piece in ("reply", "forward"):
                if sends == max_sends:
                    piece = "trace"
                else:
                    sends += 1
            if piece == "throw":
                self.throw(c, hid, inline, caught)
            elif piece == "rebind":
                self.rebind(c, hid, own_set)
            else:
                getattr(self, piece)(c, hid)
        if caught:
            c.uncatch()
        c.end()
        if caught:
            c.bind(h)
            c.trace(TAG_CAUGHT, 3)
            c.end()


# ----------------------------------------------------------------- generator
def net_soup(seed: int, n_replicas: int, profile: str = "replica", diverge: str = "regs") -> Scenario:
    """A random networked scenario.

    profile="replica": anything goes.  profile="lp": what tw_lpb_load's
    contract allows -- a symmetric topology, delays >= 50 µs (the lookahead),
    no access to another node's variables, no kill from main (a cross-node ref
    is opaque there), one send per handler; `meta` carries the per-lane
    capacities.  Every third lp seed is a fan-in: every node's link 0 points at
    node 0 and every daemon's first send goes there; every third is light: one
    round, so at most 24 messages in all and every inbox within the 32 records
    a lane drains itself (the others' inboxes take the sorted due-run path).

    diverge="regs": per-replica `main_regs` give each replica its own period
    (0-7 µs) and rounds (1-4), inherited by the daemons through the fork's
    register copy.  diverge="table": constants and no `main_regs`; the replicas
    differ by their link-table column only (the send-free prefix's condition)."""
    if profile not in ("replica", "lp") or diverge not in ("regs", "table"):
        raise ValueError("profile: 'replica' | 'lp'; diverge: 'regs' | 'table'")
    lp = profile == "lp"
    rng = np.random.default_rng([int(seed), 0x6e657473])
    N = int(rng.integers(3, 7))
    MAIN = N
    fan_in = lp and seed % 3 == 0
    light = lp and seed % 3 == 1      # one round with a budget of one hop: every inbox stays light
    symmetric = lp or bool(rng.random() < 0.7)
    out = _topology(rng, N, symmetric, fan_in)
    topo = Topology.from_out_lists(N + 1, out)
    L = topo.n_links
    min_deg = min(len(o) for o in out[:N])

    p = Program()
    for k in KINDS:
        p.kind(k)
    nsets = int(rng.integers(2, 4))
    g = _Gen(rng, profile, N, nsets, min_deg)
    use_raw = bool(rng.random() < 0.3)

    def raw_listener(c, accept):      # listenR: log, and turn away payloads that are 0 mod 3
        c.trace(TAG_RAW, 0)
        c.mov(2, 0).modi(2, 3)
        c.jnei(2, 0, accept)

    handlers = []                     # (label name, hid, set, inline, pure)
    hid = 0
    for s in range(nsets):
        n_k = int(rng.integers(1, 4))
        kinds = [KINDS[int(i)] for i in sorted(rng.choice(3, size=n_k, replace=False))]
        inline = [k for k in kinds if rng.random() < 0.35]
        lst = {}
        for k in kinds:
            name = f"h{s}{k}"
            pure = k not in inline and bool(rng.random() < (0.5 if fan_in and s == 0 else 0.2))
            handlers.append((name, hid, s, k in inline, pure))
            lst[k] = name
            hid += 1
        p.listener_set(lst, inline=inline, raw=raw_listener if (use_raw and s == nsets - 1) else None)

    # ---- main
    table_mode = diverge == "table"
    period_c, rounds_c = int(rng.integers(0, 8)), int(rng.integers(1, 5))
    if light:
        rounds_c = 1
    max_rounds = 1 if light else 4
    kill = (not lp) and bool(rng.random() < 0.6)
    c = p.function("main")
    if table_mode:
        c.seti(0, period_c).seti(1, rounds_c)
    for n in range(N):
        c.seti(2, n).fork(f"daemon{n}", ref=3, node_reg=2).nstore(3, n % 4)
        w = int(rng.integers(0, 3))
        if w:
            c.wait(for_(w))
    kill_node = None
    if kill:
        slot = int(rng.integers(0, min(4, N)))
        kill_node = max(n for n in range(N) if n % 4 == slot)
        c.wait(for_(int(rng.choice([1, 3, 8, 20, 60]))))
        c.nload(3, slot).kill_thread(3)
    c.end()

    # ---- daemons: r0 = period, r1 = rounds left (the payload), r2 / r3 = links
    owned = []
    originals = 0
    for n in range(N):
        deg = len(out[n])
        c = p.function(f"daemon{n}")
        start = int(rng.integers(1, 4))
        if table_mode:
            c.wait(for_(start))
        own = bool(rng.random() < 0.5)
        owned.append(own)
        c.listen(n % nsets, owned=own)
        c.link(2, int(rng.integers(0, deg)))
        loop = c.here()
        if table_mode:
            c.wait(for_(period_c))
        else:
            c.wait_reg(0)
        k1 = 0 if fan_in else int(rng.integers(0, deg))
        if rng.random() < 0.4:
            # the last round jumps to the SEND of the LINK ; SEND pair and
            # sends over the link r2 was left with
            second = c.label()
            c.jeqi(1, 1, second).link(2, k1)
            c.bind(second)
            c.send(2, KINDS[int(rng.integers(0, 3))], 1)
        else:
            c.link(2, k1).send(2, KINDS[int(rng.integers(0, 3))], 1)
        nsend = 1
        if rng.random() < 0.5:
            c.link(3, int(rng.integers(0, deg))).send(3, KINDS[int(rng.integers(0, 3))], 1)
            nsend = 2
        originals += max_rounds * nsend
        c.addi(1, -1).jnei(1, 0, loop)
        c.wait(for_(int(rng.choice([0, 5, 60, 3000]))))
        if rng.random() < 0.5:
            c.unlisten()
        c.end()

    for name, h_id, s, inl, pure in handlers:
        g.handler(p.function(name), h_id, s, inl, pure)

    img = p.finalize()

    # ---- link table, transmission time
    hi = int(rng.choice([0, 2, 5, 2000]))
    lo = 50 if lp else 0
    depth = int(rng.integers(1, 4))
    drop_log2 = int(rng.choice([0, 2, 3]))
    if hi == 0 and drop_log2 == 0:
        drop_log2 = 2                 # (equal delays everywhere: the drop coins are what differs)
    table = draw_table(L, n_replicas, np.arange(L), lo, lo + hi, link_depth=depth, drop_log2=drop_log2,
                       seed_base=1000 * int(seed))
    msg_bytes = link_bw = None
    if rng.random() < 0.3:
        msg_bytes = rng.integers(10, 2000, size=len(KINDS)).astype(np.uint32)
        link_bw = rng.choice(np.array([0, 1_000_000, 5_000_000, 100_000_000], np.uint64), size=L).astype(np.uint64)
    main_regs = None
    if not table_mode:
        g2 = np.random.default_rng([int(seed), 0x72656773])
        main_regs = np.zeros((n_replicas, 4), np.int64)
        main_regs[:, 0] = g2.integers(0, 8, size=n_replicas)
        main_regs[:, 1] = g2.integers(1, max_rounds + 1, size=n_replicas)

    meta = dict(config="net_soup", seed=int(seed), profile=profile, diverge=diverge, n_daemons=N, out=out,
                symmetric=symmetric, fan_in=fan_in, nsets=nsets, raw=use_raw, owned=owned, kill_node=kill_node,
                hi=hi, link_depth=depth, drop_log2=drop_log2, tx=msg_bytes is not None,
                throw_sites=g.throw_sites, rebind_handlers=g.rebind_handlers,
                inline_handlers=sum(1 for h in handlers if h[3]), pure_handlers=sum(1 for h in handlers if h[4]))
    if lp:
        # every message: an original (rounds x 1-2 sends per daemon) or one of
        # the <= rounds hops it pays for (one send per handler), so no inbox
        # ever holds more than `msgs` records; a node is light (<= 32) only
        # when the whole traffic is: the seeds with one round.  A lane's
        # threads: the daemon, and per message a deliverer, a handler and at
        # most one watchdog.
        msgs = originals * (1 + max_rounds)
        cap = 32 if msgs <= 32 else int(min(2048, 1 << int(np.ceil(np.log2(msgs)))))
        caps = np.full(N + 1, cap, np.uint32)
        caps[MAIN] = 4
        meta.update(lp_inbox_cap=caps, lp_max_slots=int(min(1024, 3 * msgs + 16)),
                    lp_queue_capacity=int(min(2048, 3 * msgs + 16)),
                    lp_outbox_cap=int((msgs + 2 * (N + 1) + 64) * n_replicas))
    return Scenario(
        name=f"net_soup{seed}_{profile}_{diverge}", image=img, topo=topo, n_replicas=n_replicas,
        main_pc=img.pc_of("main"), main_node=MAIN, link_table=table, main_regs=main_regs,
        max_slots=256, queue_capacity=4096, run_capacity=512, max_timeouts=4096, max_frames=4,
        near_horizon_us=int(rng.choice([10_000_000, 64])), msg_bytes=msg_bytes, link_bw=link_bw, meta=meta)


def reducer_command(scn: Scenario, replica: int, mode: int = 0) -> str:
    m = scn.meta
    return (f"python tests/netsoup.py --seed {m['seed']} --replica {replica} --replicas {scn.n_replicas} "
            f"--profile {m['profile']} --diverge {m['diverge']} --mode {mode}")


# ------------------------------------------------------------------ coverage
def coverage(seeds=SEEDS, n_replicas=GPU_REPLICAS, profile="replica", diverge="regs", term_replicas=None):
    """What the seed list reaches, from the oracle alone: one dict per seed.
    `term_replicas` bounds the replicas whose term and trace logs are read
    (None: all of them)."""
    import oracle

    EXC_TK = isa.KIND_EXC | TK
    rows = []
    for seed in seeds:
        scn = net_soup(seed, n_replicas, profile=profile, diverge=diverge)
        m = scn.meta
        res, h = oracle.run_batch(scn, threads=8)
        row = dict(seed=seed, scn=scn, res=res, hashes=h,
                   status={int(k): int(v) for k, v in zip(*np.unique(res["status"], return_counts=True))},
                   distinct=len(set(zip(res["events"].tolist(), h.sum(axis=1).tolist()))),
                   flags=fused_flags(scn.image.insns),
                   wraps=int((res["delivered"] + res["dropped"] + res["undeliverable"]
                              > scn.topo.n_links * scn.link_depth).sum()),
                   killed_owned=0, killed_pending=0, inline_uncaught_throw=0, rebinds=0, max_traces=0)
        for r in range(n_replicas if term_replicas is None else min(term_replicas, n_replicas)):
            o = oracle.run(scn, replica=r, term_cap=1 << 13, trace_cap=1 << 12)
            assert len(o.terms) < 1 << 13 and len(o.traces) < 1 << 12
            row["max_traces"] = max(row["max_traces"], len(o.traces))
            kn = m["kill_node"]
            if kn is not None:
                # TW_KIND_EXC terms come from delivered asynchronous exceptions
                # alone (a handler's own THROW unwinds in place, without a
                # term), and main's kill is the soup's only throwTo of
                # ThreadKilled: the term is the daemon's death.  It was still
                # alive, so it had not reached its UNLISTEN (which END follows
                # in the same step); it still held the binding it made with
                # owned = 1 unless a handler re-bound the node before
                at = [i for i, t in enumerate(o.terms) if t[1] == kn and t[2] == EXC_TK]
                rebound = at and any(t[1] == kn and t[2] == (isa.KIND_TRACE | TAG_REBIND) for t in o.terms[:at[0]])
                if at and m["owned"][kn] and not rebound:
                    row["killed_owned"] += 1
                if at and any(t[1] == kn and t[2] >> 16 == isa.KIND_UNDELIV >> 16 for t in o.terms[at[0] + 1:]):
                    row["killed_pending"] += 1
            tags = {t[2] for t in o.traces}
            if any(tag in tags and s["inline"] and not s["caught"] for tag, s in m["throw_sites"].items()):
                row["inline_uncaught_throw"] += 1
            row["rebinds"] += TAG_REBIND in tags
        if profile == "lp":
            row["excluded"] = int((~lp_compared(scn, res, h)).sum())
        rows.append(row)
    return rows


def lp_compared(scn: Scenario, res=None, hashes=None) -> np.ndarray:
    """The replicas a batched-LP run is compared on: the oracle gives identical
    fields and hashes under the canonical, LIFO, SCRAMBLE and FORKFIRST orders
    and the replica ends DONE -- the documented contract of tw_lpb_load."""
    import oracle
    from timewarp.abi import RESULT_FIELDS

    if res is None:
        res, hashes = oracle.run_batch(scn, threads=8)
    ok = res["status"] == isa.REP_DONE
    for mode in (oracle.MODE_LIFO, oracle.MODE_SCRAMBLE, oracle.MODE_FORKFIRST):
        r2, h2 = oracle.run_batch(scn, mode=mode, threads=8)
        for f in RESULT_FIELDS:
            if f != "tie_flags":
                ok &= res[f] == r2[f]
        ok &= (hashes == h2).all(axis=1)
    return ok


def coverage_report() -> str:
    out = ["net soup: what the committed seed list covers, from the oracle alone (python tests/netsoup.py --coverage)",
           f"seeds {SEEDS}; profile=lp: {LP_SEEDS}"]
    for profile, diverge, R in (("replica", "regs", GPU_REPLICAS), ("replica", "table", GPU_REPLICAS),
                                ("lp", "regs", LP_REPLICAS)):
        rows = coverage(LP_SEEDS if profile == "lp" else SEEDS, R, profile, diverge)
        hist = {}
        for row in rows:
            for k, v in row["status"].items():
                hist[_STATUS.get(k, k)] = hist.get(_STATUS.get(k, k), 0) + v
        out.append(f"\n== profile={profile} diverge={diverge}, {R} replicas per seed")
        out.append(f"status histogram: {hist}")
        out.append("seed  N  links depth hi drop tx  distinct  delivered dropped undeliv  max_ev  kill_owned kill_pending "
                   "inline_throw rebinds wraps" + ("  excluded" if profile == "lp" else "") + "  fused")
        for row in rows:
            s, m, res = row["scn"], row["scn"].meta, row["res"]
            out.append(f"{row['seed']:4d} {m['n_daemons']:2d} {s.topo.n_links:6d} {m['link_depth']:5d} {m['hi']:4d} "
                       f"{m['drop_log2']:2d} {int(m['tx']):2d} {row['distinct']:9d} {int(res['delivered'].sum()):10d} "
                       f"{int(res['dropped'].sum()):7d} {int(res['undeliverable'].sum()):7d} {int(res['events'].max()):7d} "
                       f"{row['killed_owned']:11d} {row['killed_pending']:12d} {row['inline_uncaught_throw']:12d} "
                       f"{row['rebinds']:7d} {row['wraps']:5d}"
                       + (f" {row['excluded']:9d}" if profile == "lp" else "")
                       + "  " + ",".join(sorted(f[3:] for f in row["flags"])))
        if profile == "lp":
            ex = sum(r["excluded"] for r in rows)
            out.append(f"excluded from the batched-LP comparison: {ex} of {R * len(rows)} "
                       f"({100.0 * ex / (R * len(rows)):.2f} %), at most {max(r['excluded'] for r in rows)} in one seed")
    return "\n".join(out)


# ------------------------------------------------------------------- reducer
_OPS = {v: k[3:] for k, v in vars(isa).items() if k.startswith("OP_") and k != "OP_COUNT"}
_TERM = {1: "RESUME", 2: "EXC", 3: "TRACE", 4: "RECV", 5: "DROP", 6: "UNDELIV"}
_STATUS = {v: k[4:] for k, v in vars(isa).items() if k.startswith("REP_")}


def listing(img) -> str:
    by_pc = {}
    for name, lab in img.labels.items():
        if lab.pc is not None:
            by_pc.setdefault(lab.pc, []).append(name)
    rows = []
    for pc, (w, imm) in enumerate(img.insns.tolist()):
        for name in by_pc.get(pc, []):
            rows.append(f"{name}:")
        op, a, b = w & 0xFF, (w >> 8) & 0xFF, w >> 16
        imm = imm - (1 << 32) if imm >= 1 << 31 else imm
        rows.append(f"  {pc:4d}  {_OPS.get(op, f'op{op}'):<10} a={a} b={b:#06x} imm={imm}")
    return "\n".join(rows)


def describe(scn: Scenario, replica: int, mode: int = 0, term_cap: int = 1 << 16) -> str:
    """Everything about one replica a mismatch needs, from the CPU alone."""
    import oracle

    t, m = scn.topo, scn.meta
    rows = [f"== {scn.name}: replica {replica}, oracle mode {mode}", listing(scn.image),
            f"consts: {scn.image.consts.tolist()}",
            f"listener_pc [set][kind] (bit 31: inline):\n{np.array2string(scn.image.listener_pc, formatter=dict(int=hex))}",
            "== topology (link: src -> dst, reverse link)"]
    for l, (s, d, r) in enumerate(zip(t.src_of().tolist(), t.dst.tolist(), t.rev.tolist())):
        col = scn.link_table[l, :, replica]
        ent = ", ".join(f"{int(e) & 0x7FFFFFFF}{'(drop)' if int(e) >> 31 else ''}" for e in col)
        bw = "" if scn.link_bw is None else f"  bw {int(scn.link_bw[l])} B/s"
        rows.append(f"  link {l:2d}: {s} -> {d}, rev {'none' if r == isa.PC_NONE else r}; table [{ent}]{bw}")
    if scn.msg_bytes is not None:
        rows.append(f"msg_bytes: {scn.msg_bytes.tolist()}")
    if scn.main_regs is not None:
        rows.append(f"main_regs: {scn.main_regs[replica].tolist()}")
    rows.append("meta: " + ", ".join(f"{k}={v}" for k, v in m.items() if not k.startswith("lp_") and k != "out"))
    o = oracle.run(scn, replica=replica, mode=mode, term_cap=term_cap)
    res = dict(o.result)
    rows.append(f"== oracle result: {res} ({_STATUS.get(res['status'], '?')})")
    rows.append("node hashes: " + " ".join(f"{int(h):016x}" for h in o.hashes))
    rows.append(f"== term log ({len(o.terms)} terms: t node kind val)")
    for tt, node, kind, val in o.terms:
        rows.append(f"  {tt:8d} n{node} {_TERM.get(kind >> 16, '?'):<7} {kind & 0xFFFF:5d} {val}")
    return "\n".join(rows)


def _main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="net soup reducer: one replica through the oracle, on the CPU")
    ap.add_argument("--coverage", action="store_true", help="print the seed list's coverage figures instead")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--replica", type=int, default=0)
    ap.add_argument("--replicas", type=int, default=GPU_REPLICAS, help="the batch the replica belongs to")
    ap.add_argument("--profile", default="replica", choices=["replica", "lp"])
    ap.add_argument("--diverge", default="regs", choices=["regs", "table"])
    ap.add_argument("--mode", type=int, default=0, help="oracle tie mode: 0 canonical, 1 pqueue, 2 lifo, "
                                                        "3 scramble, 5 forkfirst")
    a = ap.parse_args(argv)
    if a.coverage:
        print(coverage_report())
        return
    scn = net_soup(a.seed, max(a.replicas, a.replica + 1), profile=a.profile, diverge=a.diverge)
    print(describe(scn, a.replica, a.mode))


if __name__ == "__main__":
    _main()
