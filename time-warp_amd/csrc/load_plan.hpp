// load_plan.hpp — the host logic of tw_load / tw_lp_load / tw_lpb_load that
// needs no device (engine.hip's load stages): the descriptor and
// argument checks, the batch classes of the image's pcs (the wave kernel) and
// of its handlers (tw_lp_due), the batched mode's phases and inbox offsets,
// and the choice of the kernel geometry.  Kept free of HIP so it compiles
// into a plain host program (tests/load_plan_main.cpp, run under ASan /
// UBSan).  The device's limits come in as arguments (LoadLimits: tw_dev.hpp's
// TW_LIGHT and TW_HEAVY_CAP; the LDS limit as pick_geometry's sparse_fits).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/timewarp.h"

namespace tw {

inline int validate(const tw_scenario_desc* s) {
    if (!s || s->abi_version != TW_ABI_VERSION) return TW_ERR_INVALID;
    if (s->n_replicas == 0 || s->n_nodes == 0 || !s->insns || s->n_insns < TW_PC_USER || s->n_insns > 0xFFFF)
        return TW_ERR_INVALID;
    if (s->max_slots < 1 || s->queue_capacity < 1 || s->link_depth < 1 || !s->out_off) return TW_ERR_INVALID;
    if (s->max_frames > TW_MAX_FRAMES) return TW_ERR_INVALID;
    if (s->main_pc >= s->n_insns || s->main_node >= s->n_nodes || s->max_timeouts > 65536) return TW_ERR_INVALID;
    if (s->n_links && (!s->link_dst || !s->link_rev)) return TW_ERR_INVALID;
    if (s->n_listener_sets && (!s->listener_pc || !s->n_msg_kinds)) return TW_ERR_INVALID;
    // fixed stubs
    const uint32_t stub_ops[6] = {TW_OP_WAIT_REG, TW_OP_DELIVER, TW_OP_END, TW_OP_WAIT_REG, TW_OP_TMO_FIRE, TW_OP_END};
    for (int i = 0; i < 6; ++i)
        if ((s->insns[i].w0 & 0xFF) != stub_ops[i]) return TW_ERR_INVALID;
    for (uint32_t l = 0; l < s->n_links; ++l)
        if (s->link_dst[l] >= s->n_nodes) return TW_ERR_INVALID;
    if (s->out_off[s->n_nodes] != s->n_links) return TW_ERR_INVALID;
    return TW_OK;
}

// Batch class of every resume pc for the wave kernel (wave.hip PC_*): what the
// code a thread runs from that pc until its next yield may touch.
//   1 (LOCAL)   its own record, its own node's vars / binding / out-links, and
//               forks (whose records and queue entries the batch commit writes);
//   2 (DELIVER) LOCAL plus the destination node of a delivery (the deliverer stub);
//   0 (ALONE)   anything that can reach another thread or another node's state
//               (throwTo, throw, the watchdog's fire, cross-node vars, in-place
//               handlers): such an event runs as a batch of one.
// Events in one batch have equal timestamps, consecutive seqs and disjoint node
// footprints, so running them side by side commits the same effects as
// TimedT's one-at-a-time loop (TimedT.hs:239-263).  (Sends go over the sender's
// own out-links, as every lowered scenario's LINK / RLINK links do.)
inline void classify_pcs(const tw_scenario_desc* s, std::vector<uint8_t>& cls) {
    const uint32_t n = s->n_insns;
    cls.assign((size_t)n + 1, 0);
    bool inline_any = false;
    for (size_t i = 0; i < (size_t)s->n_listener_sets * s->n_msg_kinds; ++i)
        if (s->listener_pc[i] != TW_PC_NONE && (s->listener_pc[i] & TW_LPC_INLINE)) inline_any = true;
    std::vector<uint32_t> seen(n, 0xFFFFFFFFu), stk;
    for (uint32_t p0 = 0; p0 < n; ++p0) {
        bool alone = false, dlv = false;
        stk.assign(1, p0);
        seen[p0] = p0;
        while (!stk.empty() && !alone) {
            const uint32_t q = stk.back();
            stk.pop_back();
            const uint32_t op = s->insns[q].w0 & 0xFFu;
            const uint32_t imm = (uint32_t)s->insns[q].imm;
            uint32_t nx[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
            switch (op) {
            case TW_OP_THROW_TO: case TW_OP_THROW: case TW_OP_TMO_FIRE: case TW_OP_NLOADX: case TW_OP_NSTOREX:
                alone = true;
                break;
            case TW_OP_END: case TW_OP_WAIT_REL: case TW_OP_WAIT_ABS: case TW_OP_WAIT_REG: case TW_OP_FORK:
            case TW_OP_TMO_BEGIN:
                break;  // the step ends here
            case TW_OP_DELIVER:
                if (inline_any) alone = true;
                dlv = true;
                nx[0] = q + 1;  // undeliverable: the deliverer goes on
                break;
            case TW_OP_JMP:
                nx[0] = imm;
                break;
            case TW_OP_JEQ: case TW_OP_JNE: case TW_OP_JLT: case TW_OP_JLE: case TW_OP_JEQI: case TW_OP_JNEI:
                nx[0] = imm;
                nx[1] = q + 1;
                break;
            default:
                if (op >= TW_OP_COUNT) alone = true;
                nx[0] = q + 1;  // (SEND: a dropped message lets the sender go on)
                break;
            }
            for (uint32_t x : nx) {
                if (x == 0xFFFFFFFFu) continue;
                if (x >= n) { alone = true; break; }
                if (seen[x] != p0) { seen[x] = p0; stk.push_back(x); }
            }
        }
        cls[p0] = alone ? 0 : dlv ? 2 : 1;
    }
}

// The handlers a heavy lane's due run may execute data-parallel (tw_lp_due,
// round 5): the fork_-dispatched handler of a (listener set, kind) whose code,
// on every path from its entry, touches only its own registers, reads its
// node's variables, computes out-links and reply links, traces, and sends at
// most once with END right after the send -- bench/Network's Ping handler
// `reply Pong` (Receiver/Main.hs:32-38; ForkStrategy fork_, MonadDialog.hs:317).
// Such a handler's effects are its own (hash terms, counters, one record), so
// records whose events no other event of the lane interleaves with can run one
// per thread with the totals of the sequential loop.  Forward jumps only (the
// walk is bounded by the image); no NSTORE, fork, wait, throw, listen or MYTID.
inline void classify_batch(const tw_scenario_desc* s, std::vector<uint8_t>& bat) {
    const uint32_t n = s->n_insns, nk = s->n_msg_kinds;
    bat.assign((size_t)s->n_listener_sets * nk, 0);
    auto op_at = [&](uint32_t q) { return q < n ? s->insns[q].w0 & 0xFFu : 0xFFu; };
    std::vector<uint32_t> seen(n, 0xFFFFFFFFu), stk;
    for (size_t e = 0; e < bat.size(); ++e) {
        const uint32_t lpc = s->listener_pc[e];
        if (lpc == TW_PC_NONE || (lpc & TW_LPC_INLINE) || lpc >= n) continue;
        bool ok = true;
        stk.assign(1, lpc);
        seen[lpc] = (uint32_t)e;
        while (!stk.empty() && ok) {
            const uint32_t q = stk.back();
            stk.pop_back();
            const uint32_t w = s->insns[q].w0, op = w & 0xFFu, b = w >> 16;
            const uint32_t imm = (uint32_t)s->insns[q].imm;
            uint32_t nx[2] = {q + 1, 0xFFFFFFFFu};
            switch (op) {
            case TW_OP_END: nx[0] = 0xFFFFFFFFu; break;
            case TW_OP_NOP: case TW_OP_MOV: case TW_OP_ADD: case TW_OP_SUB: case TW_OP_NLOAD: case TW_OP_LINK:
            case TW_OP_RLINK:
                break;
            case TW_OP_SETI: case TW_OP_SETK: case TW_OP_ADDI: case TW_OP_MULI: case TW_OP_NOW: case TW_OP_NODE:
                ok = !(b & TW_ALU_NSTORE);  // (the fused NSTORE writes a node variable)
                break;
            case TW_OP_TRACE:
                if (b & TW_TRACE_PAIR) nx[0] = q + 2;
                break;
            case TW_OP_JMP: case TW_OP_JEQ: case TW_OP_JNE: case TW_OP_JLT: case TW_OP_JLE: case TW_OP_JEQI:
            case TW_OP_JNEI:
                ok = imm > q && imm < n;
                nx[0] = imm;
                nx[1] = op == TW_OP_JMP ? 0xFFFFFFFFu : q + 1;
                break;
            case TW_OP_SEND: {
                // the send yields 1 µs (it forks the deliverer): the thread must end there
                const uint32_t k = (b & (TW_SEND_VIA_LINK | TW_SEND_VIA_RLINK)) ? q + 2 : q + 1;
                ok = op_at(k) == TW_OP_END;
                nx[0] = 0xFFFFFFFFu;
                break;
            }
            default: ok = false; break;
            }
            for (uint32_t x : nx) {
                if (x == 0xFFFFFFFFu || !ok) continue;
                if (x >= n) { ok = false; break; }
                if (seen[x] != (uint32_t)e) { seen[x] = (uint32_t)e; stk.push_back(x); }
            }
        }
        bat[e] = ok ? 1 : 0;
    }
}

// The device's inbox limits (tw_dev.hpp: TW_LIGHT, TW_HEAVY_CAP)
struct LoadLimits {
    uint32_t light;      // a lane with at most this many pending records drains them in the event kernel
    uint32_t heavy_cap;  // largest per-node inbox
};

// What is loaded: replicas (tw_load), a range of one scenario's nodes as lanes
// (tw_lp_load), or every replica's nodes as lanes (tw_lpb_load).  The other
// fields are the two LP loads' arguments; a replica load leaves them 0.
struct LoadMode {
    enum Kind { REPLICAS, NODES, BATCHED } kind = REPLICAS;
    uint32_t lp_begin = 0, lp_count = 0;  // the lanes' node range (BATCHED: set by load_mode_check)
    int64_t lookahead = 0;
    uint32_t inbox_cap = 0, outbox_cap = 0;
    const uint32_t* node_caps = nullptr;  // BATCHED: inbox records per node, or null: inbox_cap for each
    uint32_t rep_lg = 0;                  // BATCHED: log2 of the replica count (set by load_mode_check)

    bool lp() const { return kind != REPLICAS; }
    bool lpb() const { return kind == BATCHED; }
    uint32_t cap(uint32_t node) const { return node_caps ? node_caps[node] : inbox_cap; }
};

// The arguments of an LP load against a valid descriptor; BATCHED: also
// derives rep_lg and the lane range.
inline int load_mode_check(const tw_scenario_desc* s, LoadMode& m, const LoadLimits& lim) {
    if (m.lpb()) {
        // every replica's nodes as lanes (node-major): a power-of-two replica count
        uint32_t rep_lg = 0;
        while (rep_lg <= 16 && (1u << rep_lg) < s->n_replicas) ++rep_lg;
        if (rep_lg > 16 || (1u << rep_lg) != s->n_replicas || (uint64_t)s->n_nodes << rep_lg > 0x7FFFFFFFull ||
            m.outbox_cap < 2 || m.lookahead < 1)
            return TW_ERR_INVALID;
        uint64_t tot = 0;
        for (uint32_t n = 0; n < s->n_nodes; ++n) {
            const uint32_t k = m.cap(n);
            if (k == 0 || k > lim.heavy_cap) return TW_ERR_INVALID;
            tot += k;
        }
        if ((tot << rep_lg) > 0x7FFFFFFFull) return TW_ERR_INVALID;  // (a lane's inbox base: 31 bits, DW_IB)
        m.rep_lg = rep_lg;
        m.lp_begin = 0;
        m.lp_count = s->n_nodes << rep_lg;
    } else if (m.lp() && (s->n_replicas != 1 || m.lp_count == 0 || (uint64_t)m.lp_begin + m.lp_count > s->n_nodes ||
                          m.inbox_cap == 0 || m.inbox_cap > lim.light || m.outbox_cap == 0 || m.lookahead < 1)) {
        return TW_ERR_INVALID;
    }
    return TW_OK;
}

// The batched mode's plan of a checked load: which nodes run in phase 1 of
// every window, the nodes' inbox regions, whether tw_lp_due has work.
struct LpbPlan {
    int status = TW_OK;            // TW_ERR_INVALID: the windows would need a third phase, or a phase-1 inbox is heavy
    std::vector<uint8_t> phase;    // [n_nodes] 1: the node runs in phase 1
    bool has_ph1 = false;
    std::vector<uint32_t> ib_off;  // [n_nodes + 1] prefix sums of the nodes' inbox caps
    bool heavy_ok = false;         // some node's inbox can exceed the light limit
    size_t ib_entries = 0;         // inbox records of one buffer, every replica's
};

inline LpbPlan lpb_plan(const tw_scenario_desc* s, const LoadMode& m, const LoadLimits& lim) {
    LpbPlan p;
    // two-phase windows: a link shorter than the lookahead (over every
    // replica and ordinal) must run from a phase-0 node into a node that
    // then runs in phase 1 (after phase 0 has finished the window), and such
    // a node's inbox must be light (drained at phase 1's first tick)
    p.phase.assign(s->n_nodes, 0);
    std::vector<uint8_t> shortl(s->n_links, 0);
    for (uint32_t l = 0; l < s->n_links; ++l) {
        uint32_t dmin = 0;
        if (s->link_table) {
            dmin = 0x7FFFFFFFu;
            const uint32_t* e = s->link_table + (size_t)l * s->link_depth * s->n_replicas;
            for (size_t i = 0; i < (size_t)s->link_depth * s->n_replicas; ++i) {
                const uint32_t v = e[i] & 0x7FFFFFFFu;
                dmin = v < dmin ? v : dmin;
            }
        }
        if ((int64_t)dmin < m.lookahead) {
            shortl[l] = 1;
            p.phase[s->link_dst[l]] = 1;
        }
    }
    for (uint32_t n = 0; n < s->n_nodes; ++n)
        for (uint32_t l = s->out_off[n]; l < s->out_off[n + 1]; ++l)
            if (shortl[l] && p.phase[n]) p.status = TW_ERR_INVALID;
    for (uint32_t n = 0; n < s->n_nodes; ++n) {
        if (!p.phase[n]) continue;
        p.has_ph1 = true;
        if (m.cap(n) > lim.light) p.status = TW_ERR_INVALID;
    }
    p.ib_off.resize((size_t)s->n_nodes + 1);
    p.ib_off[0] = 0;
    for (uint32_t n = 0; n < s->n_nodes; ++n) {
        const uint32_t k = m.cap(n);
        p.ib_off[n + 1] = p.ib_off[n] + k;
        if (k > lim.light) p.heavy_ok = true;
    }
    p.ib_entries = (size_t)p.ib_off[s->n_nodes] << m.rep_lg;
    return p;
}

// geometry by replica count (the name in TW_GEOMETRY overrides; LP mode is
// dense, whatever the name): <= 4096: a wavefront per replica (C5: 0.32 G
// events/s vs 0.25 sparse, 0.20 narrow); < 65536: narrow (C3 at 8192: 2.5 vs
// 0.99 sparse, 0.74 wave); else dense (one workgroup of 256 per CU).
// sparse_fits: the image fits into LDS beside the sparse geometry's queue.
inline int pick_geometry(bool lp, size_t R, uint32_t run_capacity, const char* name, bool sparse_fits) {
    // dense batches of a scenario without far runs (run_capacity 0, e.g.
    // C2's ping-pong: every event within the near horizon) take the
    // compact geometry: two waves per SIMD
    int geo = lp ? TW_GEO_DENSE : R <= 4096 ? TW_GEO_WAVE : R < 65536 ? TW_GEO_NARROW
                                : run_capacity == 0 ? TW_GEO_COMPACT : TW_GEO_DENSE;
    const std::pair<const char*, int> names[] = {{"dense", TW_GEO_DENSE}, {"compact", TW_GEO_COMPACT},
                                                 {"sparse", TW_GEO_SPARSE}, {"half", TW_GEO_HALF},
                                                 {"wave", TW_GEO_WAVE}, {"narrow", TW_GEO_NARROW}};
    for (const auto& n : names)
        if (name && !lp && !strcmp(name, n.first)) geo = n.second;
    if (geo == TW_GEO_SPARSE && !sparse_fits) geo = TW_GEO_DENSE;
    return geo;
}

}  // namespace tw
