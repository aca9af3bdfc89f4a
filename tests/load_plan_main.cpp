// Stand-alone host program over csrc/load_plan.hpp (no HIP): the load's
// descriptor and argument checks, the two image classifiers, the batched
// mode's plan and the geometry choice.
// Built and run by tests/test_load_host.py with -fsanitize=address,undefined.
// With an argument, a text file:
//   `image n_insns n_sets n_kinds`, w0 imm per instruction, the listener pcs:
//       prints `cls` (classify_pcs) and `bat` (classify_batch) lines;
//   `plan n_nodes n_links n_replicas link_depth lookahead outbox_cap`, out_off,
//   link_dst, the link table, one inbox cap per node:
//       prints the check's status and lpb_plan's results.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../time-warp_amd/csrc/load_plan.hpp"

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            return 1;                                         \
        }                                                     \
    } while (0)

using tw::LoadLimits;
using tw::LoadMode;
using tw::LpbPlan;

static const LoadLimits LIM{32u, 2048u};

static tw_insn I(uint32_t op, uint32_t a = 0, uint32_t b = 0, int32_t imm = 0) {
    return tw_insn{op | (a << 8) | (b << 16), imm};
}

// ---- images
static tw_scenario_desc image(const std::vector<tw_insn>& in, const std::vector<uint32_t>& lpc, uint32_t n_kinds) {
    tw_scenario_desc s{};
    s.insns = in.data();
    s.n_insns = (uint32_t)in.size();
    s.listener_pc = lpc.data();
    s.n_msg_kinds = n_kinds;
    s.n_listener_sets = n_kinds ? (uint32_t)(lpc.size() / n_kinds) : 0u;
    return s;
}
static std::vector<uint8_t> pcs(const std::vector<tw_insn>& in, const std::vector<uint32_t>& lpc = {}) {
    const tw_scenario_desc s = image(in, lpc, lpc.empty() ? 0u : 1u);
    std::vector<uint8_t> cls;
    tw::classify_pcs(&s, cls);
    return cls;
}
// class of the handler at pc 0 as the only listener entry
static int bat0(const std::vector<tw_insn>& in, uint32_t lpc0 = 0) {
    const std::vector<uint32_t> lpc = {lpc0};
    const tw_scenario_desc s = image(in, lpc, 1);
    std::vector<uint8_t> bat;
    tw::classify_batch(&s, bat);
    return bat.size() == 1 ? bat[0] : -1;
}

static int test_classify_pcs() {
    const uint32_t alone[] = {TW_OP_THROW_TO, TW_OP_THROW, TW_OP_TMO_FIRE, TW_OP_NLOADX, TW_OP_NSTOREX};
    for (uint32_t op : alone) {
        CHECK(pcs({I(op), I(TW_OP_END)})[0] == 0);
        CHECK(pcs({I(TW_OP_SETI), I(op), I(TW_OP_END)})[0] == 0);  // reached through computation
    }
    // a step ends at each yield: what lies behind it belongs to another step
    const uint32_t yields[] = {TW_OP_END, TW_OP_WAIT_REL, TW_OP_WAIT_ABS, TW_OP_WAIT_REG, TW_OP_FORK, TW_OP_TMO_BEGIN};
    for (uint32_t op : yields) {
        const std::vector<uint8_t> c = pcs({I(TW_OP_SETI), I(op), I(TW_OP_THROW), I(TW_OP_END)});
        CHECK(c.size() == 5 && c[0] == 1 && c[1] == 1 && c[2] == 0 && c[3] == 1 && c[4] == 0);
    }
    // DELIVER: the destination node's footprint; with an inline listener anywhere, alone
    CHECK(pcs({I(TW_OP_DELIVER), I(TW_OP_END)})[0] == 2);
    CHECK(pcs({I(TW_OP_DELIVER), I(TW_OP_END)}, {1u, TW_PC_NONE})[0] == 2);  // (TW_PC_NONE is no inline entry)
    CHECK(pcs({I(TW_OP_DELIVER), I(TW_OP_END)}, {1u, 1u | TW_LPC_INLINE})[0] == 0);
    CHECK(pcs({I(TW_OP_DELIVER), I(TW_OP_THROW)})[0] == 0);  // undeliverable: the deliverer goes on
    CHECK(pcs({I(TW_OP_SETI), I(TW_OP_DELIVER), I(TW_OP_END)})[0] == 2);
    // jumps: in range, both arms of a conditional one, out of range
    CHECK(pcs({I(TW_OP_JMP, 0, 0, 2), I(TW_OP_THROW), I(TW_OP_END)})[0] == 1);
    CHECK(pcs({I(TW_OP_JEQI, 0, 0, 3), I(TW_OP_END), I(TW_OP_END), I(TW_OP_THROW)})[0] == 0);
    CHECK(pcs({I(TW_OP_JNE, 0, 0, 2), I(TW_OP_THROW), I(TW_OP_END)})[0] == 0);
    CHECK(pcs({I(TW_OP_JLT, 0, 0, 2), I(TW_OP_END), I(TW_OP_END)})[0] == 1);
    CHECK(pcs({I(TW_OP_JMP, 0, 0, 3), I(TW_OP_END), I(TW_OP_END)})[0] == 0);
    CHECK(pcs({I(TW_OP_JMP, 0, 0, -2), I(TW_OP_END)})[0] == 0);
    CHECK(pcs({I(TW_OP_JLE, 0, 0, 1000), I(TW_OP_END)})[0] == 0);
    CHECK(pcs({I(TW_OP_JMP, 0, 0, 0)})[0] == 1);  // (a loop: every pc once)
    // falling off the image; an unknown opcode
    CHECK(pcs({I(TW_OP_SETI)})[0] == 0);
    CHECK(pcs({I(TW_OP_COUNT), I(TW_OP_END)})[0] == 0);
    CHECK(pcs({I(0xFF), I(TW_OP_END)})[0] == 0);
    CHECK(pcs({I(TW_OP_SEND), I(TW_OP_END)})[0] == 1);  // (a dropped message lets the sender go on)
    CHECK(pcs({}).size() == 1);
    return 0;
}

static int test_classify_batch() {
    // bench/Network's `reply Pong`: traces, the reply link, one send, END
    CHECK(bat0({I(TW_OP_TRACE), I(TW_OP_RLINK), I(TW_OP_SEND), I(TW_OP_END)}) == 1);
    CHECK(bat0({I(TW_OP_NLOAD), I(TW_OP_ADDI), I(TW_OP_NOW), I(TW_OP_END)}) == 1);
    // the fused NSTORE writes a node variable
    CHECK(bat0({I(TW_OP_SETI, 0, TW_ALU_NSTORE), I(TW_OP_END), I(TW_OP_END)}) == 0);
    CHECK(bat0({I(TW_OP_ADDI, 0, TW_ALU_NSTORE), I(TW_OP_END), I(TW_OP_END)}) == 0);
    CHECK(bat0({I(TW_OP_NSTORE), I(TW_OP_END)}) == 0);
    // forward jumps only
    CHECK(bat0({I(TW_OP_JEQI, 0, 0, 2), I(TW_OP_END), I(TW_OP_END)}) == 1);
    CHECK(bat0({I(TW_OP_JEQI, 0, 0, 2), I(TW_OP_FORK), I(TW_OP_END)}) == 0);  // the fall-through arm
    CHECK(bat0({I(TW_OP_JEQI, 0, 0, 2), I(TW_OP_END), I(TW_OP_FORK)}) == 0);  // the taken arm
    CHECK(bat0({I(TW_OP_JMP, 0, 0, 2), I(TW_OP_FORK), I(TW_OP_END)}) == 1);   // (a JMP has one arm)
    CHECK(bat0({I(TW_OP_NOP), I(TW_OP_JMP, 0, 0, 0)}) == 0);
    CHECK(bat0({I(TW_OP_JMP, 0, 0, 0)}) == 0);
    CHECK(bat0({I(TW_OP_JNE, 0, 0, 9), I(TW_OP_END)}) == 0);
    // SEND: END right behind it, behind the VIA_LINK / VIA_RLINK form's extra word
    CHECK(bat0({I(TW_OP_SEND), I(TW_OP_NOP), I(TW_OP_END)}) == 0);
    CHECK(bat0({I(TW_OP_SEND)}) == 0);
    CHECK(bat0({I(TW_OP_SEND, 0, TW_SEND_VIA_LINK), I(TW_OP_THROW), I(TW_OP_END)}) == 1);
    CHECK(bat0({I(TW_OP_SEND, 0, TW_SEND_VIA_RLINK), I(TW_OP_THROW), I(TW_OP_END)}) == 1);
    CHECK(bat0({I(TW_OP_SEND, 0, TW_SEND_VIA_LINK), I(TW_OP_END), I(TW_OP_NOP), I(TW_OP_END)}) == 0);
    CHECK(bat0({I(TW_OP_SEND, 0, TW_SEND_VIA_LINK), I(TW_OP_END)}) == 0);
    // TRACE_PAIR skips its second word
    CHECK(bat0({I(TW_OP_TRACE, 0, TW_TRACE_PAIR), I(TW_OP_THROW), I(TW_OP_END)}) == 1);
    CHECK(bat0({I(TW_OP_TRACE), I(TW_OP_THROW), I(TW_OP_END)}) == 0);
    CHECK(bat0({I(TW_OP_TRACE, 0, TW_TRACE_PAIR), I(TW_OP_END)}) == 0);  // (continues past the image)
    // what a handler may not do; falling off the image
    const uint32_t bad[] = {TW_OP_FORK, TW_OP_WAIT_REL, TW_OP_THROW_TO, TW_OP_LISTEN, TW_OP_MYTID, TW_OP_COUNT};
    for (uint32_t op : bad) CHECK(bat0({I(op), I(TW_OP_END)}) == 0);
    CHECK(bat0({I(TW_OP_NOP)}) == 0);
    // entries that are no fork_-dispatched handler
    CHECK(bat0({I(TW_OP_END)}, TW_PC_NONE) == 0);
    CHECK(bat0({I(TW_OP_END)}, 0u | TW_LPC_INLINE) == 0);
    CHECK(bat0({I(TW_OP_END)}, 7u) == 0);
    CHECK(bat0({I(TW_OP_END)}, 0u) == 1);
    {   // two sets x two kinds: every entry on its own, a shared handler included
        const std::vector<tw_insn> in = {I(TW_OP_END), I(TW_OP_FORK), I(TW_OP_END)};
        const std::vector<uint32_t> lpc = {0u, 1u, TW_PC_NONE, 0u};
        const tw_scenario_desc s = image(in, lpc, 2);
        std::vector<uint8_t> bat;
        tw::classify_batch(&s, bat);
        CHECK(bat == (std::vector<uint8_t>{1, 0, 0, 1}));
    }
    return 0;
}

// ---- scenarios for the checks and the plan
struct Net {
    std::vector<tw_insn> in = {I(TW_OP_WAIT_REG), I(TW_OP_DELIVER), I(TW_OP_END),
                               I(TW_OP_WAIT_REG), I(TW_OP_TMO_FIRE), I(TW_OP_END), I(TW_OP_END)};
    std::vector<uint32_t> out_off, dst, rev, table;
    tw_scenario_desc s{};
    // links[k] = {from, to, delay}; sorted by `from`
    Net(uint32_t n_nodes, uint32_t n_replicas, const std::vector<std::vector<uint32_t>>& links, bool with_table = true) {
        out_off.assign(n_nodes + 1, 0);
        for (const auto& l : links) {
            ++out_off[l[0] + 1];
            dst.push_back(l[1]);
            rev.push_back(TW_PC_NONE);
            for (uint32_t r = 0; r < n_replicas && with_table; ++r) table.push_back(l[2] + (r ? 1u : 0u));
        }
        for (uint32_t n = 0; n < n_nodes; ++n) out_off[n + 1] += out_off[n];
        s.abi_version = TW_ABI_VERSION;
        s.n_replicas = n_replicas;
        s.n_nodes = n_nodes;
        s.insns = in.data();
        s.n_insns = (uint32_t)in.size();
        s.main_pc = TW_PC_USER;
        s.n_links = (uint32_t)links.size();
        s.out_off = out_off.data();
        s.link_dst = dst.data();
        s.link_rev = rev.data();
        s.link_depth = 1;
        s.link_table = with_table ? table.data() : nullptr;
        s.max_slots = 8;
        s.queue_capacity = 8;
    }
};
static LoadMode batched(int64_t lookahead, uint32_t inbox_cap, const uint32_t* caps = nullptr, uint32_t outbox = 64) {
    LoadMode m;
    m.kind = LoadMode::BATCHED;
    m.lookahead = lookahead;
    m.inbox_cap = inbox_cap;
    m.outbox_cap = outbox;
    m.node_caps = caps;
    return m;
}

static int test_checks() {
    Net ok(3, 4, {{0, 1, 1000}, {1, 2, 1000}});
    CHECK(tw::validate(&ok.s) == TW_OK);
    CHECK(tw::validate(nullptr) == TW_ERR_INVALID);
    {
        Net n(3, 4, {{0, 1, 1000}, {1, 2, 1000}});
        n.s.abi_version = TW_ABI_VERSION + 1;
        CHECK(tw::validate(&n.s) == TW_ERR_INVALID);
    }
    {
        Net n(3, 4, {{0, 1, 1000}, {1, 5, 1000}});  // a link to no node
        CHECK(tw::validate(&n.s) == TW_ERR_INVALID);
    }
    {
        Net n(3, 4, {{0, 1, 1000}});
        n.in[4] = I(TW_OP_END);  // not the watchdog's stub
        CHECK(tw::validate(&n.s) == TW_ERR_INVALID);
        n.in[4] = I(TW_OP_TMO_FIRE);
        n.s.main_pc = n.s.n_insns;
        CHECK(tw::validate(&n.s) == TW_ERR_INVALID);
        n.s.main_pc = TW_PC_USER;
        n.s.max_frames = TW_MAX_FRAMES + 1;
        CHECK(tw::validate(&n.s) == TW_ERR_INVALID);
        n.s.max_frames = TW_MAX_FRAMES;
        CHECK(tw::validate(&n.s) == TW_OK);
        n.out_off[3] = 2;  // out_off's end is not the link count
        CHECK(tw::validate(&n.s) == TW_ERR_INVALID);
    }
    // a replica load has no arguments to check
    LoadMode rep;
    CHECK(tw::load_mode_check(&ok.s, rep, LIM) == TW_OK && !rep.lp() && !rep.lpb());
    // node-partitioned: one replica, a node range inside the scenario, a light inbox
    Net one(8, 1, {{0, 1, 1000}});
    auto nodes = [&](uint32_t b, uint32_t n, int64_t L, uint32_t ib, uint32_t ob, const tw_scenario_desc* s) {
        LoadMode m;
        m.kind = LoadMode::NODES;
        m.lp_begin = b; m.lp_count = n; m.lookahead = L; m.inbox_cap = ib; m.outbox_cap = ob;
        return tw::load_mode_check(s, m, LIM);
    };
    CHECK(nodes(0, 8, 1000, 16, 64, &one.s) == TW_OK);
    CHECK(nodes(6, 2, 1, 32, 1, &one.s) == TW_OK);
    CHECK(nodes(6, 3, 1000, 16, 64, &one.s) == TW_ERR_INVALID);
    CHECK(nodes(0xFFFFFFFFu, 2, 1000, 16, 64, &one.s) == TW_ERR_INVALID);  // (begin + count in 64 bits)
    CHECK(nodes(0, 0, 1000, 16, 64, &one.s) == TW_ERR_INVALID);
    CHECK(nodes(0, 8, 0, 16, 64, &one.s) == TW_ERR_INVALID);
    CHECK(nodes(0, 8, 1000, 0, 64, &one.s) == TW_ERR_INVALID);
    CHECK(nodes(0, 8, 1000, 33, 64, &one.s) == TW_ERR_INVALID);
    CHECK(nodes(0, 8, 1000, 16, 0, &one.s) == TW_ERR_INVALID);
    CHECK(nodes(0, 3, 1000, 16, 64, &ok.s) == TW_ERR_INVALID);  // four replicas
    // batched: a power-of-two replica count of at most 2^16, lanes and inbox records in 31 bits
    for (uint32_t r : {1u, 2u, 8u, 65536u}) {
        Net n(3, 1, {{0, 1, 1000}});
        n.s.n_replicas = r;
        LoadMode m = batched(1000, 32);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        CHECK((1u << m.rep_lg) == r && m.lp_begin == 0 && m.lp_count == 3 * r && m.lp() && m.lpb());
    }
    for (uint32_t r : {3u, 6u, 70u, 65537u, 131072u, 0x80000000u, 0x80000001u, 0xFFFFFFFFu}) {
        Net n(3, 1, {{0, 1, 1000}});
        n.s.n_replicas = r;
        LoadMode m = batched(1000, 32);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_ERR_INVALID);
    }
    {
        LoadMode m = batched(1000, 32, nullptr, 1);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_ERR_INVALID);  // the outbox holds pairs
        m = batched(0, 32);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_ERR_INVALID);
        m = batched(1000, 0);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_ERR_INVALID);
        m = batched(1000, 2049);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_ERR_INVALID);
        m = batched(1000, 2048);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_OK);
        const uint32_t zero[] = {4, 0, 4}, big[] = {4, 2049, 4}, fine[] = {1, 2048, 33};
        m = batched(1000, 32, zero);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_ERR_INVALID);
        m = batched(1000, 32, big);
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_ERR_INVALID);
        m = batched(1000, 0, fine);  // (the per-node caps stand in for inbox_cap)
        CHECK(tw::load_mode_check(&ok.s, m, LIM) == TW_OK && m.cap(1) == 2048 && m.cap(2) == 33);
    }
    {
        // lanes past 31 bits: 2^15 (+ 1) nodes x 2^16 replicas; inbox records past
        // 31 bits: 2^15 - 1 nodes x 2^16 replicas with two records each
        Net n(1, 1, {});
        n.s.n_replicas = 65536;
        std::vector<uint32_t> off((1u << 15) + 2, 0);
        n.s.out_off = off.data();
        n.s.n_nodes = (1u << 15) + 1;
        LoadMode m = batched(1000, 1);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_ERR_INVALID);
        n.s.n_nodes = 1u << 15;
        m = batched(1000, 1);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_ERR_INVALID);  // 2^31 lanes
        n.s.n_nodes = (1u << 15) - 1;
        m = batched(1000, 1);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        m = batched(1000, 2);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_ERR_INVALID);
    }
    return 0;
}

static int test_lpb_plan() {
    {
        // every link as long as the lookahead (the table's other replicas: 1 µs more): one phase
        Net n(3, 4, {{0, 1, 1000}, {1, 2, 1000}, {2, 0, 5000}});
        const uint32_t caps[] = {4, 33, 2048};
        LoadMode m = batched(1000, 32, caps);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        const LpbPlan p = tw::lpb_plan(&n.s, m, LIM);
        CHECK(p.status == TW_OK && !p.has_ph1 && p.heavy_ok && m.rep_lg == 2);
        CHECK(p.phase == (std::vector<uint8_t>{0, 0, 0}));
        CHECK(p.ib_off == (std::vector<uint32_t>{0, 4, 37, 2085}));
        CHECK(p.ib_entries == (size_t)2085 * 4);
        // ... one µs more of lookahead: links 0 and 1 are short, and node 1 has both ends of one
        m.lookahead = 1001;
        CHECK(tw::lpb_plan(&n.s, m, LIM).status == TW_ERR_INVALID);
    }
    {
        // the minimum over the replicas counts: replica 0's 999 µs under the others' 1000
        Net n(2, 2, {{0, 1, 999}});
        LoadMode m = batched(1000, 8);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        const LpbPlan p = tw::lpb_plan(&n.s, m, LIM);
        CHECK(p.status == TW_OK && p.has_ph1 && !p.heavy_ok && p.phase == (std::vector<uint8_t>{0, 1}));
        CHECK(p.ib_off == (std::vector<uint32_t>{0, 8, 16}) && p.ib_entries == 32);
        // ... and the drop bit of a table entry is no delay
        n.table[0] = 1000u | 0x80000000u;
        CHECK(!tw::lpb_plan(&n.s, m, LIM).has_ph1);
    }
    {
        // a phase-1 node with a heavy inbox; at the light limit it is fine
        Net n(3, 1, {{0, 2, 0}, {1, 2, 0}});
        const uint32_t heavy[] = {4, 4, 33}, light[] = {2048, 4, 32};
        LoadMode m = batched(1000, 32, heavy);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        LpbPlan p = tw::lpb_plan(&n.s, m, LIM);
        CHECK(p.status == TW_ERR_INVALID && p.has_ph1);
        m = batched(1000, 32, light);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        p = tw::lpb_plan(&n.s, m, LIM);
        CHECK(p.status == TW_OK && p.has_ph1 && p.heavy_ok && p.phase == (std::vector<uint8_t>{0, 0, 1}));
    }
    {
        // no link table: every delay is 0 µs, every link short
        Net n(2, 1, {{0, 1, 7}}, false);
        LoadMode m = batched(1, 8);
        CHECK(tw::load_mode_check(&n.s, m, LIM) == TW_OK);
        const LpbPlan p = tw::lpb_plan(&n.s, m, LIM);
        CHECK(p.status == TW_OK && p.phase == (std::vector<uint8_t>{0, 1}));
        Net loop(2, 1, {{0, 1, 7}, {1, 0, 7}}, false);
        CHECK(tw::lpb_plan(&loop.s, m, LIM).status == TW_ERR_INVALID);
    }
    return 0;
}

static int test_pick_geometry() {
    using tw::pick_geometry;
    CHECK(pick_geometry(false, 1, 16, nullptr, true) == TW_GEO_WAVE);
    CHECK(pick_geometry(false, 4096, 16, nullptr, true) == TW_GEO_WAVE);
    CHECK(pick_geometry(false, 4097, 16, nullptr, true) == TW_GEO_NARROW);
    CHECK(pick_geometry(false, 65535, 0, nullptr, true) == TW_GEO_NARROW);
    CHECK(pick_geometry(false, 65536, 16, nullptr, true) == TW_GEO_DENSE);
    CHECK(pick_geometry(false, 65536, 0, nullptr, true) == TW_GEO_COMPACT);
    CHECK(pick_geometry(false, 4096, 0, nullptr, true) == TW_GEO_WAVE);  // (run_capacity counts for dense batches only)
    const std::pair<const char*, int> names[] = {{"dense", TW_GEO_DENSE}, {"compact", TW_GEO_COMPACT},
                                                 {"sparse", TW_GEO_SPARSE}, {"half", TW_GEO_HALF},
                                                 {"wave", TW_GEO_WAVE}, {"narrow", TW_GEO_NARROW}};
    for (const auto& n : names) {
        CHECK(pick_geometry(false, 70, 16, n.first, true) == n.second);
        CHECK(pick_geometry(false, 1u << 20, 0, n.first, true) == n.second);
        CHECK(pick_geometry(true, 70, 0, n.first, true) == TW_GEO_DENSE);  // LP ignores the name
    }
    for (const char* n : {"", "Dense", "densest", "lpb", "lp"}) {
        CHECK(pick_geometry(false, 70, 16, n, true) == TW_GEO_WAVE);
        CHECK(pick_geometry(false, 1u << 20, 16, n, true) == TW_GEO_DENSE);
    }
    CHECK(pick_geometry(true, 1u << 20, 0, nullptr, true) == TW_GEO_DENSE);
    // an image too large for the sparse geometry's LDS: dense
    CHECK(pick_geometry(false, 70, 16, "sparse", false) == TW_GEO_DENSE);
    CHECK(pick_geometry(false, 70, 16, "narrow", false) == TW_GEO_NARROW);
    CHECK(pick_geometry(false, 70, 16, nullptr, false) == TW_GEO_WAVE);
    return 0;
}

// ---- files
static int image_file(FILE* f) {
    unsigned n = 0, ns = 0, nk = 0;
    CHECK(fscanf(f, "%u %u %u", &n, &ns, &nk) == 3);
    std::vector<tw_insn> in(n);
    for (unsigned i = 0; i < n; ++i) {
        unsigned w0 = 0;
        int imm = 0;
        CHECK(fscanf(f, "%u %d", &w0, &imm) == 2);
        in[i] = tw_insn{w0, imm};
    }
    std::vector<uint32_t> lpc((size_t)ns * nk);
    for (uint32_t& x : lpc) CHECK(fscanf(f, "%" SCNu32, &x) == 1);
    tw_scenario_desc s = image(in, lpc, nk);
    s.n_listener_sets = ns;
    std::vector<uint8_t> cls, bat;
    tw::classify_pcs(&s, cls);
    tw::classify_batch(&s, bat);
    printf("cls");
    for (uint8_t x : cls) printf(" %u", x);
    printf("\nbat");
    for (uint8_t x : bat) printf(" %u", x);
    printf("\n");
    return 0;
}

static int plan_file(FILE* f) {
    unsigned nn = 0, nl = 0, nr = 0, depth = 0, outbox = 0;
    long long L = 0;
    CHECK(fscanf(f, "%u %u %u %u %lld %u", &nn, &nl, &nr, &depth, &L, &outbox) == 6);
    Net n(1, 1, {});
    std::vector<uint32_t> off(nn + 1), dst(nl), rev(nl, TW_PC_NONE), tab((size_t)nl * depth * nr), caps(nn);
    for (uint32_t& x : off) CHECK(fscanf(f, "%" SCNu32, &x) == 1);
    for (uint32_t& x : dst) CHECK(fscanf(f, "%" SCNu32, &x) == 1);
    for (uint32_t& x : tab) CHECK(fscanf(f, "%" SCNu32, &x) == 1);
    for (uint32_t& x : caps) CHECK(fscanf(f, "%" SCNu32, &x) == 1);
    n.s.n_nodes = nn; n.s.n_links = nl; n.s.n_replicas = nr; n.s.link_depth = depth;
    n.s.out_off = off.data(); n.s.link_dst = dst.data(); n.s.link_rev = rev.data(); n.s.link_table = tab.data();
    LoadMode m = batched(L, 0, caps.data(), outbox);
    int rc = tw::validate(&n.s);
    if (!rc) rc = tw::load_mode_check(&n.s, m, LIM);
    printf("check %d\n", rc);
    if (rc) return 0;
    const LpbPlan p = tw::lpb_plan(&n.s, m, LIM);
    printf("status %d rep_lg %u has_ph1 %d heavy_ok %d ib_entries %zu\nphase1", p.status, m.rep_lg, (int)p.has_ph1,
           (int)p.heavy_ok, p.ib_entries);
    for (uint32_t i = 0; i < nn; ++i)
        if (p.phase[i]) printf(" %u", i);
    printf("\nib_off");
    for (uint32_t x : p.ib_off) printf(" %u", x);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        CHECK(f);
        char kind[16] = {0};
        CHECK(fscanf(f, "%15s", kind) == 1);
        const int rc = !strcmp(kind, "image") ? image_file(f) : !strcmp(kind, "plan") ? plan_file(f) : 1;
        fclose(f);
        return rc;
    }
    if (test_classify_pcs() || test_classify_batch() || test_checks() || test_lpb_plan() || test_pick_geometry()) return 1;
    printf("load plan ok\n");
    return 0;
}
