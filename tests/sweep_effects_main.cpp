// Stand-alone host program over csrc/prefix_clean.hpp (no HIP): the effects
// table beside the kill table.  Built and run by
// tests/test_sweep_effects_host.py with -fsanitize=address,undefined.
// With arguments `image.txt n`: a program image as text (`n_insns n_consts`,
// then w0 imm per instruction, then the constants), classified here; a parked
// state of n + 1 kill wakes with two victims each is laid out around its kill
// stub and sweep time, and the effects table's counts are printed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../time-warp_amd/csrc/prefix_clean.hpp"

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            return 1;                                         \
        }                                                     \
    } while (0)

using namespace tw;

namespace {

constexpr int64_t T = 120000000;
constexpr uint32_t ST = PCL_F_STARTED, MAIN = PCL_F_MAIN, OWNS = PCL_F_OWNS;
constexpr uint32_t KILLED = 1u << PCL_EXC_THREAD_KILLED;  // a frame mask's bit

// a parked replica's records and run entries, and the directory over them
struct Parked {
    CleanLayout L{0x10000ull, 0x900000ull, 4, 0, 16, 8, 4, 8, 4};
    std::map<uint64_t, std::vector<uint32_t>> q;  // 16-byte rows by address
    uint64_t rh[4] = {0, 0, 0, 0}, rn[4] = {0, 0, 0, 0};
    std::vector<PrefixRow> rows;
    std::vector<uint8_t> snap;

    explicit Parked(uint32_t S = 16, uint32_t Cr = 8) {
        L.S = S;
        L.Cr = Cr;
        L.RQ = (uint64_t)S * L.R;
    }
    uint64_t rec_addr(uint32_t slot, uint32_t qd) const { return L.slots + ((uint64_t)qd * L.RQ + (uint64_t)slot * L.R) * 16u; }
    uint64_t run_addr(uint32_t j, uint32_t pos) const { return L.runs + (((uint64_t)j * L.Cr + pos) * L.R) * 16u; }
    static uint32_t w0(uint32_t pc, uint32_t flags, uint32_t frames = 0, uint32_t exc = 0) {
        return pc | (frames << 16) | (flags << PCL_FL_SHIFT) | (exc << PCL_EXC_SHIFT);
    }
    static uint64_t ref(uint32_t slot, uint32_t tid) { return ((uint64_t)tid << 32) | slot; }
    // m0, m1: the masks of its frames (quad 1's first two words, upper halves)
    void thread(uint32_t slot, uint32_t w0v, uint32_t node, uint32_t tid, uint32_t seq, uint64_t r1 = 0, uint64_t r2 = 0,
                uint32_t m0 = 0, uint32_t m1 = 0) {
        q[rec_addr(slot, 0)] = {w0v, node, tid, seq};
        q[rec_addr(slot, 1)] = {(m0 << 16) | 7u, (m1 << 16) | 9u, 0, 0};
        q[rec_addr(slot, 2)] = {0, 0, (uint32_t)r1, (uint32_t)(r1 >> 32)};  // r0, r1
        q[rec_addr(slot, 3)] = {(uint32_t)r2, (uint32_t)(r2 >> 32), 0, 0};  // r2, r3
    }
    void entry(uint32_t j, uint32_t pos, int64_t t, uint32_t slot, uint32_t seq) {
        q[run_addr(j, pos)] = {(uint32_t)t, (uint32_t)((uint64_t)t >> 32), slot, seq};
    }
    void finish() {
        rows.clear();
        snap.clear();
        rows.push_back(PrefixRow{0x100ull, 0u, 8u});
        snap.resize(8, 0xAB);
        for (auto& kv : q) {
            while (snap.size() % 16) snap.push_back(0);
            rows.push_back(PrefixRow{kv.first, (uint32_t)snap.size(), 16u});
            const uint8_t* b = (const uint8_t*)kv.second.data();
            snap.insert(snap.end(), b, b + 16);
        }
    }
    CleanPlan plan;
    CleanEffects build(const uint32_t* stub, int64_t t = T) {
        finish();
        plan = clean_build(L, rows.data(), rows.size(), snap.data(), snap.size(), rh, rn, stub, t);
        return clean_effects(L, rows.data(), rows.size(), snap.data(), snap.size(), stub, plan);
    }
};

// stub words by pc (n_insns = 8): 1: two throwTos r1, r2; 2: one throwTo r1
const uint32_t STUB[9] = {0, SWB_VALID | SWB_TWO | (1u << 2) | (2u << 4), SWB_VALID | (1u << 2), 0, 0, 0, 0, 0, 0};

uint32_t nadd(const EffEnt& e) { return (e.flags >> EFF_NADD_SHIFT) & 15u; }
uint32_t nrel(const EffEnt& e) { return (e.flags >> EFF_NREL_SHIFT) & 15u; }

int hand_made() {
    {   // two refs and one; killer and victims on one node, on two and on three
        Parked p;
        p.thread(3, Parked::w0(1, 0), 1, 10, 5, Parked::ref(4, 11), Parked::ref(5, 12));    // all on node 1
        p.thread(4, Parked::w0(4, ST), 1, 11, 6);
        p.thread(5, Parked::w0(5, ST, 1), 1, 12, 7, 0, 0, 1u << 5);                          // a frame for another code
        p.thread(6, Parked::w0(2, 0), 2, 13, 8, Parked::ref(7, 14));                         // one ref, on node 3
        p.thread(7, Parked::w0(4, ST, 2), 3, 14, 9, 0, 0, 1u << 5, 1u << 6);
        p.thread(8, Parked::w0(1, 0), 0, 15, 20, Parked::ref(9, 16), Parked::ref(10, 17));   // both victims on node 2
        p.thread(9, Parked::w0(4, ST), 2, 16, 21);
        p.thread(10, Parked::w0(4, ST), 2, 17, 22);
        p.thread(11, Parked::w0(1, 0), 0, 18, 23, Parked::ref(12, 19), Parked::ref(13, 20)); // nodes 0, 0, 3
        p.thread(12, Parked::w0(4, ST), 0, 19, 24);
        p.thread(13, Parked::w0(4, ST), 3, 20, 25);
        p.thread(14, Parked::w0(1, 0), 0, 21, 26, Parked::ref(15, 22), Parked::ref(1, 23));  // nodes 0, 1, 2
        p.thread(15, Parked::w0(4, ST), 1, 22, 27);
        p.thread(1, Parked::w0(4, ST), 2, 23, 28);
        p.rh[0] = 2; p.rn[0] = 5;
        p.entry(0, 2, T, 3, 5);
        p.entry(0, 3, T, 6, 8);
        p.entry(0, 4, T, 8, 20);
        p.entry(0, 5, T, 11, 23);
        p.entry(0, 6, T, 14, 26);
        const CleanEffects fx = p.build(STUB);
        CHECK(p.plan.claimable == 5 && fx.eff.size() == 5 && fx.exclusive);
        const EffEnt& a = fx.eff[0];
        CHECK((a.flags & EFF_VERDICT) && (a.flags & EFF_EXCL) && nadd(a) == 1 && nrel(a) == 0);
        CHECK(a.pc == 1 && a.add_node[0] == 1 && a.add_kills[0] == 2);
        CHECK(a.slot[0] == 3 && a.slot[1] == 4 && a.slot[2] == 5);
        CHECK(a.w0[0] == Parked::w0(1, 0) && a.w0[1] == Parked::w0(4, ST) && a.w0[2] == Parked::w0(5, ST, 1));
        CHECK(a.w1[0] == 1 && a.w1[1] == 1 && a.w1[2] == 1);
        const EffEnt& b = fx.eff[1];
        CHECK((b.flags & EFF_VERDICT) && (b.flags & EFF_EXCL) && nadd(b) == 2 && b.pc == 2);
        CHECK(b.add_node[0] == 2 && b.add_kills[0] == 0 && b.add_node[1] == 3 && b.add_kills[1] == 1);
        CHECK(b.slot[0] == 6 && b.slot[1] == 7 && b.slot[2] == 0 && b.w1[1] == 3 && b.w0[2] == 0);
        const EffEnt& c = fx.eff[2];
        CHECK(nadd(c) == 2 && c.add_node[0] == 0 && c.add_kills[0] == 0 && c.add_node[1] == 2 && c.add_kills[1] == 2);
        const EffEnt& d = fx.eff[3];
        CHECK(nadd(d) == 2 && d.add_node[0] == 0 && d.add_kills[0] == 1 && d.add_node[1] == 3 && d.add_kills[1] == 1);
        const EffEnt& e = fx.eff[4];
        CHECK(nadd(e) == 3 && e.add_node[0] == 0 && e.add_kills[0] == 0 && e.add_node[1] == 1 && e.add_kills[1] == 1 &&
              e.add_node[2] == 2 && e.add_kills[2] == 1);
        for (const EffEnt& x : fx.eff) CHECK(nrel(x) == 0 && x.pad0 == 0 && x.pad1 == 0);
    }
    {   // F_OWNS on the killer, on a victim, on all three
        Parked p;
        p.thread(1, Parked::w0(1, OWNS), 1, 10, 11, Parked::ref(4, 20), Parked::ref(5, 21));
        p.thread(4, Parked::w0(4, ST), 1, 20, 30);
        p.thread(5, Parked::w0(4, ST), 2, 21, 31);
        p.thread(2, Parked::w0(1, 0), 1, 11, 12, Parked::ref(6, 22), Parked::ref(7, 23));
        p.thread(6, Parked::w0(4, ST), 1, 22, 32);
        p.thread(7, Parked::w0(4, ST | OWNS), 3, 23, 33);
        p.thread(3, Parked::w0(1, OWNS), 0, 12, 13, Parked::ref(8, 24), Parked::ref(9, 25));
        p.thread(8, Parked::w0(4, ST | OWNS), 1, 24, 34);
        p.thread(9, Parked::w0(4, ST | OWNS), 2, 25, 35);
        p.rh[1] = 0; p.rn[1] = 3;
        for (uint32_t k = 0; k < 3; ++k) p.entry(1, k, T, 1 + k, 11 + k);
        const CleanEffects fx = p.build(STUB);
        CHECK(p.plan.claimable == 3 && fx.exclusive);
        CHECK(nrel(fx.eff[0]) == 1 && fx.eff[0].rel_node[0] == 1 && fx.eff[0].rel_tid[0] == 10);
        CHECK(nrel(fx.eff[1]) == 1 && fx.eff[1].rel_node[0] == 3 && fx.eff[1].rel_tid[0] == 23);
        const EffEnt& c = fx.eff[2];
        CHECK(nrel(c) == 3 && c.rel_node[0] == 0 && c.rel_tid[0] == 12 && c.rel_node[1] == 1 && c.rel_tid[1] == 24 &&
              c.rel_node[2] == 2 && c.rel_tid[2] == 25);
        for (const EffEnt& x : fx.eff) CHECK(x.flags & EFF_VERDICT);
    }
    {   // the static verdict: a frame that catches ThreadKilled, a finally frame
        // (mask 0), three frames, an exception pending, not started, a kill-stub
        // entry as victim, a node out of range; and two that pass
        const struct { uint32_t w0v, node, m0, m1; bool ok; } V[9] = {
            {Parked::w0(4, ST, 1), 1, KILLED | 4u, 0, false},
            {Parked::w0(4, ST, 1), 1, 0, 0, false},
            {Parked::w0(4, ST, 2), 1, 4u, KILLED, false},
            {Parked::w0(4, ST, 2), 1, 4u, 0, false},
            {Parked::w0(4, ST, 3), 1, 4u, 4u, false},
            {Parked::w0(4, ST, 0, 3), 1, 0, 0, false},
            {Parked::w0(4, 0), 1, 0, 0, false},
            {Parked::w0(4, ST, 2), 1, 4u, 8u, true},
            {Parked::w0(4, ST, 1), 1, 4u, KILLED, true},  // (the second mask is no frame's)
        };
        Parked q(32, 16);
        for (uint32_t k = 0; k < 9; ++k) {
            q.thread(1 + k, Parked::w0(2, 0), 1, 10 + k, 40 + k, Parked::ref(12 + k, 60 + k));
            q.thread(12 + k, V[k].w0v, V[k].node, 60 + k, 80 + k, 0, 0, V[k].m0, V[k].m1);
            q.entry(0, k, T, 1 + k, 40 + k);
        }
        // a victim that resumes at a kill-stub entry, and one on a node out of range
        q.thread(10, Parked::w0(2, 0), 1, 19, 49, Parked::ref(21, 69));
        q.thread(21, Parked::w0(2, ST), 1, 69, 89);
        q.entry(0, 9, T, 10, 49);
        q.thread(11, Parked::w0(2, 0), 1, 20, 50, Parked::ref(22, 70));
        q.thread(22, Parked::w0(4, ST), 9, 70, 90);
        q.entry(0, 10, T, 11, 50);
        q.rh[0] = 0; q.rn[0] = 11;
        const CleanEffects fx = q.build(STUB);
        CHECK(q.plan.claimable == 11 && fx.eff.size() == 11 && fx.exclusive);
        for (uint32_t k = 0; k < 9; ++k) CHECK(((fx.eff[k].flags & EFF_VERDICT) != 0) == V[k].ok);
        CHECK(!(fx.eff[9].flags & EFF_VERDICT) && !(fx.eff[10].flags & EFF_VERDICT));
    }
    {   // a victim named twice: by two kill wakes, and by both refs of one
        Parked p;
        p.thread(1, Parked::w0(1, 0), 1, 10, 11, Parked::ref(4, 20), Parked::ref(4, 20));
        p.thread(2, Parked::w0(1, 0), 1, 11, 12, Parked::ref(5, 21), Parked::ref(6, 22));
        p.thread(3, Parked::w0(1, 0), 1, 12, 13, Parked::ref(6, 22), Parked::ref(7, 23));
        p.thread(8, Parked::w0(2, 0), 1, 13, 14, Parked::ref(9, 24));
        p.thread(4, Parked::w0(4, ST), 1, 20, 30);
        p.thread(5, Parked::w0(4, ST), 1, 21, 31);
        p.thread(6, Parked::w0(4, ST), 1, 22, 32);
        p.thread(7, Parked::w0(4, ST), 1, 23, 33);
        p.thread(9, Parked::w0(4, ST), 1, 24, 34);
        p.rh[0] = 0; p.rn[0] = 4;
        p.entry(0, 0, T, 1, 11);
        p.entry(0, 1, T, 2, 12);
        p.entry(0, 2, T, 3, 13);
        p.entry(0, 3, T, 8, 14);
        const CleanEffects fx = p.build(STUB);
        CHECK(p.plan.claimable == 4 && !fx.exclusive);
        CHECK(!(fx.eff[0].flags & EFF_EXCL) && !(fx.eff[1].flags & EFF_EXCL) && !(fx.eff[2].flags & EFF_EXCL));
        CHECK(fx.eff[3].flags & EFF_EXCL);
        CHECK(nadd(fx.eff[0]) == 1 && fx.eff[0].add_kills[0] == 2);  // (as apply would merge them, were both claimed)
    }
    {   // the refs recorded for every kill wake, claimable or not: a killer in
        // slot 0 is not claimable, its refs still count for exclusivity
        Parked p;
        p.thread(0, Parked::w0(1, 0), 1, 9, 10, Parked::ref(4, 20), Parked::ref(5, 21));
        p.thread(1, Parked::w0(2, 0), 1, 10, 11, Parked::ref(6, 22));
        p.thread(4, Parked::w0(4, ST), 1, 20, 30);
        p.thread(5, Parked::w0(4, ST), 1, 21, 31);
        p.thread(6, Parked::w0(4, ST), 1, 22, 32);
        p.rh[0] = 0; p.rn[0] = 2;
        p.entry(0, 0, T, 0, 10);
        p.entry(0, 1, T, 1, 11);
        CleanEffects fx = p.build(STUB);
        CHECK(p.plan.claimable == 1 && fx.exclusive);
        CHECK(fx.eff[0].flags == 0 && fx.eff[0].nxref == 2 && fx.eff[0].xref[0] == 4 && fx.eff[0].xref[1] == 20 &&
              fx.eff[0].xref[2] == 5 && fx.eff[0].xref[3] == 21);
        CHECK((fx.eff[1].flags & EFF_EXCL) && fx.eff[1].nxref == 1 && fx.eff[1].xref[0] == 6 && fx.eff[1].xref[1] == 22 &&
              fx.eff[1].xref[2] == 0);
        // ... and with slot 0's killer naming the other's victim, nothing is exclusive
        p.thread(0, Parked::w0(1, 0), 1, 9, 10, Parked::ref(4, 20), Parked::ref(6, 22));
        fx = p.build(STUB);
        CHECK(p.plan.claimable == 1 && !fx.exclusive && !(fx.eff[1].flags & EFF_EXCL));
        // a superseded entry (seq differs) records none
        p.entry(0, 0, T, 0, 99);
        fx = p.build(STUB);
        CHECK(fx.eff[0].nxref == 0 && fx.exclusive);
    }
    {   // two positions that are not claimable (a stale second ref each) name one
        // live victim: their refs are recorded, so the table-wide flag is false;
        // and one such position that names its victim twice
        Parked p;
        p.thread(1, Parked::w0(1, 0), 1, 10, 11, Parked::ref(4, 20), Parked::ref(6, 77));   // 6: tid 22, not 77
        p.thread(2, Parked::w0(1, 0), 1, 11, 12, Parked::ref(4, 20), Parked::ref(6, 78));
        p.thread(3, Parked::w0(2, 0), 1, 12, 13, Parked::ref(5, 21));                        // claimable
        p.thread(4, Parked::w0(4, ST), 1, 20, 30);
        p.thread(5, Parked::w0(4, ST), 1, 21, 31);
        p.thread(6, Parked::w0(4, ST), 1, 22, 32);
        p.rh[0] = 0; p.rn[0] = 3;
        for (uint32_t k = 0; k < 3; ++k) p.entry(0, k, T, 1 + k, 11 + k);
        CleanEffects fx = p.build(STUB);
        CHECK(p.plan.claimable == 1 && p.plan.ents[0].nref == 0 && p.plan.ents[1].nref == 0);
        CHECK(fx.eff[0].nxref == 2 && fx.eff[1].nxref == 2 && fx.eff[0].xref[0] == 4 && fx.eff[1].xref[0] == 4);
        CHECK((fx.eff[2].flags & EFF_EXCL) && !fx.exclusive);
        // with the second of them gone the table is exclusive again (slot 6 is named once)
        p.rn[0] = 1;
        p.rh[1] = 0; p.rn[1] = 1;
        p.entry(1, 0, T, 3, 13);
        fx = p.build(STUB);
        CHECK(p.plan.claimable == 1 && fx.eff.size() == 2 && fx.eff[0].nxref == 2 && fx.exclusive);
        // one position that is not claimable naming its live victim twice
        p.thread(1, Parked::w0(1, 0), 1, 10, 11, Parked::ref(4, 20), Parked::ref(4, 20));
        p.thread(4, Parked::w0(4, ST | MAIN), 1, 20, 30);   // (main as victim: not claimable)
        fx = p.build(STUB);
        CHECK(p.plan.claimable == 1 && p.plan.ents[0].nref == 0 && fx.eff[0].nxref == 2 && !fx.exclusive);
    }
    {   // a run window that wraps its ring
        Parked p;
        for (uint32_t k = 0; k < 4; ++k) {
            p.thread(1 + k, Parked::w0(2, 0), k, 10 + k, 11 + k, Parked::ref(8 + k, 20 + k));
            p.thread(8 + k, Parked::w0(4, ST), 3 - k, 20 + k, 30 + k);
        }
        p.rh[3] = 5; p.rn[3] = 6;
        p.entry(3, 5, 77, 13, 1);
        const uint32_t pos[4] = {6, 7, 0, 1};
        for (uint32_t k = 0; k < 4; ++k) p.entry(3, pos[k], T, 1 + k, 11 + k);
        p.entry(3, 2, T + 5, 13, 2);
        const CleanEffects fx = p.build(STUB);
        CHECK(p.plan.win[3].pos0 == 6 && p.plan.win[3].n == 4 && fx.eff.size() == 4 && fx.exclusive);
        for (uint32_t k = 0; k < 4; ++k) {
            const EffEnt& e = fx.eff[k];
            CHECK(e.slot[0] == 1 + k && e.slot[1] == 8 + k && e.add_node[0] == k && nadd(e) == 2 && e.add_node[1] == 3 - k &&
                  e.add_kills[0] == 0 && e.add_kills[1] == 1);
        }
    }
    {   // operands out of range, positions that are not claimable: empty rows; no table at all
        Parked p;
        p.thread(1, Parked::w0(2, 0), 1, 10, 11, Parked::ref(400, 20));          // ref slot >= S
        p.thread(2, Parked::w0(200, 0), 1, 11, 12, Parked::ref(8, 20));          // pc >= n_insns
        p.thread(3, Parked::w0(2, 0), 9, 12, 13, Parked::ref(8, 20));            // node >= N
        p.thread(8, Parked::w0(4, ST), 1, 20, 30);
        p.rh[0] = 0; p.rn[0] = 4;
        for (uint32_t k = 0; k < 3; ++k) p.entry(0, k, T, 1 + k, 11 + k);
        p.entry(0, 3, T, 4000, 19);                                              // entry slot >= S
        const CleanEffects fx = p.build(STUB);
        CHECK(p.plan.claimable == 0 && fx.eff.size() == 4 && !fx.exclusive);
        for (const EffEnt& e : fx.eff) CHECK(e.flags == 0 && e.slot[0] == 0 && e.add_node[0] == 0);
        // a table whose rows the directory no longer has; null inputs
        CleanPlan fake;
        fake.ents.assign(2, KillEnt{});
        fake.ents[0].e[2] = 5; fake.ents[0].nref = 1; fake.ents[0].ref[0] = 700;
        fake.ents[1].e[2] = 900; fake.ents[1].nref = 7;
        const CleanEffects g = clean_effects(p.L, p.rows.data(), p.rows.size(), p.snap.data(), p.snap.size(), STUB, fake);
        CHECK(g.eff.size() == 2 && g.eff[0].flags == 0 && g.eff[1].flags == 0 && !g.exclusive);
        const CleanEffects z = clean_effects(p.L, nullptr, 0, nullptr, 0, STUB, fake);
        CHECK(z.eff.size() == 2 && !z.exclusive);
        const CleanEffects y = clean_effects(p.L, p.rows.data(), p.rows.size(), p.snap.data(), 24, STUB, p.plan);
        CHECK(y.eff.size() == 4 && !y.exclusive);
    }
    printf("effects ok\n");
    return 0;
}

int from_image(const char* path, unsigned n) {
    FILE* f = fopen(path, "r");
    CHECK(f);
    unsigned ni = 0, nc = 0;
    CHECK(fscanf(f, "%u %u", &ni, &nc) == 2);
    std::vector<tw_insn> in(ni);
    std::vector<int64_t> k(nc);
    for (unsigned i = 0; i < ni; ++i) {
        unsigned w0 = 0;
        int imm = 0;
        CHECK(fscanf(f, "%u %d", &w0, &imm) == 2);
        in[i] = tw_insn{w0, imm};
    }
    for (unsigned i = 0; i < nc; ++i) CHECK(fscanf(f, "%" SCNd64, &k[i]) == 1);
    fclose(f);
    const SweepPlan sp = sweep_classify(in.data(), ni, k.data(), nc);
    CHECK(sp.times.size() == 1);
    uint32_t pc = ni;
    for (uint32_t i = 0; i + 1 < ni && pc == ni; ++i)
        if ((in[i].w0 & 0xFFu) == TW_OP_WAIT_ABS && sp.stub[i + 1]) pc = i + 1;
    CHECK(pc < ni && (sp.stub[pc] & SWB_TWO));
    CHECK(SWB_RA0(sp.stub[pc]) == 1 && SWB_RA1(sp.stub[pc]) == 2);
    // a victim's resume pc: any that is no kill-stub entry
    uint32_t vpc = 0;
    while (vpc < ni && sp.stub[vpc]) ++vpc;
    CHECK(vpc < ni);
    // n + 1 kill wakes (one per node and the observer's), two victims each on
    // the killer's node, the second with a frame for another code and its
    // node's owned listener; dealt over the runs; slot 0 is main
    const uint32_t K = n + 1, S = 3 * K + 1;
    Parked p(S, K + 3);
    p.L.n_insns = ni;
    p.L.N = n + 1;
    p.thread(0, Parked::w0(0, MAIN | ST), 0, 0, 1);
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < K; ++i) {
        const uint32_t ks = 1 + 3 * i, j = i & 3u;
        p.thread(ks, Parked::w0(pc, 0), i % (n + 1), 100 + 3 * i, 1000 + 3 * i, Parked::ref(ks + 1, 101 + 3 * i),
                 Parked::ref(ks + 2, 102 + 3 * i));
        p.thread(ks + 1, Parked::w0(vpc, ST), i % (n + 1), 101 + 3 * i, 1001 + 3 * i);
        p.thread(ks + 2, Parked::w0(vpc, ST | OWNS, 1), i % (n + 1), 102 + 3 * i, 1002 + 3 * i, 0, 0, 1u << 5);
        p.entry(j, cnt[j]++, sp.times[0], ks, 1000 + 3 * i);
    }
    for (uint32_t j = 0; j < 4; ++j) p.rn[j] = cnt[j];
    const CleanEffects fx = p.build(sp.stub.data(), sp.times[0]);
    uint32_t rows = 0, verdict = 0, excl = 0, adds = 0, kills = 0, rels = 0;
    for (const EffEnt& e : fx.eff) {
        rows += e.flags != 0;
        verdict += (e.flags & EFF_VERDICT) != 0;
        excl += (e.flags & EFF_EXCL) != 0;
        adds += nadd(e);
        rels += nrel(e);
        for (uint32_t a = 0; a < nadd(e); ++a) kills += e.add_kills[a];
        CHECK(e.flags == 0 || (e.pc == pc && e.add_node[0] == e.w1[0]));
    }
    printf("positions %zu rows %u verdict %u exclusive %u adds %u kills %u releases %u all_exclusive %u\n", fx.eff.size(),
           rows, verdict, excl, adds, kills, rels, fx.exclusive ? 1u : 0u);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 2) return from_image(argv[1], (unsigned)atoi(argv[2]));
    return hand_made();
}
