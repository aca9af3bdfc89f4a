// Stand-alone host program over csrc/prefix_clean.hpp (no HIP): the kill table
// and the claimed slots of a snapshot, and the row tags.  Built and run by
// tests/test_prefix_clean_host.py with -fsanitize=address,undefined.
// With arguments `image.txt n`: a program image as text (`n_insns n_consts`,
// then w0 imm per instruction, then the constants), classified here; a parked
// state of n + 1 kill wakes with two victims each is laid out around its kill
// stub and sweep time, and the table's counts are printed.
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
constexpr uint32_t F_STARTED_ = 1u, F_MAIN_ = 2u;

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
    void thread(uint32_t slot, uint32_t w0v, uint32_t node, uint32_t tid, uint32_t seq, uint64_t r1 = 0, uint64_t r2 = 0) {
        q[rec_addr(slot, 0)] = {w0v, node, tid, seq};
        q[rec_addr(slot, 1)] = {0, 0, 0, 0};
        q[rec_addr(slot, 2)] = {0, 0, (uint32_t)r1, (uint32_t)(r1 >> 32)};  // r0, r1
        q[rec_addr(slot, 3)] = {(uint32_t)r2, (uint32_t)(r2 >> 32), 0, 0};  // r2, r3
    }
    void entry(uint32_t j, uint32_t pos, int64_t t, uint32_t slot, uint32_t seq) {
        q[run_addr(j, pos)] = {(uint32_t)t, (uint32_t)((uint64_t)t >> 32), slot, seq};
    }
    // a few rows of other sizes in front, as the real directory has
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
    CleanPlan build(const uint32_t* stub, int64_t t = T) {
        finish();
        return clean_build(L, rows.data(), rows.size(), snap.data(), snap.size(), rh, rn, stub, t);
    }
};

// stub words by pc (n_insns = 8): 1: two throwTos r1, r2; 2: one throwTo r1
const uint32_t STUB[9] = {0, SWB_VALID | SWB_TWO | (1u << 2) | (2u << 4), SWB_VALID | (1u << 2), 0, 0, 0, 0, 0, 0};

bool is(const std::vector<uint32_t>& a, std::initializer_list<uint32_t> b) { return a == std::vector<uint32_t>(b); }

int hand_made() {
    {   // two refs; entries before and behind T; one ref in another run
        Parked p;
        p.thread(3, Parked::w0(1, 0), 1, 10, 5, Parked::ref(4, 11), Parked::ref(5, 12));
        p.thread(4, Parked::w0(4, F_STARTED_), 1, 11, 6);
        p.thread(5, Parked::w0(4, F_STARTED_), 1, 12, 7);
        p.thread(6, Parked::w0(2, 0), 2, 13, 8, Parked::ref(7, 14));
        p.thread(7, Parked::w0(4, F_STARTED_, 1), 2, 14, 9);
        p.rh[0] = 2; p.rn[0] = 3;
        p.entry(0, 2, 5000, 9, 1);
        p.entry(0, 3, T, 3, 5);
        p.entry(0, 4, T + 1, 9, 2);
        p.rh[2] = 0; p.rn[2] = 1;
        p.entry(2, 0, T, 6, 8);
        const CleanPlan c = p.build(STUB);
        CHECK(c.ents.size() == 2 && c.claimable == 2);
        CHECK(c.win.size() == 4 && c.win[0].pos0 == 3 && c.win[0].n == 1 && c.win[0].base == 0);
        CHECK(c.win[1].n == 0 && c.win[2].pos0 == 0 && c.win[2].n == 1 && c.win[2].base == 1 && c.win[3].n == 0);
        const KillEnt& a = c.ents[0];
        CHECK(a.e[0] == (uint32_t)T && a.e[1] == (uint32_t)((uint64_t)T >> 32) && a.e[2] == 3 && a.e[3] == 5);
        CHECK(a.kw2 == 10 && a.kw3 == 5 && a.nref == 2);
        CHECK(a.ref[0] == 4 && a.ref[1] == 11 && a.ref[2] == 5 && a.ref[3] == 12);
        CHECK(a.vw[0] == 11 && a.vw[1] == 6 && a.vw[2] == 12 && a.vw[3] == 7);
        const KillEnt& b = c.ents[1];
        CHECK(b.e[2] == 6 && b.kw2 == 13 && b.kw3 == 8 && b.nref == 1 && b.ref[0] == 7 && b.ref[1] == 14 && b.ref[2] == 0);
        CHECK(b.vw[0] == 14 && b.vw[1] == 9);
        CHECK(is(c.slots, {3, 4, 5, 6, 7}));
        // tags: quads 1 - 3 of the five claimed slots and nothing else
        const std::vector<uint32_t> tag = clean_tags(p.L, p.rows.data(), p.rows.size(), c.slots);
        CHECK(tag.size() == p.rows.size());
        uint32_t tagged = 0;
        for (size_t i = 0; i < tag.size(); ++i) {
            if (tag[i] == PCL_NO_SLOT) continue;
            ++tagged;
            bool found = false;
            for (uint32_t qd = 1; qd <= 3; ++qd) found = found || p.rows[i].dst == p.rec_addr(tag[i], qd);
            CHECK(found && p.rows[i].es == 16);
        }
        CHECK(tagged == 15);
        // no entry at that time
        const CleanPlan none = p.build(STUB, T + 7);
        CHECK(none.ents.empty() && none.slots.empty() && none.claimable == 0 && none.win[0].n == 0);
    }
    {   // a stale ref; a victim that is not queued; main and slot 0 as victims; a self-victim
        Parked p;
        p.thread(0, Parked::w0(5, F_MAIN_ | F_STARTED_), 0, 0, 3);
        p.thread(1, Parked::w0(1, 0), 1, 10, 11, Parked::ref(8, 77), Parked::ref(9, 21));  // 8: tid 20, not 77
        p.thread(2, Parked::w0(2, 0), 1, 12, 12, Parked::ref(10, 22));                      // 10: w3 == 0
        p.thread(3, Parked::w0(2, 0), 1, 13, 13, Parked::ref(0, 0));                        // slot 0 (main)
        p.thread(4, Parked::w0(2, 0), 1, 14, 14, Parked::ref(11, 23));                      // 11: F_MAIN
        p.thread(5, Parked::w0(2, 0), 1, 15, 15, Parked::ref(5, 15));                       // itself
        p.thread(6, Parked::w0(2, 0), 1, 16, 16, Parked::ref(9, 21));                       // fine
        p.thread(8, Parked::w0(4, F_STARTED_), 1, 20, 30);
        p.thread(9, Parked::w0(4, F_STARTED_), 1, 21, 31);
        p.thread(10, Parked::w0(4, F_STARTED_), 1, 22, 0);
        p.thread(11, Parked::w0(4, F_STARTED_ | F_MAIN_), 1, 23, 32);
        p.rh[1] = 0; p.rn[1] = 6;
        for (uint32_t k = 0; k < 6; ++k) p.entry(1, k, T, k + 1, 11 + k);
        const CleanPlan c = p.build(STUB);
        CHECK(c.ents.size() == 6 && c.claimable == 1 && c.win[1].n == 6 && c.win[1].pos0 == 0);
        for (uint32_t k = 0; k < 5; ++k) {
            CHECK(c.ents[k].nref == 0 && c.ents[k].e[2] == k + 1);
            for (int i = 0; i < 4; ++i) CHECK(c.ents[k].ref[i] == 0 && c.ents[k].vw[i] == 0);
        }
        CHECK(c.ents[5].nref == 1 && c.ents[5].ref[0] == 9);
        CHECK(is(c.slots, {6, 9}));  // 9 also named by the position with the stale ref: claimed once, by the other
    }
    {   // a victim named twice: by two kill wakes, and by both refs of one
        Parked p;
        p.thread(1, Parked::w0(1, 0), 1, 10, 11, Parked::ref(4, 20), Parked::ref(4, 20));
        p.thread(2, Parked::w0(1, 0), 1, 11, 12, Parked::ref(4, 20), Parked::ref(5, 21));
        p.thread(4, Parked::w0(4, F_STARTED_), 1, 20, 30);
        p.thread(5, Parked::w0(4, F_STARTED_), 1, 21, 31);
        p.rh[0] = 0; p.rn[0] = 2;
        p.entry(0, 0, T, 1, 11);
        p.entry(0, 1, T, 2, 12);
        const CleanPlan c = p.build(STUB);
        CHECK(c.claimable == 2 && is(c.slots, {1, 2, 4, 5}));
        CHECK(c.ents[0].ref[0] == 4 && c.ents[0].ref[2] == 4 && c.ents[0].vw[1] == 30 && c.ents[0].vw[3] == 30);
        const std::vector<uint32_t> tag = clean_tags(p.L, p.rows.data(), p.rows.size(), c.slots);
        uint32_t tagged = 0;
        for (uint32_t t : tag) tagged += t != PCL_NO_SLOT;
        CHECK(tagged == 12);
    }
    {   // a run window that wraps its ring
        Parked p;
        for (uint32_t k = 0; k < 4; ++k) {
            p.thread(1 + k, Parked::w0(2, 0), 1, 10 + k, 11 + k, Parked::ref(8 + k, 20 + k));
            p.thread(8 + k, Parked::w0(4, F_STARTED_), 1, 20 + k, 30 + k);
        }
        p.rh[3] = 5; p.rn[3] = 6;
        p.entry(3, 5, 77, 13, 1);
        const uint32_t pos[4] = {6, 7, 0, 1};
        for (uint32_t k = 0; k < 4; ++k) p.entry(3, pos[k], T, 1 + k, 11 + k);
        p.entry(3, 2, T + 5, 13, 2);
        const CleanPlan c = p.build(STUB);
        CHECK(c.win[3].pos0 == 6 && c.win[3].n == 4 && c.win[3].base == 0 && c.claimable == 4);
        for (uint32_t k = 0; k < 4; ++k) CHECK(c.ents[k].e[2] == 1 + k && c.ents[k].ref[0] == 8 + k);
        CHECK(is(c.slots, {1, 2, 3, 4, 8, 9, 10, 11}));
    }
    {   // operands out of range, rows the directory lacks, killers validate would refuse
        Parked p;
        p.thread(1, Parked::w0(2, 0), 1, 10, 11, Parked::ref(400, 20));          // ref slot >= S
        p.thread(2, Parked::w0(200, 0), 1, 11, 12, Parked::ref(8, 20));          // pc >= n_insns
        p.thread(3, Parked::w0(2, 0), 9, 12, 13, Parked::ref(8, 20));            // node >= N
        p.thread(4, Parked::w0(2, 0, 1), 1, 13, 14, Parked::ref(8, 20));         // a frame
        p.thread(5, Parked::w0(2, 0, 0, 3), 1, 14, 15, Parked::ref(8, 20));      // an exception pending
        p.thread(6, Parked::w0(2, 0), 1, 15, 99, Parked::ref(8, 20));            // superseded entry (seq differs)
        p.thread(7, Parked::w0(4, 0), 1, 16, 17, Parked::ref(8, 20));            // not a kill stub
        p.thread(8, Parked::w0(4, F_STARTED_), 1, 20, 30);
        p.rh[0] = 0; p.rn[0] = 8;
        for (uint32_t k = 0; k < 7; ++k) p.entry(0, k, T, 1 + k, 11 + k);
        p.entry(0, 7, T, 12, 18);                                                // a record the directory lacks
        p.rh[1] = 0; p.rn[1] = 1;
        p.entry(1, 0, T, 4000, 19);                                              // entry slot >= S
        p.rh[2] = 0; p.rn[2] = 9;                                                // count above the ring
        p.rh[3] = 8; p.rn[3] = 1;                                                // head outside the ring
        const CleanPlan c = p.build(STUB);
        CHECK(c.ents.size() == 9 && c.claimable == 0 && c.slots.empty());
        CHECK(c.win[0].n == 8 && c.win[1].n == 1 && c.win[2].n == 0 && c.win[3].n == 0);
        for (const KillEnt& e : c.ents) CHECK(e.nref == 0);
        // null inputs, an empty directory
        const CleanPlan z = clean_build(p.L, nullptr, 0, nullptr, 0, p.rh, p.rn, STUB, T);
        CHECK(z.ents.empty() && z.slots.empty() && z.win.size() == 4);
        const CleanPlan y = clean_build(p.L, p.rows.data(), 0, p.snap.data(), p.snap.size(), p.rh, p.rn, STUB, T);
        CHECK(y.ents.empty() && y.slots.empty());
        // a snapshot shorter than the directory says
        const CleanPlan x = clean_build(p.L, p.rows.data(), p.rows.size(), p.snap.data(), 24, p.rh, p.rn, STUB, T);
        CHECK(x.slots.empty());
    }
    printf("clean ok\n");
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
    // the parked resume pc: the stub entry behind a WAIT_ABS (`schedule (at t) kill`)
    uint32_t pc = ni;
    for (uint32_t i = 0; i + 1 < ni && pc == ni; ++i)
        if ((in[i].w0 & 0xFFu) == TW_OP_WAIT_ABS && sp.stub[i + 1]) pc = i + 1;
    CHECK(pc < ni && (sp.stub[pc] & SWB_TWO));
    const uint32_t a0 = SWB_RA0(sp.stub[pc]), a1 = SWB_RA1(sp.stub[pc]);
    CHECK(a0 == 1 && a1 == 2);  // (Parked::thread lays the refs out in r1 and r2)
    // n + 1 kill wakes (one per node and the observer's), two victims each,
    // dealt over the runs; slot 0 is main
    const uint32_t K = n + 1, S = 3 * K + 1;
    Parked p(S, K + 3);
    p.L.n_insns = ni;
    p.L.N = n + 1;
    p.thread(0, Parked::w0(0, F_MAIN_ | F_STARTED_), 0, 0, 1);
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < K; ++i) {
        const uint32_t ks = 1 + 3 * i, j = i & 3u;
        p.thread(ks, Parked::w0(pc, 0), i % (n + 1), 100 + 3 * i, 1000 + 3 * i, Parked::ref(ks + 1, 101 + 3 * i),
                 Parked::ref(ks + 2, 102 + 3 * i));
        p.thread(ks + 1, Parked::w0(0, F_STARTED_), i % (n + 1), 101 + 3 * i, 1001 + 3 * i);
        p.thread(ks + 2, Parked::w0(0, F_STARTED_, 1), i % (n + 1), 102 + 3 * i, 1002 + 3 * i);
        p.entry(j, cnt[j]++, sp.times[0], ks, 1000 + 3 * i);
    }
    for (uint32_t j = 0; j < 4; ++j) p.rn[j] = cnt[j];
    const CleanPlan c = p.build(sp.stub.data(), sp.times[0]);
    const std::vector<uint32_t> tag = clean_tags(p.L, p.rows.data(), p.rows.size(), c.slots);
    uint32_t tagged = 0;
    for (uint32_t t : tag) tagged += t != PCL_NO_SLOT;
    printf("positions %zu claimable %u claimed %zu tagged %u\n", c.ents.size(), c.claimable, c.slots.size(), tagged);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 2) return from_image(argv[1], (unsigned)atoi(argv[2]));
    return hand_made();
}
