// Stand-alone host program over csrc/prefix_clean.hpp (no HIP): the class of
// every directory row (clean_classes).  Built and run by
// tests/test_prefix_rows_host.py with -fsanitize=address,undefined.
// With arguments `image.txt n`: a program image as text (as
// prefix_clean_main.cpp reads it); a parked state of n + 1 kill wakes with two
// victims each and the observer's kill wake in slot 0 is laid out around the
// image's kill stub and sweep time, with the arrays tw_reset fills behind it,
// and the rows per class are printed.
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
constexpr uint32_t OWN0 = 0xFFFFFFFFu, REL0 = 0xFFFFFFFEu;

// a parked replica: records, run entries and the arrays tw_reset fills, with
// the directory over them (widest rows first, as prefix_directory sorts them)
struct Parked {
    CleanLayout L{0x10000ull, 0x900000ull, 4, 0, 16, 8, 4, 8, 4};
    // nvars, hash, bind, bind_own, bind_rel, tmo_done; N nodes, two timeouts
    ResetLayout rs{0x2000000ull, 0x2100000ull, 0x2200000ull, 0x2300000ull, 0x2400000ull, 0x2500000ull, 4, 2,
                   nullptr, nullptr, OWN0, REL0};
    std::map<uint64_t, std::vector<uint32_t>> q;  // 16-byte rows by address
    std::map<uint64_t, uint64_t> v8;              // 8-byte rows
    std::map<uint64_t, uint32_t> v4, v1;          // 4-byte rows, bytes
    uint64_t rh[4] = {0, 0, 0, 0}, rn[4] = {0, 0, 0, 0};
    std::vector<PrefixRow> rows;
    std::vector<uint8_t> snap;

    explicit Parked(uint32_t S = 16, uint32_t Cr = 8, uint32_t N = 4) {
        L.S = S;
        L.Cr = Cr;
        L.N = N;
        L.RQ = (uint64_t)S * L.R;
        rs.N = N;
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
    void nvar(uint32_t i, int64_t x) { v8[rs.nvars + (uint64_t)i * L.R * 8u] = (uint64_t)x; }
    void hash(uint32_t n, uint64_t x) { v8[rs.hash + (uint64_t)n * L.R * 8u] = x; }
    void bind(uint32_t n, uint32_t x) { v4[rs.bind + (uint64_t)n * L.R * 4u] = x; }
    void own(uint32_t n, uint32_t x) { v4[rs.bind_own + (uint64_t)n * L.R * 4u] = x; }
    void rel(uint32_t n, uint32_t x) { v4[rs.bind_rel + (uint64_t)n * L.R * 4u] = x; }
    void tmo(uint32_t e, uint8_t x) { v1[rs.tmo_done + (uint64_t)e * L.R] = x; }
    void finish() {
        rows.clear();
        snap.clear();
        auto put = [&](uint64_t addr, uint32_t es, const void* p) {
            rows.push_back(PrefixRow{addr, (uint32_t)snap.size(), es});
            snap.insert(snap.end(), (const uint8_t*)p, (const uint8_t*)p + es);
        };
        for (auto& kv : q) put(kv.first, 16u, kv.second.data());
        put(0x100ull, 8u, "\xAB\xAB\xAB\xAB\xAB\xAB\xAB\xAB");  // (a scalar row: of no class)
        for (auto& kv : v8) put(kv.first, 8u, &kv.second);
        for (auto& kv : v4) put(kv.first, 4u, &kv.second);
        for (auto& kv : v1) put(kv.first, 1u, &kv.second);
    }
    CleanPlan build(const uint32_t* stub, int64_t t = T) {
        finish();
        return clean_build(L, rows.data(), rows.size(), snap.data(), snap.size(), rh, rn, stub, t);
    }
    RowClasses classes(const CleanPlan& p, bool reset = true) const {
        return clean_classes(L, rows.data(), rows.size(), snap.data(), snap.size(), p, reset ? &rs : nullptr);
    }
    size_t row_at(uint64_t addr) const {
        for (size_t i = 0; i < rows.size(); ++i)
            if (rows[i].dst == addr) return i;
        return rows.size();
    }
};

// stub words by pc (n_insns = 8): 1: two throwTos r1, r2; 2: one throwTo r1
const uint32_t STUB[9] = {0, SWB_VALID | SWB_TWO | (1u << 2) | (2u << 4), SWB_VALID | (1u << 2), 0, 0, 0, 0, 0, 0};

// the counts add up, every classed row is what its class says, and the RC_BODY
// rows and tags are clean_tags'
int consistent(const Parked& p, const CleanPlan& c, const RowClasses& k) {
    CHECK(k.cls.size() == p.rows.size() && k.tag.size() == p.rows.size());
    const std::vector<uint32_t> tag = clean_tags(p.L, p.rows.data(), p.rows.size(), c.slots);
    uint32_t n[RC_COUNT] = {0, 0, 0, 0, 0};
    uint64_t by[RC_COUNT] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < p.rows.size(); ++i) {
        const uint8_t cl = k.cls[i];
        CHECK(cl < RC_COUNT);
        ++n[cl];
        by[cl] += p.rows[i].es;
        CHECK((cl == RC_BODY) == (tag[i] != PCL_NO_SLOT));
        if (cl == RC_BODY) CHECK(k.tag[i] == tag[i]);
        if (cl == RC_NONE || cl == RC_RESET) CHECK(k.tag[i] == PCL_NO_SLOT);
        if (cl == RC_BODY || cl == RC_HDR || cl == RC_RUN) {
            CHECK(p.rows[i].es == 16 && k.tag[i] != 0 && k.tag[i] < p.L.S);  // (never slot 0)
            bool cs = false;
            for (uint32_t s : c.slots) cs = cs || s == k.tag[i];
            CHECK(cs);
        }
        if (cl == RC_HDR) CHECK(p.rows[i].dst == p.rec_addr(k.tag[i], 0));
        if (cl == RC_RESET) CHECK(p.rows[i].es < 16);
    }
    for (int x = 0; x < RC_COUNT; ++x) CHECK(k.n[x] == n[x] && k.bytes[x] == by[x]);
    uint64_t all = 0;
    for (int x = 0; x < RC_COUNT; ++x) all += k.bytes[x];
    CHECK(all == p.snap.size());
    return 0;
}

int hand_made() {
    {   // two refs and one; entries before and behind T; the observer's kill wake in slot 0
        Parked p;
        p.thread(0, Parked::w0(2, F_MAIN_ | F_STARTED_), 0, 0, 4, Parked::ref(7, 14));
        p.thread(3, Parked::w0(1, 0), 1, 10, 5, Parked::ref(4, 11), Parked::ref(5, 12));
        p.thread(4, Parked::w0(4, F_STARTED_), 1, 11, 6);
        p.thread(5, Parked::w0(4, F_STARTED_), 1, 12, 7);
        p.thread(6, Parked::w0(2, 0), 2, 13, 8, Parked::ref(7, 14));
        p.thread(7, Parked::w0(4, F_STARTED_, 1), 2, 14, 9);
        p.thread(9, Parked::w0(4, F_STARTED_), 3, 15, 1);  // a sleeper: not claimed
        p.rh[0] = 2; p.rn[0] = 4;
        p.entry(0, 2, 5000, 9, 1);
        p.entry(0, 3, T, 3, 5);
        p.entry(0, 4, T, 0, 4);  // the observer's: a killer in slot 0 is not claimable
        p.entry(0, 5, T + 1, 9, 2);
        p.rh[2] = 0; p.rn[2] = 1;
        p.entry(2, 0, T, 6, 8);
        const CleanPlan c = p.build(STUB);
        CHECK(c.ents.size() == 3 && c.claimable == 2 && c.slots.size() == 5);
        const RowClasses k = p.classes(c);
        if (consistent(p, c, k)) return 1;
        CHECK(k.n[RC_HDR] == 5 && k.n[RC_BODY] == 15 && k.n[RC_RUN] == 2 && k.n[RC_RESET] == 0);
        // the claimable positions' entries, tagged with their killers
        CHECK(k.cls[p.row_at(p.run_addr(0, 3))] == RC_RUN && k.tag[p.row_at(p.run_addr(0, 3))] == 3);
        CHECK(k.cls[p.row_at(p.run_addr(2, 0))] == RC_RUN && k.tag[p.row_at(p.run_addr(2, 0))] == 6);
        // the observer's position, the entries off T, slot 0 and the sleeper: class 0
        CHECK(k.cls[p.row_at(p.run_addr(0, 4))] == RC_NONE);
        CHECK(k.cls[p.row_at(p.run_addr(0, 2))] == RC_NONE && k.cls[p.row_at(p.run_addr(0, 5))] == RC_NONE);
        for (uint32_t qd = 0; qd < 4; ++qd) {
            CHECK(k.cls[p.row_at(p.rec_addr(0, qd))] == RC_NONE);
            CHECK(k.cls[p.row_at(p.rec_addr(9, qd))] == RC_NONE);
            CHECK(k.cls[p.row_at(p.rec_addr(7, qd))] == (qd ? RC_BODY : RC_HDR) && k.tag[p.row_at(p.rec_addr(7, qd))] == 7);
        }
        // no entry at that time: no table, no class
        const CleanPlan none = p.build(STUB, T + 7);
        const RowClasses kn = p.classes(none);
        if (consistent(p, none, kn)) return 1;
        CHECK(kn.n[RC_NONE] == p.rows.size());
    }
    {   // a run window that wraps its ring; a position that is not claimable inside it
        Parked p;
        for (uint32_t k = 0; k < 4; ++k) {
            p.thread(1 + k, Parked::w0(2, 0), 1, 10 + k, 11 + k, Parked::ref(8 + k, k == 2 ? 99 : 20 + k));  // (k == 2: a stale ref)
            p.thread(8 + k, Parked::w0(4, F_STARTED_), 1, 20 + k, 30 + k);
        }
        p.rh[3] = 5; p.rn[3] = 6;
        p.entry(3, 5, 77, 13, 1);
        const uint32_t pos[4] = {6, 7, 0, 1};
        for (uint32_t k = 0; k < 4; ++k) p.entry(3, pos[k], T, 1 + k, 11 + k);
        p.entry(3, 2, T + 5, 13, 2);
        const CleanPlan c = p.build(STUB);
        CHECK(c.win[3].pos0 == 6 && c.win[3].n == 4 && c.claimable == 3);
        const RowClasses k = p.classes(c);
        if (consistent(p, c, k)) return 1;
        CHECK(k.n[RC_RUN] == 3 && k.n[RC_HDR] == 6 && k.n[RC_BODY] == 18);
        for (uint32_t i = 0; i < 4; ++i) {
            const size_t r = p.row_at(p.run_addr(3, pos[i]));
            CHECK(k.cls[r] == (i == 2 ? RC_NONE : RC_RUN));
            if (i != 2) CHECK(k.tag[r] == 1 + i);
        }
        CHECK(k.cls[p.row_at(p.run_addr(3, 5))] == RC_NONE && k.cls[p.row_at(p.run_addr(3, 2))] == RC_NONE);
        CHECK(k.cls[p.row_at(p.rec_addr(3, 0))] == RC_NONE && k.cls[p.row_at(p.rec_addr(10, 0))] == RC_NONE);
    }
    {   // the arrays tw_reset fills: zero and non-zero nv_init, with and without listen_init
        Parked p;
        p.thread(1, Parked::w0(2, 0), 1, 10, 11, Parked::ref(2, 20));
        p.thread(2, Parked::w0(4, F_STARTED_), 1, 20, 30);
        p.rh[0] = 0; p.rn[0] = 1;
        p.entry(0, 0, T, 1, 11);
        for (uint32_t i = 0; i < 16; ++i) p.nvar(i, i % 4 == 0 ? (int64_t)(7 + i) : i == 5 ? (int64_t)-3 : (int64_t)0);  // var 0 written; node 1's var 1 is -3
        for (uint32_t n = 0; n < 4; ++n) {
            p.hash(n, n == 2 ? 0ull : 0x1234ull + n);
            p.bind(n, n == 1 ? 0u : 40u + n);
            p.own(n, n == 3 ? OWN0 : 100u + n);
            p.rel(n, n == 0 ? 55u : REL0);
        }
        p.tmo(0, 0);
        p.tmo(1, 1);
        const CleanPlan c = p.build(STUB);
        CHECK(c.claimable == 1);
        {   // no nv_init, no listen_init: zeros
            const RowClasses k = p.classes(c);
            if (consistent(p, c, k)) return 1;
            // nvars: 11 zero rows; hash: node 2; bind: node 1; own: node 3; rel: nodes 1 - 3; tmo 0
            CHECK(k.n[RC_RESET] == 11 + 1 + 1 + 1 + 3 + 1);
            CHECK(k.bytes[RC_RESET] == 11 * 8 + 8 + 4 + 4 + 12 + 1);
            CHECK(k.cls[p.row_at(p.rs.nvars + 5ull * p.L.R * 8u)] == RC_NONE);
            CHECK(k.cls[p.row_at(p.rs.nvars + 6ull * p.L.R * 8u)] == RC_RESET);
            CHECK(k.cls[p.row_at(p.rs.bind_rel)] == RC_NONE && k.cls[p.row_at(p.rs.bind_own)] == RC_NONE);
            CHECK(k.cls[p.row_at(p.rs.tmo_done)] == RC_RESET && k.cls[p.row_at(p.rs.tmo_done + p.L.R)] == RC_NONE);
            CHECK(k.n[RC_HDR] == 2 && k.n[RC_RUN] == 1 && k.n[RC_BODY] == 6);
            // without the reset layout: none of them
            const RowClasses k0 = p.classes(c, false);
            if (consistent(p, c, k0)) return 1;
            CHECK(k0.n[RC_RESET] == 0 && k0.n[RC_HDR] == 2 && k0.n[RC_RUN] == 1);
        }
        {   // nv_init and listen_init as loaded: the class follows the values
            int64_t nvi[16];
            uint32_t lsi[4] = {40, 0, 9, 43};
            for (uint32_t i = 0; i < 16; ++i) nvi[i] = i == 0 ? 7 : i == 5 ? -3 : i == 6 ? 1 : 0;
            p.rs.nv_init = nvi;
            p.rs.listen_init = lsi;
            const RowClasses k = p.classes(c);
            if (consistent(p, c, k)) return 1;
            // nvars: row 0 (7 == 7), row 5 (-3), not row 6 (0 != 1), the other 10 zero rows;
            // bind: nodes 0, 1 and 3 (node 2 holds 42, not 9)
            CHECK(k.n[RC_RESET] == 12 + 1 + 3 + 1 + 3 + 1);
            CHECK(k.cls[p.row_at(p.rs.nvars)] == RC_RESET && k.cls[p.row_at(p.rs.nvars + 5ull * p.L.R * 8u)] == RC_RESET);
            CHECK(k.cls[p.row_at(p.rs.nvars + 6ull * p.L.R * 8u)] == RC_NONE);
            CHECK(k.cls[p.row_at(p.rs.nvars + 4ull * p.L.R * 8u)] == RC_NONE);  // 11 != 0
            CHECK(k.cls[p.row_at(p.rs.bind + 2ull * p.L.R * 4u)] == RC_NONE);
            CHECK(k.cls[p.row_at(p.rs.bind + 3ull * p.L.R * 4u)] == RC_RESET);
            p.rs.nv_init = nullptr;
            p.rs.listen_init = nullptr;
        }
        {   // arrays the context lacks, rows beyond the arrays' ends, a snapshot shorter than the directory says
            const ResetLayout keep = p.rs;
            p.rs.hash = 0;
            p.rs.T = 1;   // (the second timeout's row is no longer tmo_done's)
            p.rs.N = 3;   // (node 3's rows neither)
            const RowClasses k = p.classes(c);
            if (consistent(p, c, k)) return 1;
            CHECK(k.cls[p.row_at(keep.hash + 2ull * p.L.R * 8u)] == RC_NONE);
            CHECK(k.cls[p.row_at(keep.bind_own + 3ull * p.L.R * 4u)] == RC_NONE);
            CHECK(k.cls[p.row_at(keep.nvars + 13ull * p.L.R * 8u)] == RC_NONE);
            CHECK(k.cls[p.row_at(keep.nvars + 9ull * p.L.R * 8u)] == RC_RESET);
            p.rs = keep;
            const size_t cut = p.rows[p.row_at(p.rs.bind_rel + 1ull * p.L.R * 4u)].off + 2;  // inside a 4-byte row
            const RowClasses ks = clean_classes(p.L, p.rows.data(), p.rows.size(), p.snap.data(), cut, c, &p.rs);
            CHECK(ks.cls[p.row_at(p.rs.bind_rel + 1ull * p.L.R * 4u)] == RC_NONE);
            CHECK(ks.cls[p.row_at(p.rs.bind_rel + 2ull * p.L.R * 4u)] == RC_NONE);
            CHECK(ks.cls[p.row_at(p.rs.nvars + 9ull * p.L.R * 8u)] == RC_RESET);
            // a row that starts inside an element's stride is not the array's
            std::vector<PrefixRow> odd = p.rows;
            const size_t z = p.row_at(p.rs.nvars + 9ull * p.L.R * 8u);
            odd[z].dst += 8;
            const RowClasses ko = clean_classes(p.L, odd.data(), odd.size(), p.snap.data(), p.snap.size(), c, &p.rs);
            CHECK(ko.cls[z] == RC_NONE);
        }
    }
    {   // rows the directory lacks, operands out of range
        Parked p;
        p.thread(1, Parked::w0(2, 0), 1, 10, 11, Parked::ref(2, 20));
        p.thread(2, Parked::w0(4, F_STARTED_), 1, 20, 30);
        p.rh[0] = 0; p.rn[0] = 1;
        p.entry(0, 0, T, 1, 11);
        const CleanPlan c = p.build(STUB);
        CHECK(c.claimable == 1);
        {   // the directory without the killer's header row and the run entry
            std::vector<PrefixRow> cut;
            for (const PrefixRow& r : p.rows)
                if (r.dst != p.rec_addr(1, 0) && r.dst != p.run_addr(0, 0)) cut.push_back(r);
            const RowClasses k = clean_classes(p.L, cut.data(), cut.size(), p.snap.data(), p.snap.size(), c, &p.rs);
            CHECK(k.cls.size() == cut.size() && k.n[RC_HDR] == 1 && k.n[RC_RUN] == 0 && k.n[RC_BODY] == 6);
        }
        {   // a plan whose windows, entries and slots point outside
            CleanPlan bad = c;
            bad.win[0].base = 7;                     // entries past the table's end
            bad.win[1] = KillWin{6, 5, 0, 0};        // a window that wraps, over rows the directory lacks
            bad.slots.push_back(4000);               // a slot >= S
            bad.ents[0].e[2] = 5000;
            const RowClasses k = p.classes(bad);
            CHECK(k.n[RC_RUN] == 0 && k.n[RC_HDR] == 2 && k.n[RC_BODY] == 6);
            bad = c;
            bad.ents[0].e[2] = 9;                    // a killer that is not claimed
            CHECK(p.classes(bad).n[RC_RUN] == 0);
            bad = c;
            bad.win.clear();                         // no windows at all
            CHECK(p.classes(bad).n[RC_RUN] == 0);
        }
        // null rows, an empty directory, no replicas, no snapshot
        const RowClasses z = clean_classes(p.L, nullptr, 0, nullptr, 0, c, &p.rs);
        CHECK(z.cls.empty() && z.tag.empty());
        const RowClasses y = clean_classes(p.L, p.rows.data(), 0, p.snap.data(), p.snap.size(), c, &p.rs);
        CHECK(y.cls.empty());
        CleanLayout L0 = p.L;
        L0.R = 0;
        const RowClasses x = clean_classes(L0, p.rows.data(), p.rows.size(), p.snap.data(), p.snap.size(), c, &p.rs);
        CHECK(x.n[RC_NONE] == p.rows.size());
        const RowClasses w = clean_classes(p.L, p.rows.data(), p.rows.size(), nullptr, 0, c, &p.rs);
        CHECK(w.n[RC_RESET] == 0 && w.n[RC_HDR] == 2 && w.n[RC_RUN] == 1);
    }
    printf("rows ok\n");
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
    CHECK(SWB_RA0(sp.stub[pc]) == 1 && SWB_RA1(sp.stub[pc]) == 2);  // (Parked::thread lays the refs out in r1 and r2)
    // n + 1 kill wakes, two victims each, dealt over the runs; slot 0 is the
    // observer, parked in a kill wake of its own at the same time
    const uint32_t K = n + 1, S = 3 * K + 1, N = n + 1;
    Parked p(S, K + 3, N);
    p.L.n_insns = ni;
    uint32_t cnt[4] = {0, 0, 0, 0};
    p.thread(0, Parked::w0(pc, F_MAIN_ | F_STARTED_), 0, 0, 1, Parked::ref(2, 101), Parked::ref(3, 102));
    p.entry(0, cnt[0]++, sp.times[0], 0, 1);
    for (uint32_t i = 0; i < K; ++i) {
        const uint32_t ks = 1 + 3 * i, j = i & 3u;
        p.thread(ks, Parked::w0(pc, 0), i % N, 100 + 3 * i, 1000 + 3 * i, Parked::ref(ks + 1, 101 + 3 * i),
                 Parked::ref(ks + 2, 102 + 3 * i));
        p.thread(ks + 1, Parked::w0(0, F_STARTED_), i % N, 101 + 3 * i, 1001 + 3 * i);
        p.thread(ks + 2, Parked::w0(0, F_STARTED_, 1), i % N, 102 + 3 * i, 1002 + 3 * i);
        p.entry(j, cnt[j]++, sp.times[0], ks, 1000 + 3 * i);
    }
    for (uint32_t j = 0; j < 4; ++j) p.rn[j] = cnt[j];
    // the ring's state at the snapshot: variable 0 of every node written, a
    // hash, a bound listener and its owner on every node, none released
    for (uint32_t i = 0; i < 4 * N; ++i) p.nvar(i, i % 4 == 0 ? 100 + i : 0);
    for (uint32_t m = 0; m < N; ++m) {
        p.hash(m, 0x9E3779B97F4A7C15ull * (m + 1));
        p.bind(m, 1u + m);
        p.own(m, 500u + m);
        p.rel(m, REL0);
    }
    p.tmo(0, 0);
    p.tmo(1, 0);
    const CleanPlan c = p.build(sp.stub.data(), sp.times[0]);
    const RowClasses rc = p.classes(c);
    if (consistent(p, c, rc)) return 1;
    CHECK(rc.cls[p.row_at(p.run_addr(0, 0))] == RC_NONE);  // the observer's position
    printf("positions %zu claimable %u hdr %u body %u run %u reset %u reset_bytes %" PRIu64 "\n", c.ents.size(),
           c.claimable, rc.n[RC_HDR], rc.n[RC_BODY], rc.n[RC_RUN], rc.n[RC_RESET], rc.bytes[RC_RESET]);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 2) return from_image(argv[1], (unsigned)atoi(argv[2]));
    return hand_made();
}
