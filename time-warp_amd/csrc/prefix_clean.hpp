// prefix_clean.hpp — which rows of the send-free prefix's snapshot an apply
// may leave unstored, and the table the killThread sweep proves it with
// (prefix.hip, sweep.hip).  Kept free of HIP so it compiles into a
// plain host program (tests/prefix_clean_main.cpp, run under ASan / UBSan).
//
// Between the snapshot and the image's last sweep time T most threads stay
// parked: the kill wakes at T and the victims their registers name.  Neither
// the sweep nor anything else stores quads 1 - 3 of such a record (frames and
// pending exception value; r0 - r3) unless the header's (w2, w3) -- tid and
// queued seq -- changes with it (§3o: the writer audit).  The KILL TABLE holds,
// for every run position whose snapshot entry is at T, what tw_sweep_validate
// loads there anyway: the run entry, the killer's (w2, w3), its refs and each
// victim's (w2, w3).  A position is CLAIMABLE if it passes the static side of
// validate's checks; the slots claimable positions name -- killer and victims
// -- are the CLAIMED SLOTS, and a replica whose words at a position differ
// from the table's marks that position's slots dirty.  The EFFECTS TABLE
//  says, per position, what its pops do: where a replica's words
// are the table's, the sweep applies them without loading a header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "sweep_classify.hpp"

namespace tw {

// One row of a replica-minor array: R elements of `es` bytes from device
// address `dst` (replica 0's element), whose snapshot value lies `off` bytes
// into the snapshot buffer.  es is 1, 4, 8 or a multiple of 16; off is a
// multiple of es (of 16 for the wider rows).
struct PrefixRow {
    uint64_t dst;
    uint32_t off;
    uint32_t es;
};

// the header fields read here (tw_dev.hpp's FL_SHIFT, EXC_SHIFT, F_MAIN:
// prefix.hip asserts that they agree)
constexpr uint32_t PCL_FL_SHIFT = 20u, PCL_EXC_SHIFT = 26u, PCL_F_MAIN = 2u;
constexpr uint32_t PCL_NO_SLOT = 0xFFFFFFFFu;  // a row's tag: not a claimed slot's quad 1 - 3

// The words of the clean flags, device memory.  CF_ALL_DIRTY: some replica was
// not checked against the whole table (not attempted, refused, a window the
// table's does not fit).  CF_VALID: published by the sweep's last kernel --
// every replica checked, none with work left; consumed by the next apply.
// CF_HDR_OK (§3v): published with it -- CF_VALID, and every replica the sweep
// carried out was terminal, so that no sweep kernel stored a thread header
// (until then the word is finalize's: CFH_GENERAL where one took the general path).
enum { CF_ALL_DIRTY, CF_VALID, CF_HDR_OK, CF_COUNT };
constexpr uint32_t CFH_GENERAL = 2u;

// One run position of the table: four quads, read by the sweep as such.
struct KillEnt {
    uint32_t e[4];    // the run entry: time lo, hi, slot, seq
    uint32_t kw2, kw3, nref, pad;  // the killer's tid and seq; refs (0: the position is not claimable)
    uint32_t ref[4];  // ref0 slot, tid; ref1 slot, tid
    uint32_t vw[4];   // victim 0's w2, w3; victim 1's
};
static_assert(sizeof(KillEnt) == 64, "KillEnt is four quads");
// KillEnt::pad of the table on the device: the position's EFF_VERDICT (below),
// where validate has the word in registers anyway (set by the host's glue)
constexpr uint32_t KILL_VERDICT = 1u;

// A run's table window: ring positions [pos0, pos0 + n) (it may wrap), whose
// entries are `base`, `base + 1`, .. of the table.
struct KillWin {
    uint32_t pos0, n, base, pad;
};

// the parked layout of sweep_dev.hpp's rec_row and run_row, as numbers
struct CleanLayout {
    uint64_t slots, runs;  // device address of replica 0's first record quad / run entry
    uint64_t R, RQ;        // elements per row; elements between a record's quads
    uint32_t S, Cr, N, n_insns, n_runs;
};

struct CleanPlan {
    std::vector<KillEnt> ents;
    std::vector<KillWin> win;     // [n_runs]
    std::vector<uint32_t> slots;  // the claimed slots, ascending
    uint32_t claimable = 0;       // positions
};

// The kill table of sweep time T from a snapshot: its bytes, its row
// directory, replica 0's run heads and counts (rh, rn: n_runs words each) and
// the image's stub words (n_insns + 1).  Whatever does not resolve -- a row the
// directory lacks, an operand out of range -- leaves its position unclaimed.
inline CleanPlan clean_build(const CleanLayout& L, const PrefixRow* rows, size_t n_rows, const uint8_t* snap,
                             size_t snap_bytes, const uint64_t* rh, const uint64_t* rn, const uint32_t* stub, int64_t T) {
    CleanPlan p;
    p.win.assign(L.n_runs, KillWin{0u, 0u, 0u, 0u});
    if (!rows || !snap || !rh || !rn || !stub || L.R == 0) return p;
    std::unordered_map<uint64_t, uint32_t> at;  // a 16-byte row's address -> its snapshot offset
    for (size_t i = 0; i < n_rows; ++i)
        if (rows[i].es == 16 && (uint64_t)rows[i].off + 16 <= snap_bytes) at.emplace(rows[i].dst, rows[i].off);
    struct Quad { uint32_t x, y, z, w; };
    auto quad = [&](uint64_t addr, Quad& q) {
        auto it = at.find(addr);
        if (it == at.end()) return false;
        std::memcpy(&q, snap + it->second, 16);
        return true;
    };
    auto rec = [&](uint32_t slot, uint32_t qd, Quad& q) {
        return slot < L.S && quad(L.slots + ((uint64_t)qd * L.RQ + (uint64_t)slot * L.R) * 16u, q);
    };
    auto reg_of = [](const Quad& q2, const Quad& q3, uint32_t i) {
        const uint32_t lo = i == 0 ? q2.x : i == 1 ? q2.z : i == 2 ? q3.x : q3.z;
        const uint32_t hi = i == 0 ? q2.y : i == 1 ? q2.w : i == 2 ? q3.y : q3.w;
        return ((uint64_t)hi << 32) | lo;
    };
    std::vector<uint8_t> claimed(L.S, 0);
    for (uint32_t j = 0; j < L.n_runs; ++j) {
        if (rn[j] == 0 || rn[j] > L.Cr || rh[j] >= L.Cr) continue;
        KillWin w{0u, 0u, (uint32_t)p.ents.size(), 0u};
        for (uint32_t k = 0; k < (uint32_t)rn[j]; ++k) {
            uint32_t pos = (uint32_t)rh[j] + k;
            pos = pos >= L.Cr ? pos - L.Cr : pos;
            Quad e;
            const bool have = quad(L.runs + (((uint64_t)j * L.Cr + pos) * L.R) * 16u, e);
            const bool at_T = have && (int64_t)(((uint64_t)e.y << 32) | e.x) == T;
            if (!at_T) {
                if (w.n) break;  // (a run is monotone: the entries at T are one stretch)
                continue;
            }
            if (w.n == 0) w.pos0 = pos;
            ++w.n;
            KillEnt ke;
            std::memset(&ke, 0, sizeof(ke));
            ke.e[0] = e.x; ke.e[1] = e.y; ke.e[2] = e.z; ke.e[3] = e.w;
            p.ents.push_back(ke);
            KillEnt& o = p.ents.back();
            // the static side of tw_sweep_validate: a live kill-stub wake, no
            // exception pending, no frames, not main (nor slot 0, which tw_reset writes)
            Quad h, q2, q3;
            if (e.z == 0 || !rec(e.z, 0, h) || !rec(e.z, 2, q2) || !rec(e.z, 3, q3)) continue;
            const uint32_t pc = h.x & 0xFFFFu, sw = stub[pc < L.n_insns ? pc : L.n_insns];
            if (h.w != e.w || h.w == 0 || (h.x >> PCL_EXC_SHIFT) != 0 || !(sw & SWB_VALID) ||
                (((h.x >> PCL_FL_SHIFT) & 0x3Fu) & PCL_F_MAIN) || ((h.x >> 16) & 15u) != 0 || h.y >= L.N)
                continue;
            const uint32_t nref = (sw & SWB_TWO) ? 2u : 1u;
            const uint64_t ref[2] = {reg_of(q2, q3, SWB_RA0(sw)), nref > 1 ? reg_of(q2, q3, SWB_RA1(sw)) : 0ull};
            bool ok = true;
            for (uint32_t v = 0; v < nref && ok; ++v) {
                // a snapshot thread with that tid, queued, not main, not slot 0, not the killer
                const uint32_t ts = (uint32_t)ref[v], tid = (uint32_t)(ref[v] >> 32);
                Quad vh;
                ok = ts != 0 && ts != e.z && rec(ts, 0, vh) && vh.z == tid && vh.w != 0 &&
                     !(((vh.x >> PCL_FL_SHIFT) & 0x3Fu) & PCL_F_MAIN);
                if (ok) {
                    o.ref[2 * v] = ts; o.ref[2 * v + 1] = tid;
                    o.vw[2 * v] = vh.z; o.vw[2 * v + 1] = vh.w;
                }
            }
            if (!ok) {
                std::memset(o.ref, 0, sizeof(o.ref));
                std::memset(o.vw, 0, sizeof(o.vw));
                continue;
            }
            o.kw2 = h.z; o.kw3 = h.w; o.nref = nref;
            ++p.claimable;
            claimed[e.z] = 1;
            for (uint32_t v = 0; v < nref; ++v) claimed[o.ref[2 * v]] = 1;
        }
        if (w.n) p.win[j] = w;
    }
    for (uint32_t s = 0; s < L.S; ++s)
        if (claimed[s]) p.slots.push_back(s);
    return p;
}

// The header fields the effects table reads (tw_dev.hpp's F_STARTED, F_OWNS and
// TW_EXC_THREAD_KILLED: sweep.hip asserts that they agree)
constexpr uint32_t PCL_F_STARTED = 1u, PCL_F_OWNS = 8u, PCL_EXC_THREAD_KILLED = 1u;

// What a claimable position's pops do, from the snapshot alone:
// one row per table position, parallel to CleanPlan::ents, eight quads.  The
// sweep reads the first four of a position whose words validate found equal
// to the table's: by §3o's claim, extended to w0 and w1, the replica's three
// headers are then the snapshot's and the row says everything apply would
// have learnt from them.
constexpr uint32_t EFF_VERDICT = 1u;  // every victim passes validate's static checks
constexpr uint32_t EFF_EXCL = 2u;     // no victim named by another position's recorded refs, or twice here
constexpr uint32_t EFF_NADD_SHIFT = 8u, EFF_NREL_SHIFT = 12u;  // counts, 0 - 3 each
struct EffEnt {
    uint32_t flags;         // EFF_* | adds << EFF_NADD_SHIFT | releases << EFF_NREL_SHIFT (0: not claimable)
    uint32_t pc;            // the killer's resume pc: add 0 carries term0(T, RESUME | pc)
    uint32_t add_node[3];   // the hash adds, merged per node as tw_sweep_apply merges them;
    uint32_t add_kills[3];  // ... add 0 is the killer's node; ThreadKilled terms in each
    uint32_t rel_node[3];   // the owned listeners released (bind_rel[node] = tid), killer first
    uint32_t pad0;
    uint32_t rel_tid[3];
    uint32_t pad1;
    // (the next nine words: what a store of the dead headers would need; no
    // kernel reads them -- the fast entry of a surviving replica is not built, §3t)
    uint32_t slot[3];       // killer, victim 0, victim 1 (unused: 0)
    uint32_t w0[3];         // their snapshot headers' w0 (pc, frames, flags, pending exception)
    uint32_t w1[3];         // ... and w1 (node)
    uint32_t pad2[2];
    // Every position whose snapshot killer is a kill wake, claimable or not (a
    // killer in slot 0 is not): the refs its registers hold, (slot, tid) each.
    // A replica whose refs at a position are these is bound to the table there
    // without its killer's (w2, w3) being compared.
    uint32_t nxref;
    uint32_t xref[4];
};
static_assert(sizeof(EffEnt) == 128, "EffEnt is eight quads");

struct CleanEffects {
    std::vector<EffEnt> eff;  // [CleanPlan::ents.size()]
    bool exclusive = false;   // some position is claimable and no slot is named twice by the recorded refs
};

// The effects table of a kill table built from the same snapshot and stub words.
inline CleanEffects clean_effects(const CleanLayout& L, const PrefixRow* rows, size_t n_rows, const uint8_t* snap,
                                  size_t snap_bytes, const uint32_t* stub, const CleanPlan& p) {
    CleanEffects out;
    out.eff.assign(p.ents.size(), EffEnt{});
    if (!rows || !snap || !stub || L.R == 0) return out;
    std::unordered_map<uint64_t, uint32_t> at;
    for (size_t i = 0; i < n_rows; ++i)
        if (rows[i].es == 16 && (uint64_t)rows[i].off + 16 <= snap_bytes) at.emplace(rows[i].dst, rows[i].off);
    struct Quad { uint32_t x, y, z, w; };
    auto rec = [&](uint32_t slot, uint32_t qd, Quad& q) {
        if (slot >= L.S) return false;
        auto it = at.find(L.slots + ((uint64_t)qd * L.RQ + (uint64_t)slot * L.R) * 16u);
        if (it == at.end()) return false;
        std::memcpy(&q, snap + it->second, 16);
        return true;
    };
    auto reg_of = [](const Quad& q2, const Quad& q3, uint32_t i) {
        const uint32_t lo = i == 0 ? q2.x : i == 1 ? q2.z : i == 2 ? q3.x : q3.z;
        const uint32_t hi = i == 0 ? q2.y : i == 1 ? q2.w : i == 2 ? q3.y : q3.w;
        return ((uint64_t)hi << 32) | lo;
    };
    // the refs of every position (a claimable one's are the kill table's), and
    // how often they name each slot
    std::vector<uint32_t> named(L.S, 0);
    for (size_t i = 0; i < p.ents.size(); ++i) {
        const KillEnt& k = p.ents[i];
        EffEnt& o = out.eff[i];
        if (k.nref >= 1 && k.nref <= 2) {
            o.nxref = k.nref;
            for (uint32_t w = 0; w < 4; ++w) o.xref[w] = k.ref[w];
        } else {
            Quad h, q2, q3;
            if (k.nref != 0 || !rec(k.e[2], 0, h) || !rec(k.e[2], 2, q2) || !rec(k.e[2], 3, q3)) continue;
            const uint32_t pc = h.x & 0xFFFFu, sw = stub[pc < L.n_insns ? pc : L.n_insns];
            if (h.w != k.e[3] || h.w == 0 || !(sw & SWB_VALID)) continue;
            o.nxref = (sw & SWB_TWO) ? 2u : 1u;
            const uint64_t r0 = reg_of(q2, q3, SWB_RA0(sw)), r1 = o.nxref > 1 ? reg_of(q2, q3, SWB_RA1(sw)) : 0ull;
            o.xref[0] = (uint32_t)r0; o.xref[1] = (uint32_t)(r0 >> 32);
            o.xref[2] = (uint32_t)r1; o.xref[3] = (uint32_t)(r1 >> 32);
        }
        for (uint32_t v = 0; v < o.nxref; ++v)
            if (o.xref[2 * v] < L.S) ++named[o.xref[2 * v]];
    }
    uint32_t claimable = 0;
    bool all = true;
    for (size_t i = 0; i < p.ents.size(); ++i) {
        const KillEnt& k = p.ents[i];
        EffEnt& o = out.eff[i];
        if (k.nref == 0 || k.nref > 2) continue;
        Quad h[3];
        bool have = rec(k.e[2], 0, h[0]);
        for (uint32_t v = 0; v < k.nref; ++v) have = have && rec(k.ref[2 * v], 0, h[1 + v]);
        if (!have) { all = false; continue; }  // (clean_build read the same rows: cannot happen)
        ++claimable;
        o.slot[0] = k.e[2];
        for (uint32_t v = 0; v < k.nref; ++v) o.slot[1 + v] = k.ref[2 * v];
        for (uint32_t s = 0; s <= k.nref; ++s) { o.w0[s] = h[s].x; o.w1[s] = h[s].y; }
        o.pc = h[0].x & 0xFFFFu;
        // the adds: the killer's node first, with the victims on it; the others
        // as one add where they share a node (sweep.hip: m0, m1, s0, s1, both)
        const uint32_t kn = h[0].y, n0 = h[1].y, n1 = k.nref > 1 ? h[2].y : 0u;
        const bool c1 = k.nref > 1, m0 = n0 == kn, m1 = c1 && n1 == kn;
        uint32_t na = 1;
        o.add_node[0] = kn;
        o.add_kills[0] = (m0 ? 1u : 0u) + (m1 ? 1u : 0u);
        const bool s0 = !m0, s1 = c1 && !m1, both = s0 && s1 && n0 == n1;
        if (s0) { o.add_node[na] = n0; o.add_kills[na] = both ? 2u : 1u; ++na; }
        if (s1 && !both) { o.add_node[na] = n1; o.add_kills[na] = 1u; ++na; }
        uint32_t nr = 0;
        for (uint32_t s = 0; s <= k.nref; ++s)
            if (((h[s].x >> PCL_FL_SHIFT) & 0x3Fu) & PCL_F_OWNS) { o.rel_node[nr] = h[s].y; o.rel_tid[nr] = h[s].z; ++nr; }
        bool verdict = true, excl = true;  // (exclusive among all positions' refs, claimable or not)
        for (uint32_t v = 0; v < k.nref; ++v) {
            const Quad& vh = h[1 + v];
            const uint32_t fl = (vh.x >> PCL_FL_SHIFT) & 0x3Fu, nfr = (vh.x >> 16) & 15u, pc = vh.x & 0xFFFFu;
            bool ok = (fl & PCL_F_STARTED) && !(fl & PCL_F_MAIN) && (vh.x >> PCL_EXC_SHIFT) == 0 && nfr <= 2 &&
                      vh.w != 0 && vh.y < L.N && stub[pc < L.n_insns ? pc : L.n_insns] == 0;
            Quad f{0u, 0u, 0u, 0u};
            if (ok && nfr) {
                ok = rec(o.slot[1 + v], 1, f);
                const uint32_t f0 = f.x >> 16, f1 = nfr > 1 ? f.y >> 16 : 0xFFFFu;
                ok = ok && f0 != 0 && f1 != 0 && !((f0 | (nfr > 1 ? f1 : 0u)) & (1u << PCL_EXC_THREAD_KILLED));
            }
            verdict = verdict && ok;
            excl = excl && named[o.slot[1 + v]] == 1;
        }
        all = all && excl;
        o.flags = (verdict ? EFF_VERDICT : 0u) | (excl ? EFF_EXCL : 0u) | (na << EFF_NADD_SHIFT) | (nr << EFF_NREL_SHIFT);
    }
    // A table-bound replica trusts the recorded refs of positions that are not
    // claimable too (validate takes them for the table's), so the table-wide
    // flag speaks of every recorded ref: no slot named twice, by whatever position.
    for (uint32_t s = 0; s < L.S; ++s) all = all && named[s] <= 1;
    out.exclusive = claimable != 0 && all;
    return out;
}

// The tag of every directory row: the slot whose quad 1, 2 or 3 it is when that
// slot is claimed, PCL_NO_SLOT for every other row.
inline std::vector<uint32_t> clean_tags(const CleanLayout& L, const PrefixRow* rows, size_t n_rows,
                                        const std::vector<uint32_t>& slots) {
    std::vector<uint32_t> tag(n_rows, PCL_NO_SLOT);
    std::vector<uint8_t> claimed(L.S, 0);
    for (uint32_t s : slots)
        if (s < L.S) claimed[s] = 1;
    const uint64_t span = L.RQ * 16u;  // bytes between a record's quads
    for (size_t i = 0; i < n_rows && L.R && span; ++i) {
        if (rows[i].es != 16 || rows[i].dst < L.slots) continue;
        const uint64_t b = rows[i].dst - L.slots, q = b / span, in = b % span;
        if (q < 1 || q > 3 || in % (L.R * 16u) != 0) continue;
        const uint64_t s = in / (L.R * 16u);
        if (s < L.S && claimed[s]) tag[i] = (uint32_t)s;
    }
    return tag;
}

// The CLASS of every directory row: what lets an apply leave it
// unstored.  RC_BODY rows are clean_tags' (same tags); the others widen it.
//   RC_HDR    quad 0 of a claimed slot (tag: the slot): with CF_HDR_OK -- no
//             replica's sweep took the general path, which stores dead headers
//   RC_RUN    the run entry at a claimable table position (tag: the position's
//             killer slot, which no other position shares; validate compares
//             the entry and marks all of a position's slots together)
//   RC_RESET  a row of nvars, hash, bind, bind_own, bind_rel or tmo_done whose
//             snapshot bytes are what tw_reset has just left in that element
//             (tag: PCL_NO_SLOT; no sweep is involved)
enum : uint8_t { RC_NONE, RC_BODY, RC_HDR, RC_RUN, RC_RESET, RC_COUNT };

// What tw_reset leaves, replica-uniform: the arrays' device addresses (replica
// 0's first element; 0: no such array), their rows, and each element's value.
// nvars: nv_init[i] (null: 0); hash: 0; bind: listen_init[n] (null: 0);
// bind_own, bind_rel: the two constants; tmo_done: 0.
struct ResetLayout {
    uint64_t nvars, hash, bind, bind_own, bind_rel, tmo_done;
    uint32_t N, T;                // nodes (nvars: 4 rows each); timeouts
    const int64_t* nv_init;       // [4 * N] or null
    const uint32_t* listen_init;  // [N] or null
    uint32_t own0, rel0;
};

struct RowClasses {
    std::vector<uint8_t> cls;   // [n_rows] RC_*
    std::vector<uint32_t> tag;  // [n_rows] the slot whose dirty byte decides (RC_BODY, RC_HDR, RC_RUN), else PCL_NO_SLOT
    uint32_t n[RC_COUNT] = {0, 0, 0, 0, 0};      // rows per class
    uint64_t bytes[RC_COUNT] = {0, 0, 0, 0, 0};  // ... and their bytes per replica
};

// rs null: no RC_RESET rows.  A plan without claimed slots gives RC_RESET rows only.
inline RowClasses clean_classes(const CleanLayout& L, const PrefixRow* rows, size_t n_rows, const uint8_t* snap,
                                size_t snap_bytes, const CleanPlan& p, const ResetLayout* rs) {
    RowClasses out;
    out.cls.assign(n_rows, RC_NONE);
    out.tag.assign(n_rows, PCL_NO_SLOT);
    if (!rows || L.R == 0) { out.n[RC_NONE] = (uint32_t)n_rows; return out; }
    std::vector<uint8_t> claimed(L.S, 0);
    for (uint32_t s : p.slots)
        if (s < L.S) claimed[s] = 1;
    // claimable positions by their run entry's address
    std::unordered_map<uint64_t, uint32_t> killer;
    for (uint32_t j = 0; j < L.n_runs && j < p.win.size() && L.Cr; ++j) {
        const KillWin& w = p.win[j];
        for (uint32_t k = 0; k < w.n; ++k) {
            if ((size_t)w.base + k >= p.ents.size()) break;
            const KillEnt& e = p.ents[w.base + k];
            if (e.nref == 0 || e.e[2] >= L.S || !claimed[e.e[2]]) continue;
            const uint32_t pos = (w.pos0 + k) % L.Cr;
            killer.emplace(L.runs + (((uint64_t)j * L.Cr + pos) * L.R) * 16u, e.e[2]);
        }
    }
    const uint64_t span = L.RQ * 16u;  // bytes between a record's quads
    // whether row r lies in a reset array of `n` rows of `es` bytes from `base`; its row index
    auto in = [&](const PrefixRow& r, uint64_t base, uint64_t n, uint32_t es, uint64_t& ix) {
        if (!base || r.es != es || r.dst < base) return false;
        const uint64_t b = r.dst - base, step = L.R * es;
        ix = b / step;
        return b % step == 0 && ix < n;
    };
    for (size_t i = 0; i < n_rows; ++i) {
        const PrefixRow& r = rows[i];
        uint8_t c = RC_NONE;
        if (r.es == 16) {
            auto it = killer.find(r.dst);
            if (it != killer.end()) {
                c = RC_RUN;
                out.tag[i] = it->second;
            } else if (span && r.dst >= L.slots) {
                const uint64_t b = r.dst - L.slots, q = b / span, off = b % span;
                const uint64_t s = off / (L.R * 16u);
                if (q <= 3 && off % (L.R * 16u) == 0 && s < L.S && claimed[s]) {
                    c = q == 0 ? RC_HDR : RC_BODY;
                    out.tag[i] = (uint32_t)s;
                }
            }
        } else if (rs && snap && (uint64_t)r.off + r.es <= snap_bytes) {
            uint64_t ix = 0;
            const uint8_t* v = snap + r.off;
            uint64_t want = 0;
            bool hit = true;
            if (in(r, rs->nvars, 4ull * rs->N, 8, ix)) want = rs->nv_init ? (uint64_t)rs->nv_init[ix] : 0ull;
            else if (in(r, rs->hash, rs->N, 8, ix)) want = 0;
            else if (in(r, rs->bind, rs->N, 4, ix)) want = rs->listen_init ? rs->listen_init[ix] : 0u;
            else if (in(r, rs->bind_own, rs->N, 4, ix)) want = rs->own0;
            else if (in(r, rs->bind_rel, rs->N, 4, ix)) want = rs->rel0;
            else if (in(r, rs->tmo_done, rs->T, 1, ix)) want = 0;
            else hit = false;
            uint64_t have = 0;
            std::memcpy(&have, v, r.es);  // (es is 1, 4 or 8; little-endian words)
            if (hit && have == want) c = RC_RESET;
        }
        out.cls[i] = c;
    }
    for (size_t i = 0; i < n_rows; ++i) {
        ++out.n[out.cls[i]];
        out.bytes[out.cls[i]] += rows[i].es;
    }
    return out;
}

}  // namespace tw
