// sweep.hip — same-time killThread sweeps as data-parallel kernels.
//
// C3's teardown is, per replica, 4,097 kill wakes `throwTo r1; throwTo r2; END`
// at one absolute time T and the 8,194 victim pops behind them: a serial chain
// of ~12.3k pops on the event loop's one lane per replica.  The host stops
// every replica just before a statically known sweep time (sh_run runs the
// event kernel to T - 1 first) and these kernels carry out all the pops at T
// of a replica at once, over the state the event kernel's epilogue persisted.
// Lanes are 64 consecutive replicas (the replica-minor arrays coalesce); a
// replica's entries are dealt to gridDim.y waves.
//
//   scan      per replica: is every event at T in a prefix of the far runs?
//             (prefix lengths by binary search: runs are monotone)
//   validate  read-only, per entry: a live kill-stub wake whose refs are stale
//             or name plain victims (see below); counts killers and throwTos
//   apply     per entry, replicas that passed: what the pops would have left
//             (replicas the sweep ends: tw_sweep_apply_term, only what is
//             still read of them -- hash terms, listener releases; §3t)
//   finalize  per replica: the scalar words, run heads, free-stack top
//
// A replica that fails any check is left exactly as it was and takes the
// event kernel's sequential path.  Plain C++ and vector atomics only.
#include <hip/hip_runtime.h>

#include "tw_dev.hpp"
#include "sweep_dev.hpp"
#include "sweep_classify.hpp"

namespace {

using namespace tw;

__device__ __forceinline__ uint32_t GAS* acc_at(const SweepTab& t, const Dev& c, int w, uint32_t r) {
    return gp(t.acc) + (size_t)w * c.R + r;
}
__device__ __forceinline__ uint4 GAS* run_ent(const Dev& c, uint32_t j, uint32_t pos, uint32_t r) {
    return gp(c.runs) + run_row(c, j, pos) + r;
}
__device__ __forceinline__ uint4 GAS* rec_q(const Dev& c, uint32_t slot, uint32_t r, uint32_t q) {
    return gp(c.slots) + rec_row(c, slot, q) + r;
}
__device__ __forceinline__ uint32_t seq_limit(const Dev& c) {
    return c.tie_mode == TW_TIE_FORKFIRST ? 0x7FFFFFFFu : 0xFFFFFFFFu;
}
// The sweep of stop `expect` runs once, right after the event-kernel launch
// that left every replica parked (n_active == 0: the launch's count of lanes
// that still had something to do before its t_end).  The host enqueues it
// after every launch of the segment; the others leave here.
__device__ __forceinline__ bool sweep_gate(const Dev& c, const SweepTab& t, uint32_t expect) {
    return *gp(c.n_active) == 0u && gp(t.stats)[SWS_FIRED] == (unsigned long long)expect;
}
// register i of a record from its register quads
__device__ __forceinline__ uint64_t reg_of(uint4 q2, uint4 q3, uint32_t i) {
    const uint32_t lo = i == 0 ? q2.x : i == 1 ? q2.z : i == 2 ? q3.x : q3.z;
    const uint32_t hi = i == 0 ? q2.y : i == 1 ? q2.w : i == 2 ? q3.y : q3.w;
    return ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------- scan
__global__ void __launch_bounds__(256) tw_sweep_scan(Dev c, SweepTab t, int64_t T, uint32_t expect) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= c.R || !sweep_gate(c, t, expect)) return;
    const size_t R = c.R;
    const uint64_t GAS* sc = gp(c.scal) + r;
    for (int w = 0; w < SW_COUNT; ++w) *acc_at(t, c, w, r) = 0u;
    const bool att = sc[SC_STATUS * R] == TW_REP_RUNNING && sc[SC_PENDING_MAIN * R] == 0 && sc[SC_LIVE * R] != 0 &&
                     c.Cr != 0;
    if (!att) { *acc_at(t, c, SW_BAD, r) = 2u; return; }
    // the earliest event outside the runs: near spill, far-heap top
    int64_t other = INT64_MAX;
    uint32_t nn = (uint32_t)sc[SC_NEAR_N * R];
    const bool spill_ok = nn <= t.near_cap;
    nn = spill_ok ? nn : 0u;
    for (uint32_t j = 0; j < nn; ++j) {
        const int64_t x = ent_t(gp(c.near_spill)[(size_t)j * R + r]);
        other = x < other ? x : other;
    }
    if ((uint32_t)sc[SC_FAR_N * R]) {
        const int64_t x = ent_t(gp(c.far)[r]);
        other = x < other ? x : other;
    }
    int64_t rmin = INT64_MAX;
    uint32_t pl[TW_RUNS];
    for (uint32_t j = 0; j < TW_RUNS; ++j) {
        const uint32_t rh = (uint32_t)sc[(SC_RH0 + j) * R], rn = (uint32_t)sc[(SC_RC0 + j) * R];
        pl[j] = 0;
        if (rn == 0 || rn > c.Cr || rh >= c.Cr) continue;
        const int64_t h = ent_t(*run_ent(c, j, rh, r));
        rmin = h < rmin ? h : rmin;
        uint32_t lo = 0, hi = rn;  // entries [0, lo) are at <= T
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            uint32_t pos = rh + mid;
            pos = pos >= c.Cr ? pos - c.Cr : pos;
            if (ent_t(*run_ent(c, j, pos, r)) <= T) lo = mid + 1;
            else hi = mid;
        }
        pl[j] = lo;
    }
    const int64_t first = other < rmin ? other : rmin;
    {   // for finalize's count of replicas with work left: the next event of a
        // replica that is not attempted, or the next one outside the runs
        const int64_t x = (first == T && other > T && spill_ok) ? other : first;
        *acc_at(t, c, SW_XLO, r) = (uint32_t)x;
        *acc_at(t, c, SW_XHI, r) = (uint32_t)((uint64_t)x >> 32);
    }
    if (first != T) { *acc_at(t, c, SW_BAD, r) = 2u; return; }  // nothing at T (or stopped short of it)
    if (other <= T || !spill_ok) { *acc_at(t, c, SW_BAD, r) = 1u; return; }
    for (uint32_t j = 0; j < TW_RUNS; ++j) *acc_at(t, c, SW_PL0 + j, r) = pl[j];
    // the register-cached top of the free stack goes to its place in memory:
    // apply appends behind it (position free_n - 1 is unused while the top is cached)
    const uint32_t fn = (uint32_t)sc[SC_FREE_N * R];
    if (fn != 0 && fn <= c.S) gp(c.free_stk)[(size_t)(fn - 1) * R + r] = (uint32_t)sc[SC_FTOP * R];
}

// what both per-entry kernels read of a prefix entry's killer
struct Killer {
    uint4 h;       // header quad
    uint32_t sw;   // stub word of its resume pc
    uint64_t ref0, ref1;  // its victims' refs (ref1: of a stub with two throwTos)
    uint32_t nref;
    // the kill table's claimable position here (§3o; tab false: none): whether
    // the replica's killer (w2, w3) and run entry are the table's, its second
    // and third quad and its killer's slot (the last four: validate's)
    bool tab, hit, ent;
    uint4 ka, kr;
    uint32_t kslot;
};

// run j's window of the kill table (n == 0: no table)
__device__ __forceinline__ KillWin kill_win(const SweepTab& t, uint32_t j) {
    return t.kill ? t.kwin[j] : KillWin{0u, 0u, 0u, 0u};
}

// `pos`: the entry's ring position, `kw`: its run's table window.  Where the
// killer's (w2, w3) are the table's, its register quads are the snapshot's
// (§3o) and the refs come from the table: quads 2 and 3 are not loaded.
// (KEEP: validate goes on comparing with the table's quads; apply only takes the refs)
template <bool KEEP>
__device__ __forceinline__ bool load_killer(const Dev& c, const SweepTab& t, uint32_t r, uint4 e, int64_t T, Killer& k,
                                            uint32_t pos, const KillWin& kw) {
    k.nref = 0;
    k.sw = 0;
    k.tab = k.hit = k.ent = false;
    k.ka = k.kr = make_uint4(0u, 0u, 0u, 0u);
    k.kslot = 0;
    if (ent_t(e) != T || e.z >= c.S) return false;
    k.h = *rec_q(c, e.z, r, 0);
    uint64_t tr0 = 0, tr1 = 0;  // the table's refs
    const uint32_t tk = pos >= kw.pos0 ? pos - kw.pos0 : pos + c.Cr - kw.pos0;
    if (tk < kw.n) {
        const uint4 GAS* kp = (const uint4 GAS*)gp(t.kill) + (size_t)(kw.base + tk) * 4u;
        const uint4 ka = kp[1];
        k.tab = ka.z != 0u;
        if (k.tab) {
            // (a tid names one thread and a thread keeps its slot: the killer's
            // (w2, w3) alone say that its registers are the snapshot's; validate
            // compares the entry too, for the position's dirty marks)
            const uint4 kr = kp[2];
            k.hit = ka.x == k.h.z && ka.y == k.h.w;
            tr0 = ((uint64_t)kr.y << 32) | kr.x;
            tr1 = ((uint64_t)kr.w << 32) | kr.z;
            if (KEEP) {
                const uint4 te = kp[0];
                k.ent = te.x == e.x && te.y == e.y && te.z == e.z && te.w == e.w;
                k.ka = ka; k.kr = kr; k.kslot = te.z;
            }
        }
    }
    const uint32_t pc = k.h.x & 0xFFFFu;
    k.sw = gp(t.stub)[pc < c.n_insns ? pc : c.n_insns];
    const uint32_t fl = (k.h.x >> FL_SHIFT) & 0x3Fu;
    // live, no exception pending, a kill-stub entry, not main, no frames
    if (k.h.w != e.w || (k.h.x >> EXC_SHIFT) != 0 || !(k.sw & SWB_VALID) || (fl & F_MAIN) || ((k.h.x >> 16) & 15u) != 0 ||
        k.h.y >= c.N)
        return false;
    const uint32_t a0 = SWB_RA0(k.sw), a1 = SWB_RA1(k.sw);
    const bool two = (k.sw & SWB_TWO) != 0;
    const bool n2 = a0 < 2 || (two && a1 < 2), n3 = a0 >= 2 || (two && a1 >= 2);
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    // (not `n2 ? *rec_q(..) : z`: the conditional's uint4 temporary stays in
    // memory, a scratch frame and a 16-byte scratch store per entry in both kernels)
    uint4 q2 = z, q3 = z;
    if (n2 && !k.hit) q2 = *rec_q(c, e.z, r, 2);
    if (n3 && !k.hit) q3 = *rec_q(c, e.z, r, 3);
    k.ref0 = k.hit ? tr0 : reg_of(q2, q3, a0);
    k.ref1 = !two ? 0ull : k.hit ? tr1 : reg_of(q2, q3, a1);
    k.nref = two ? 2u : 1u;
    return true;
}

// whether the entry's refs are the ones the effects table recorded for its
// position (§3t; rare)
__device__ __forceinline__ bool refs_recorded(const Dev& c, const SweepTab& t, const Killer& k, uint32_t pos,
                                           const KillWin& kw) {
    const uint32_t tk = pos >= kw.pos0 ? pos - kw.pos0 : pos + c.Cr - kw.pos0;
    if (!t.eff || tk >= kw.n) return false;
    const uint4 GAS* ep = (const uint4 GAS*)gp(t.eff) + (size_t)(kw.base + tk) * 8u;
    const uint4 x = ep[7];
    if (ep[6].w != k.nref || x.x != (uint32_t)k.ref0 || x.y != (uint32_t)(k.ref0 >> 32)) return false;
    return k.nref < 2u || (x.z == (uint32_t)k.ref1 && x.w == (uint32_t)(k.ref1 >> 32));
}

// a dying thread's owned listener is released by one store (Lane::rel_bind);
// with several dying owners of one node the last store would win, so only the
// node's current owner may die in a sweep
__device__ __forceinline__ bool owner_ok(const Dev& c, uint32_t r, uint4 h) {
    if (!(((h.x >> FL_SHIFT) & 0x3Fu) & F_OWNS)) return true;
    return gp(c.bind_own)[(size_t)h.y * c.R + r] == h.z;
}

// ------------------------------------------------------------------ validate
// (pinned to 8 waves per SIMD: left alone the compiler takes 102 scalar
// registers, which is 7 waves; so it keeps some in lanes of a vector register)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8)))
tw_sweep_validate(Dev c, SweepTab t, int64_t T, uint32_t expect) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r >= c.R || !sweep_gate(c, t, expect)) return;
    if (*acc_at(t, c, SW_BAD, r)) return;
    const size_t R = c.R;
    const uint64_t GAS* sc = gp(c.scal) + r;
    uint32_t nk = 0, nh = 0;
    bool bad = false;
    for (uint32_t j = 0; j < TW_RUNS && !bad; ++j) {
        const uint32_t pl = *acc_at(t, c, SW_PL0 + j, r), rh = (uint32_t)sc[(SC_RH0 + j) * R];
        // the kill table's window of this run (§3o): the replica's prefix must
        // hold all of it, or some position goes unchecked
        const KillWin kw = kill_win(t, j);
        if (kw.n) {
            const uint32_t off = kw.pos0 >= rh ? kw.pos0 - rh : kw.pos0 + c.Cr - rh;
            if ((uint64_t)off + kw.n > pl) gp(t.cflags)[CF_ALL_DIRTY] = 1u;
        }
        // (§3t: the clean bits are keyed by the loop's own index -- entry i of a
        // run whose head is the window's start is table position kw.base + i)
        for (uint32_t i = blockIdx.y; i < pl && !bad; i += gridDim.y) {
            uint32_t pos = rh + i;
            pos = pos >= c.Cr ? pos - c.Cr : pos;
            const uint4 e = *run_ent(c, j, pos, r);
            Killer k;
            if (!load_killer<true>(c, t, r, e, T, k, pos, kw) || !owner_ok(c, r, k.h)) { bad = true; break; }
            ++nk;
            // A claimable table position: the entry, the killer's (w2, w3), the
            // refs and each victim's (w2, w3) as the snapshot had them, or the
            // position's slots are dirty.  (A replica that turns bad is refused:
            // finalize sets CF_ALL_DIRTY for it.)
            const bool tab = k.tab;
            bool mis = tab && (!k.hit || !k.ent || k.ka.z != k.nref);
            const uint4 ka = k.ka, kr = k.kr;
            uint4 kv = make_uint4(0u, 0u, 0u, 0u);
            if (tab) {
                const uint32_t tk = pos >= kw.pos0 ? pos - kw.pos0 : pos + c.Cr - kw.pos0;
                kv = ((const uint4 GAS*)gp(t.kill) + (size_t)(kw.base + tk) * 4u)[3];
            }
            const uint32_t kslot = k.kslot;
#pragma unroll
            for (uint32_t v = 0; v < 2; ++v) {
                if (v >= k.nref) break;
                const uint64_t ref = v ? k.ref1 : k.ref0;
                const uint32_t ts = (uint32_t)ref, tid = (uint32_t)(ref >> 32);
                // (the table's refs are below S: a ref at or above it is a mismatch here)
                mis = mis || (tab && (ts != (v ? kr.z : kr.x) || tid != (v ? kr.w : kr.y)));
                if (ts >= c.S) continue;                      // a stale ref: no-op (Lane::throw_to)
                const uint4 h = *rec_q(c, ts, r, 0);
                mis = mis || (tab && (h.z != (v ? kv.z : kv.x) || h.w != (v ? kv.w : kv.y)));
                if (h.z != tid) continue;                     // dead: slot free or reused
                const uint32_t fl = (h.x >> FL_SHIFT) & 0x3Fu, nfr = (h.x >> 16) & 15u, pc = h.x & 0xFFFFu;
                bool ok = (fl & F_STARTED) && !(fl & F_MAIN) && (h.x >> EXC_SHIFT) == 0 && nfr <= 2 && h.w != 0 &&
                          h.y < c.N && gp(t.stub)[pc < c.n_insns ? pc : c.n_insns] == 0 && owner_ok(c, r, h);
                // (§3t) a victim whose (w2, w3) are the table's has the snapshot's
                // frames quad (§3o), and the table's verdict bit says that the
                // snapshot's passes: the quad is not loaded
                const bool stat =
                    tab && (ka.w & KILL_VERDICT) != 0u && h.z == (v ? kv.z : kv.x) && h.w == (v ? kv.w : kv.y);
                if (ok && nfr && !stat) {
                    // neither a finally frame (mask 0) nor one catching ThreadKilled
                    const uint4 f = *rec_q(c, ts, r, 1);
                    const uint32_t m0 = f.x >> 16, m1 = nfr > 1 ? f.y >> 16 : 0xFFFFu;
                    ok = m0 != 0 && m1 != 0 && !((m0 | (nfr > 1 ? m1 : 0u)) & (1u << TW_EXC_THREAD_KILLED));
                }
                if (!ok) { bad = true; break; }
                ++nh;
            }
            if (mis) {  // (the table's slots, all below S: plain byte stores, rare)
                gp(t.dirty)[kslot] = 1;
                gp(t.dirty)[kr.x] = 1;
                if (ka.z > 1u) gp(t.dirty)[kr.z] = 1;
            }
            // Refs that came from the registers (no table hit: the observer's kill
            // wake in slot 0, a killer forked since the snapshot) bind the replica
            // to the table only if they are the refs recorded for the position.
            // (every wave of the replica that sees others stores the same word;
            // without the clean bits nobody reads it: sweep_term)
            if (t.bits && !(tab && k.hit) && !refs_recorded(c, t, k, pos, kw)) *acc_at(t, c, SW_NOTAB, r) = 1u;
            if (t.bits && i < kw.n) {
                // one ballot per wave and position, stored by every lane that is
                // here: one address, one value (a lane that left the loop, or
                // never had entry i, is not clean)
                const unsigned long long cb = __ballot(tab && !mis && !bad && rh == kw.pos0);
                gp(t.bits)[(size_t)(kw.base + i) * gridDim.x + blockIdx.x] = cb;
            }
        }
    }
    if (bad) {
        __hip_atomic_fetch_or(acc_at(t, c, SW_BAD, r), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (nk) {
        __hip_atomic_fetch_add(acc_at(t, c, SW_K, r), nk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nh) __hip_atomic_fetch_add(acc_at(t, c, SW_H, r), nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The replica passed validation and the sweep fits its caps.  Every pop of the
// sweep is an event and every throwTo that hits a live victim takes a seq
// (Lane::throw_to's re-stamp).  The victims are counted once per throwTo here
// (two killers naming one victim: an upper bound of the distinct victims), so
// a sweep that only just fits the event cap may be refused: never the reverse.
__device__ __forceinline__ bool sweep_go(const Dev& c, const SweepTab& t, uint32_t r, uint64_t max_events) {
    if (*acc_at(t, c, SW_BAD, r)) return false;
    const uint64_t k = *acc_at(t, c, SW_K, r), h = *acc_at(t, c, SW_H, r);
    const uint64_t ev = gp(c.scal)[(size_t)SC_EVENTS * c.R + r], sq = gp(c.scal)[(size_t)SC_SEQ * c.R + r];
    return k != 0 && ev + k + h <= max_events && sq + h < (uint64_t)seq_limit(c);
}

// A TERMINAL replica (§3t), of those sweep_go passes: every ref of its sweep is
// a ref of the kill table (SW_NOTAB clear), the table names no victim twice,
// and every thread it has left is a kill wake of the sweep or a victim one of
// them hits.  Then each hit is a victim of its own, V = H, and the sweep ends
// the replica: live reaches 0, the status becomes DONE, and nothing reads its
// thread records or its free stack before the next tw_reset.
__device__ __forceinline__ bool sweep_term(const Dev& c, const SweepTab& t, uint32_t r) {
    if (!t.bits || !t.excl || *acc_at(t, c, SW_NOTAB, r)) return false;
    const uint64_t k = *acc_at(t, c, SW_K, r), h = *acc_at(t, c, SW_H, r);
    return gp(c.scal)[(size_t)SC_LIVE * c.R + r] == k + h;
}

constexpr uint32_t NONE = 0xFFFFFFFFu;  // a ref without a live victim
static_assert(PCL_F_STARTED == F_STARTED && PCL_F_OWNS == F_OWNS && PCL_EXC_THREAD_KILLED == TW_EXC_THREAD_KILLED &&
                  PCL_FL_SHIFT == FL_SHIFT && PCL_EXC_SHIFT == EXC_SHIFT && PCL_F_MAIN == F_MAIN,
              "prefix_clean.hpp reads the header as tw_dev.hpp lays it out");

// ------------------------------------------------------- apply, terminal path
// What the pops of a terminal replica leave that anything still reads: the
// hash terms, the released listeners and the count of victims.  No header
// store, no claim swap, no free-stack append.  An entry whose clean bit is set
// takes all of it from the effects row; any other loads the headers as
// tw_sweep_apply does, and stores nothing else either.
__global__ void __launch_bounds__(64) tw_sweep_apply_term(Dev c, SweepTab t, int64_t T, uint64_t max_events,
                                                           uint32_t expect) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r >= c.R || !sweep_gate(c, t, expect)) return;
    if (!sweep_go(c, t, r, max_events) || !sweep_term(c, t, r)) return;
    const size_t R = c.R;
    const uint64_t GAS* sc = gp(c.scal) + r;
    const uint64_t vterm = term0(T, TW_KIND_EXC | TW_EXC_THREAD_KILLED);
    auto hash_add = [&](uint32_t node, unsigned long long x) {
        __hip_atomic_fetch_add((unsigned long long GAS*)(gp(c.hash) + (size_t)node * R + r), x, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    };
    uint32_t nv = 0, nfast = 0;
    for (uint32_t j = 0; j < TW_RUNS; ++j) {
        const uint32_t pl = *acc_at(t, c, SW_PL0 + j, r), rh = (uint32_t)sc[(SC_RH0 + j) * R];
        const KillWin kw = kill_win(t, j);
        const bool at0 = kw.n != 0u && rh == kw.pos0;
        for (uint32_t i = blockIdx.y; i < pl; i += gridDim.y) {
            bool clean = false;
            if (at0 && i < kw.n)
                clean = ((gp(t.bits)[(size_t)(kw.base + i) * gridDim.x + blockIdx.x] >> threadIdx.x) & 1ull) != 0ull;
            if (clean) {
                const uint4 GAS* ep = (const uint4 GAS*)gp(t.eff) + (size_t)(kw.base + i) * 8u;
                const uint4 a = ep[0], b = ep[1];  // flags, pc, add_node[0..1]; add_node[2], add_kills[0..2]
                const uint32_t na = (a.x >> EFF_NADD_SHIFT) & 15u, nr = (a.x >> EFF_NREL_SHIFT) & 15u;
                hash_add(a.z, term0(T, TW_KIND_RESUME | a.y) + (unsigned long long)b.y * vterm);
                if (na > 1u) hash_add(a.w, (unsigned long long)b.z * vterm);
                if (na > 2u) hash_add(b.x, (unsigned long long)b.w * vterm);
                if (nr) {
                    const uint4 rn = ep[2], rt = ep[3];
                    gp(c.bind_rel)[(size_t)rn.x * R + r] = rt.x;
                    if (nr > 1u) gp(c.bind_rel)[(size_t)rn.y * R + r] = rt.y;
                    if (nr > 2u) gp(c.bind_rel)[(size_t)rn.z * R + r] = rt.z;
                }
                nv += b.y + b.z + b.w;
                ++nfast;
                continue;
            }
            uint32_t pos = rh + i;
            pos = pos >= c.Cr ? pos - c.Cr : pos;
            const uint4 e = *run_ent(c, j, pos, r);
            Killer k;
            if (!load_killer<false>(c, t, r, e, T, k, pos, kw)) continue;  // (validated: cannot happen)
            if (((k.h.x >> FL_SHIFT) & 0x3Fu) & F_OWNS) gp(c.bind_rel)[(size_t)k.h.y * R + r] = k.h.z;
            // a live victim is this ref's alone (table-bound, exclusive): no claim
            auto hit = [&](uint64_t ref) -> uint32_t {
                const uint32_t ts = (uint32_t)ref, tid = (uint32_t)(ref >> 32);
                if (ts >= c.S) return NONE;
                const uint4 h = *rec_q(c, ts, r, 0);
                if (h.z != tid) return NONE;
                if (((h.x >> FL_SHIFT) & 0x3Fu) & F_OWNS) gp(c.bind_rel)[(size_t)h.y * R + r] = tid;
                return h.y;
            };
            const uint32_t n0 = hit(k.ref0);
            const uint32_t n1 = k.nref > 1 ? hit(k.ref1) : NONE;
            const bool c0 = n0 != NONE, c1 = n1 != NONE;
            const bool m0 = c0 && n0 == k.h.y, m1 = c1 && n1 == k.h.y;
            hash_add(k.h.y, term0(T, TW_KIND_RESUME | (k.h.x & 0xFFFFu)) + (m0 ? vterm : 0ull) + (m1 ? vterm : 0ull));
            const bool s0 = c0 && !m0, s1 = c1 && !m1, both = s0 && s1 && n0 == n1;
            if (s0) hash_add(n0, both ? 2ull * vterm : vterm);
            if (s1 && !both) hash_add(n1, vterm);
            nv += (c0 ? 1u : 0u) + (c1 ? 1u : 0u);
        }
    }
    if (nv) __hip_atomic_fetch_add(acc_at(t, c, SW_V, r), nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nfast) __hip_atomic_fetch_add(acc_at(t, c, SW_FAST, r), nfast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// --------------------------------------------------------------------- apply
__global__ void __launch_bounds__(64) tw_sweep_apply(Dev c, SweepTab t, int64_t T, uint64_t max_events,
                                                      uint32_t expect) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r >= c.R || !sweep_gate(c, t, expect)) return;
    if (!sweep_go(c, t, r, max_events) || sweep_term(c, t, r)) return;
    const size_t R = c.R;
    const uint64_t GAS* sc = gp(c.scal) + r;
    const uint32_t fn0 = (uint32_t)sc[SC_FREE_N * R];
    const uint64_t vterm = term0(T, TW_KIND_EXC | TW_EXC_THREAD_KILLED);
    uint32_t nv = 0;
    for (uint32_t j = 0; j < TW_RUNS; ++j) {
        const uint32_t pl = *acc_at(t, c, SW_PL0 + j, r), rh = (uint32_t)sc[(SC_RH0 + j) * R];
        const KillWin kw = kill_win(t, j);
        for (uint32_t i = blockIdx.y; i < pl; i += gridDim.y) {
            uint32_t pos = rh + i;
            pos = pos >= c.Cr ? pos - c.Cr : pos;
            const uint4 e = *run_ent(c, j, pos, r);
            Killer k;
            if (!load_killer<false>(c, t, r, e, T, k, pos, kw)) continue;  // (validated: cannot happen)
            // the kill wake's pop: END (Lane::die_prep); its resume term goes out below
            if (((k.h.x >> FL_SHIFT) & 0x3Fu) & F_OWNS) gp(c.bind_rel)[(size_t)k.h.y * R + r] = k.h.z;
            *rec_q(c, e.z, r, 0) = make_uint4(k.h.x | (F_STARTED << FL_SHIFT), k.h.y, 0xFFFFFFFFu, 0u);
            // the victim dies once: whoever takes its queued seq owns its pop
            // (returns the victim's node, NONE for a ref that is stale or another killer's)
            auto claim = [&](uint64_t ref) -> uint32_t {
                const uint32_t ts = (uint32_t)ref, tid = (uint32_t)(ref >> 32);
                if (ts >= c.S) return NONE;
                uint4 GAS* hp = rec_q(c, ts, r, 0);
                const uint4 h = *hp;
                if (h.z != tid) return NONE;  // stale, or claimed by another killer already
                // its dead tid and the taken seq, w2 and w3, in one 8-byte swap (a
                // killer that loses the race stores the same two words again)
                const uint32_t old = (uint32_t)(__hip_atomic_exchange((unsigned long long GAS*)((uint32_t GAS*)hp + 2),
                                                                      0x00000000FFFFFFFFull, __ATOMIC_RELAXED,
                                                                      __HIP_MEMORY_SCOPE_AGENT) >> 32);
                if (old == 0) return NONE;
                if (((h.x >> FL_SHIFT) & 0x3Fu) & F_OWNS) gp(c.bind_rel)[(size_t)h.y * R + r] = tid;
                return h.y;
            };
            const uint32_t n0 = claim(k.ref0);
            const uint32_t n1 = k.nref > 1 ? claim(k.ref1) : NONE;
            const bool c0 = n0 != NONE, c1 = n1 != NONE;
            // the resume term and a ThreadKilled term per claimed victim: the
            // terms of one node go out as one add (the hash is a sum mod 2^64)
            unsigned long long kt = term0(T, TW_KIND_RESUME | (k.h.x & 0xFFFFu));
            const bool m0 = c0 && n0 == k.h.y, m1 = c1 && n1 == k.h.y;
            kt += (m0 ? vterm : 0ull) + (m1 ? vterm : 0ull);
            __hip_atomic_fetch_add((unsigned long long GAS*)(gp(c.hash) + (size_t)k.h.y * R + r), kt, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            const bool s0 = c0 && !m0, s1 = c1 && !m1, both = s0 && s1 && n0 == n1;
            if (s0)
                __hip_atomic_fetch_add((unsigned long long GAS*)(gp(c.hash) + (size_t)n0 * R + r),
                                       both ? 2ull * vterm : vterm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s1 && !both)
                __hip_atomic_fetch_add((unsigned long long GAS*)(gp(c.hash) + (size_t)n1 * R + r), vterm, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t nf = 1u + (c0 ? 1u : 0u) + (c1 ? 1u : 0u);
            nv += nf - 1u;
            // the freed slots go onto the free stack, behind what it held
            const uint32_t at = fn0 + __hip_atomic_fetch_add(acc_at(t, c, SW_FREE, r), nf, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT);
            if (at < c.S) gp(c.free_stk)[(size_t)at * R + r] = e.z;
            if (c0 && at + 1u < c.S) gp(c.free_stk)[(size_t)(at + 1u) * R + r] = (uint32_t)k.ref0;
            if (c1 && at + nf - 1u < c.S) gp(c.free_stk)[(size_t)(at + nf - 1u) * R + r] = (uint32_t)k.ref1;
        }
    }
    if (nv) __hip_atomic_fetch_add(acc_at(t, c, SW_V, r), nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ finalize
__global__ void __launch_bounds__(256) tw_sweep_finalize(Dev c, SweepTab t, int64_t T, uint64_t max_events,
                                                          int64_t t_end, uint32_t expect) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (!sweep_gate(c, t, expect)) return;
    unsigned long long k = 0, v = 0, ref = 0, rem = 0, term = 0, fast = 0;
    if (r < c.R) {
        const size_t R = c.R;
        uint64_t GAS* sc = gp(c.scal) + r;
        const uint32_t bad = *acc_at(t, c, SW_BAD, r);
        // the replica's next event, for the count of replicas a later launch has work for
        int64_t next = (int64_t)(((uint64_t)*acc_at(t, c, SW_XHI, r) << 32) | *acc_at(t, c, SW_XLO, r));
        if (sweep_go(c, t, r, max_events)) {
            term = sweep_term(c, t, r) ? 1ull : 0ull;  // (as both applies saw it: live is still the event kernel's)
            // (§3v) tw_sweep_apply stored this replica's dead headers: the next apply stores the header rows
            if (t.kill && !term) gp(t.cflags)[CF_HDR_OK] = CFH_GENERAL;
            fast = *acc_at(t, c, SW_FAST, r);
            k = *acc_at(t, c, SW_K, r);
            v = *acc_at(t, c, SW_V, r);
            const uint32_t h = *acc_at(t, c, SW_H, r), m = *acc_at(t, c, SW_FREE, r);
            sc[SC_EVENTS * R] += k + v;
            sc[SC_NOW * R] = (uint64_t)T;
            sc[SC_FINAL_T * R] = (uint64_t)T;
            const uint64_t live = sc[SC_LIVE * R] - (k + v);
            sc[SC_LIVE * R] = live;
            sc[SC_SEQ * R] += h;
            const uint32_t fn = (uint32_t)sc[SC_FREE_N * R] + m;
            sc[SC_FREE_N * R] = fn;
            if (fn != 0 && fn <= c.S) sc[SC_FTOP * R] = gp(c.free_stk)[(size_t)(fn - 1) * R + r];
            for (uint32_t j = 0; j < TW_RUNS; ++j) {
                const uint32_t pl = *acc_at(t, c, SW_PL0 + j, r);
                uint32_t rh = (uint32_t)sc[(SC_RH0 + j) * R] + pl;
                rh = rh >= c.Cr ? rh - c.Cr : rh;
                sc[(SC_RH0 + j) * R] = rh;
                const uint64_t left = sc[(SC_RC0 + j) * R] - pl;
                sc[(SC_RC0 + j) * R] = left;
                if (left) {
                    const int64_t x = ent_t(*run_ent(c, j, rh, r));
                    next = x < next ? x : next;
                }
            }
            if (live == 0) sc[SC_STATUS * R] = TW_REP_DONE;  // whileM_ notDone (TimedT.hs:239)
        } else {
            // not attempted, refused or over a cap: it was not checked against the
            // whole kill table, and may pop its events one by one later (§3o)
            if (t.kill) gp(t.cflags)[CF_ALL_DIRTY] = 1u;
            if (bad != 2u) {
                ref = 1;
                next = T;
            }
        }
        // (the event kernel's own rule for a lane it counts in n_active)
        if (sc[SC_STATUS * R] == TW_REP_RUNNING &&
            (sc[SC_PENDING_MAIN * R] != 0 || sc[SC_LIVE * R] == 0 || (sc[SC_EVENTS * R] < max_events && next <= t_end)))
            rem = 1;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        k += __shfl_xor(k, m, 64);
        v += __shfl_xor(v, m, 64);
        ref += __shfl_xor(ref, m, 64);
        rem += __shfl_xor(rem, m, 64);
        term += __shfl_xor(term, m, 64);
        fast += __shfl_xor(fast, m, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (k) __hip_atomic_fetch_add(gp(t.stats) + 0, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) __hip_atomic_fetch_add(gp(t.stats) + 1, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ref) __hip_atomic_fetch_add(gp(t.stats) + 2, ref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rem) __hip_atomic_fetch_add(gp(t.stats) + SWS_LEFT, rem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (term) __hip_atomic_fetch_add(gp(t.stats) + SWS_TERM, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fast) __hip_atomic_fetch_add(gp(t.stats) + SWS_FAST, fast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the stop is done (a kernel of its own: every block of finalize reads the gate)
// ... and, with a kill table: every replica was checked against all of it and
// none has work left that could write a record after the check (§3o); and
// whether all of them were terminal, so that no header was stored either (§3v)
__global__ void tw_sweep_mark(Dev c, SweepTab t, uint32_t expect) {
    if (!sweep_gate(c, t, expect)) return;
    if (t.kill) {
        const bool valid = gp(t.cflags)[CF_ALL_DIRTY] == 0u && gp(t.stats)[SWS_LEFT] == 0ull;
        gp(t.cflags)[CF_VALID] = valid ? 1u : 0u;
        gp(t.cflags)[CF_HDR_OK] = (valid && gp(t.cflags)[CF_HDR_OK] == 0u) ? 1u : 0u;
    }
    gp(t.stats)[SWS_FIRED] = (unsigned long long)expect + 1ull;
}

}  // namespace

namespace tw {

size_t sweep_acc_words(uint32_t R) { return (size_t)SW_COUNT * R; }

hipError_t sweep_launch(const Dev& d, const SweepTab& t, hipStream_t st, int64_t T, uint64_t max_events, int64_t t_end,
                        uint32_t expect) {
    const uint32_t groups = (d.R + 63u) / 64u;
    // a replica's entries over enough waves to fill the GPU (256 CUs x 8 waves and more)
    uint32_t chunks = 131072u / groups;
    chunks = chunks < 16u ? 16u : chunks > 256u ? 256u : chunks;
    const dim3 gr((d.R + 255u) / 256u), ge(groups, chunks);
    hipLaunchKernelGGL(tw_sweep_scan, gr, dim3(256), 0, st, d, t, T, expect);
    hipLaunchKernelGGL(tw_sweep_validate, ge, dim3(64), 0, st, d, t, T, expect);
    // (each replica is one kernel's: the terminal path's or the general one's)
    if (t.bits) hipLaunchKernelGGL(tw_sweep_apply_term, ge, dim3(64), 0, st, d, t, T, max_events, expect);
    hipLaunchKernelGGL(tw_sweep_apply, ge, dim3(64), 0, st, d, t, T, max_events, expect);
    hipLaunchKernelGGL(tw_sweep_finalize, gr, dim3(256), 0, st, d, t, T, max_events, t_end, expect);
    hipLaunchKernelGGL(tw_sweep_mark, dim3(1), dim3(1), 0, st, d, t, expect);
    return hipGetLastError();
}

}  // namespace tw
