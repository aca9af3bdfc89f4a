// engine.hip — MI355X (gfx950) batched TimedT event engine + the C ABI of
// include/timewarp.h.  Built into time-warp_amd/lib/libtimewarp.so.
//
// Replaces the pure-emulation runner of time-warp:
//   launchTimedT / runTimedT   src/Control/TimeWarp/Timed/TimedT.hs:234-304
//   fork / wait / throwTo / timeout               TimedT.hs:326-376
// for R independent replicas of one lowered scenario.
//
// Mapping to the hardware:
//   * one LANE per replica: a replica's event loop is strictly sequential in
//     TimedT (one pop at a time, TimedT.hs:239-263), replicas are independent,
//     so lanes never synchronise and the whole chip streams replicas;
//   * all per-replica HBM state is replica-minor ([index][replica]): while
//     replicas run in lock-step (scenario start-up, identical programs) a
//     wavefront's 64 accesses to "the same" slot/node/queue index coalesce into
//     contiguous 1-4 KiB transactions; when they diverge each lane touches one
//     64-B line per record;
//   * at one wave per SIMD nothing hides latency, so the event loop keeps its
//     working set on chip: TimedT's event queue (a pqueue MinQueue of
//     continuations) becomes an LDS NEAR heap of 64-bit keys (events due within
//     the scenario's horizon) with its root cached in registers, plus monotone
//     FIFO runs and a 4-ary heap in HBM for far events; the record the next
//     pop most likely needs is loaded into LDS staging by LDS-DMA one step
//     ahead, so the common pop -> run -> re-queue cycle rarely waits on HBM;
//   * every thread has at most one queued event, so throwTo's queue rebuild
//     (TimedT.hs:361-368) becomes an O(1) re-stamp: a fresh (now, seq) entry is
//     pushed (or the near entry re-keyed in place) and a superseded entry is
//     dropped lazily at pop time (slot.wake_seq no longer matches);
//   * the event order is (t, seq) with seq a per-replica insertion counter —
//     bit-identical to the oracle's canonical mode.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/timewarp.h"
#include "tw_dev.hpp"
#include "shard.hpp"
#include "run_state.hpp"
#include "load_plan.hpp"
#include "live_plan.hpp"
#include "sweep_classify.hpp"
#include "sweep_dev.hpp"
#include "prefix_classify.hpp"
#include "prefix_dev.hpp"

#include "engine_dev.hpp"

// ======================================================================= C ABI
struct tw_shard {
    // the context's own: made by sh_create, outlive every load
    int device = 0;
    hipStream_t stream = nullptr;     // where everything runs (tw_set_stream may replace it)
    hipStream_t own_stream = nullptr; // the context's stream
    uint32_t* h_active = nullptr;     // pinned
    uint32_t seq0 = 0, tid0 = 1;      // tw_set_counter_base: the context's, not the load's
    // pops per lane per tick of the device loop (TW_LP_TICK_BUDGET overrides it,
    // for tests: a small budget makes windows take several ticks), and the LP
    // launches' grid limit (above it they walk the list; TW_LP_GRID env): read
    // at tw_lp_loop_begin, kept since
    uint32_t lp_budget = 1u << 14;
    uint32_t lp_grid = TW_LP_GRID;
    LaunchTimes times;                // of the last tw_run (tw_last_launch_ms, tw_stats.kernel_ms); the event pool
    // the load: every field below is written by each load_common (describe,
    // allocate) and means nothing while `loaded` is false
    bool loaded = false;
    Dev d{};
    std::vector<void*> allocs;        // the load's device memory (dalloc); freed by free_all
    Dev* d_dev = nullptr;             // device copy of d (the wave kernel reads it through the scalar cache)
    size_t lds_bytes = 0;
    int geo = TW_GEO_DENSE;  // a replica geometry's TW_GEO_* (LP contexts: dense, unused; with_geo)
    uint32_t main_pc = 0, main_node = 0;
    int64_t* main_regs = nullptr;  // device copies for tw_reset
    int64_t* nv_init = nullptr;
    uint32_t* listen_init = nullptr;
    std::vector<uint32_t> tie_flags;  // tw_tie_audit, per replica
    // the features (run_state.hpp): each resets itself at free_all
    LpMode lpm;
    StatBuf st;
    Exchange ex;
    TickGraph tg;
    Sweep sw;
    Prefix px;
    // live delays (tw_set_live_delays): the load's buffers behind Dev::live_*
    // (made at the first call, kept while it is turned off and on again) and
    // the seed of the shard's first replica
    uint4* lv_desc = nullptr;
    uint2* lv_gen = nullptr;
    uint32_t* lv_n = nullptr;
    unsigned long long* lv_sum = nullptr;
    int64_t lv_seed0 = 0;
    Dev dwin() const {                // the descriptor the device loop's kernels get
        Dev x = d;
        x.win = ex.win_buf;
        return x;
    }
};

namespace {

template <class T>
int dalloc(tw_shard* c, T** p, size_t n) {
    void* q = nullptr;
    if (n == 0) n = 1;
    HIPCHK(hipMalloc(&q, n * sizeof(T)));
    c->allocs.push_back(q);
    *p = (T*)q;
    return TW_OK;
}

// unload: the load's device memory, then every feature's own
void free_all(tw_shard* c) {
    for (void* p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    c->lv_desc = nullptr; c->lv_gen = nullptr; c->lv_n = nullptr; c->lv_sum = nullptr;
    c->px.unload();
    c->sw.unload();
    trace_release(c->d);
    c->ex.unload(c->d);
    c->st.unload();
    c->tg.unload();
    c->lpm.unload();
    c->loaded = false;
}

}  // namespace

// ============================================================ kernel geometries
// One description per geometry of tw_run_kernel: its template arguments, whether
// it has the fork-in-place variant (IP; sparse: compiled out, LP: its own inline
// paths) and its near-spill entries per lane.  Everything the host knows about a
// geometry is derived from here.  The wave geometry (wave.hip: wave_launch, no
// LDS, wave_spill_entries) is the one special case: a branch where it matters.
using RunKernel = void (*)(Dev, int64_t, uint64_t, uint32_t);
template <bool LP_, int WG_, int NC_, int TPW_, bool RUNS_, bool IP_, int SPILL_>
struct Geo {
    static constexpr bool LP = LP_, RUNS = RUNS_, IP = IP_;
    static constexpr int WG = WG_, NC = NC_, TPW = TPW_, SPILL = SPILL_;
    static constexpr bool FAR_RUNS = !LP_ && RUNS_;  // (LP lanes and compact replicas: the HBM heap only)
    static constexpr size_t LDS = fixed_lds_bytes<WG_, NC_, LP_, RUNS_>();
    template <bool GS, bool PRW, bool FIP, bool TR, bool LV = false>
    static RunKernel kernel() {
        return tw_run_kernel<LP_, WG_, NC_, TPW_, RUNS_, GS, PRW, FIP, TR, LV>;
    }
};
using GeoDense = Geo<false, TW_WG, TW_NEAR_CAP, 64, true, true, TW_NEAR_CAP>;
using GeoSparse = Geo<false, TW_WG_SPARSE, TW_NEAR_SPARSE, 64, true, false, TW_NEAR_SPARSE>;
using GeoHalf = Geo<false, TW_WG, TW_NEAR_CAP, TW_HALF_LANES, true, true, TW_NEAR_CAP>;
using GeoNarrow = Geo<false, TW_NARROW, TW_NEAR_CAP, TW_NARROW, true, (TW_NARROW >= 64), TW_NEAR_CAP>;
using GeoCompact = Geo<false, TW_WG, TW_NEAR_COMPACT, 64, false, true, TW_NEAR_CAP>;
using GeoLP = Geo<true, TW_WG_LP, TW_NEAR_LP, 64, true, false, TW_NEAR_LP>;

// f(description) of the context's geometry (not the wave geometry's)
template <class F>
static auto with_geo(const tw_shard* c, F&& f) {
    if (c->lpm.lp) return f(GeoLP{});
    switch (c->geo) {
    case TW_GEO_SPARSE: return f(GeoSparse{});
    case TW_GEO_HALF: return f(GeoHalf{});
    case TW_GEO_NARROW: return f(GeoNarrow{});
    case TW_GEO_COMPACT: return f(GeoCompact{});
    default: return f(GeoDense{});
    }
}

// The replica geometries the killThread sweeps and the send-free prefix serve:
// far runs, and the dense near layout (TW_NEAR_CAP entries per lane) that
// sweep.hip and prefix.hip read.  Both also need a tie order in which a parked
// replica's equal-time entries pop in insertion order: ordered_ties.
static bool far_run_geo(const tw_shard* c) {
    return c->geo != TW_GEO_WAVE && with_geo(c, [](auto g) { return g.FAR_RUNS && g.NC == TW_NEAR_CAP; });
}
static bool ordered_ties(const tw_shard* c) {
    return c->d.tie_mode == TW_TIE_FIFO || c->d.tie_mode == TW_TIE_FORKFIRST;
}

// The instantiations of tw_run_kernel for geometry G, each with the variant it
// is: what load_common registers and what launch_run picks from.
//   LP: the work list walked grid-stride (gs: many lanes, few listed), the
//   batched device loop's per-replica windows (prw), TRACE records kept (tr:
//   tw_set_trace on a batched LP context, tw_lp_set_trace on a node-partitioned
//   one; the others compile Lane::trace_rec out);
//   replicas: the fork-in-place variant (ip: Lane::fork_in_place), and each of
//   the two once more with live delays (lv: Lane::live_entry; tw_set_live_delays).
struct Variant {
    bool gs, prw, ip, tr, lv = false;
    bool operator==(const Variant& o) const {
        return gs == o.gs && prw == o.prw && ip == o.ip && tr == o.tr && lv == o.lv;
    }
};
template <class G, class F>
static void each_kernel(F&& f) {  // f(RunKernel, Variant)
    constexpr bool T = true, N = false;
    f(G::template kernel<N, N, N, N>(), Variant{N, N, N, N});
    if constexpr (G::IP) f(G::template kernel<N, N, T, N>(), Variant{N, N, T, N});
    if constexpr (!G::LP) {
        f(G::template kernel<N, N, N, N, T>(), Variant{N, N, N, N, T});
        if constexpr (G::IP) f(G::template kernel<N, N, T, N, T>(), Variant{N, N, T, N, T});
    }
    if constexpr (G::LP) {
        f(G::template kernel<T, N, N, N>(), Variant{T, N, N, N});
        f(G::template kernel<N, T, N, N>(), Variant{N, T, N, N});
        f(G::template kernel<T, T, N, N>(), Variant{T, T, N, N});
        f(G::template kernel<N, N, N, T>(), Variant{N, N, N, T});
        f(G::template kernel<T, N, N, T>(), Variant{T, N, N, T});
        f(G::template kernel<N, T, N, T>(), Variant{N, T, N, T});
        f(G::template kernel<T, T, N, T>(), Variant{T, T, N, T});
    }
}

// The fork-in-place variant of a replica geometry that has one: under the tie
// orders where a forked child is always the next pop (FORKFIRST, LIFO), and
// for the compact geometry in every order.  Measured (round 4):
// C3 dense FIFO 17.8 G events/s without it, 16.3 G with it (the child is
// rarely next under FIFO and the code costs registers), FORKFIRST 19.4 G;
// C2 compact FIFO 39.7 G without, 43.2-44.0 G with (ping-pong forks into an
// empty queue: the child is next under FIFO too)
template <class G>
static bool use_ip(const tw_shard* c) {
    return G::IP &&
           (c->d.tie_mode == TW_TIE_FORKFIRST || c->d.tie_mode == TW_TIE_LIFO || c->geo == TW_GEO_COMPACT);
}

template <class G>
static void launch_run(tw_shard* c, hipStream_t st, int64_t t_end, uint64_t limit, uint32_t budget,
                       uint32_t grid = 0) {
    // grid: workgroups to launch, 0 = one per WG replicas (the prefix pilot
    // launches the first only; replica kernels, whose workgroups serve their own block)
    uint32_t blocks = (grid && !G::LP) ? grid : (uint32_t)((c->d.R + G::WG - 1) / G::WG);
    Variant v{false, false, use_ip<G>(c), false, c->d.live_desc != nullptr};
    if constexpr (G::LP) {
        v = Variant{blocks > c->lp_grid, c->d.rw && c->d.win, false, c->d.trace_cap != 0};
        if (v.gs) blocks = c->lp_grid;
    }
    each_kernel<G>([&](RunKernel k, Variant kv) {
        if (kv == v)
            hipLaunchKernelGGL(k, dim3(blocks), dim3(G::WG * 64 / G::TPW), c->lds_bytes, st, c->d, t_end, limit, budget);
    });
}

namespace tw {

int sh_create(int device, tw_shard** out) {
    if (!out) return TW_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return TW_ERR_NO_DEVICE;
    {
        // the kernels are built for gfx950 (MI355X) only
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return TW_ERR_NO_DEVICE;
    }
    tw_shard* c = new (std::nothrow) tw_shard;
    if (!c) return TW_ERR_OOM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void**)&c->h_active, sizeof(uint32_t)) != hipSuccess) {
        delete c;
        return TW_ERR_HIP;
    }
    c->own_stream = c->stream;
    // testing hook: TW_TEST_PREFIX_AUDIT=1 follows every apply that may skip
    // rows with a read-only kernel over the skipped rows (tw_prefix_clean_stats)
    if (const char* a = getenv("TW_TEST_PREFIX_AUDIT")) c->px.audit = atoi(a) != 0;
    // ... and TW_TEST_PREFIX_ROWS=0 leaves the apply the rows of §3o alone to
    // skip (no header, run-entry or reset-valued rows: the A/B arm of §3v)
    if (const char* a = getenv("TW_TEST_PREFIX_ROWS")) c->px.rows_on = atoi(a) != 0;
    // ... and TW_TEST_PREFIX_LIST=0 keeps a cached apply on the early-exit grid
    // (one workgroup per row and span, those of a skipped row return)
    if (const char* a = getenv("TW_TEST_PREFIX_LIST")) c->px.list_on = atoi(a) != 0;
    // testing hook: TW_TEST_SWEEP_SLOW=1 keeps every replica on tw_sweep_apply's
    // general path (no clean bits, no terminal path: the A/B arm of §3t)
    if (const char* a = getenv("TW_TEST_SWEEP_SLOW")) c->sw.slow = atoi(a) != 0;
    // ... and TW_TEST_SWEEP_FRAMES=1 keeps tw_sweep_validate's load of every
    // victim's frames quad (the kill table then carries no verdict bits)
    if (const char* a = getenv("TW_TEST_SWEEP_FRAMES")) c->sw.frames = atoi(a) != 0;
    *out = c;
    return TW_OK;
}

void sh_destroy(tw_shard* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_all(c);
    c->times.destroy();
    c->st.destroy();
    c->ex.destroy(c->d);
    c->sw.destroy();
    if (c->h_active) (void)hipHostFree(c->h_active);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int sh_reset(tw_shard* c);

// ===================================================================== the load
// load_common's stages; the checks, the batched mode's plan, the
// classifiers and the geometry choice are load_plan.hpp's.  A stage that
// fails just returns: load_common's one failure exit frees whatever the load
// has allocated by then.
constexpr size_t TW_LDS_LIMIT = 160 * 1024;  // a workgroup's LDS: program + constants must fit beside the queues
static const LoadLimits LOAD_LIMITS{TW_LIGHT, TW_HEAVY_CAP};

// the load's device tables on their way into Dev and tw_shard (null: not in this load)
struct LoadTabs {
    uint2* insns = nullptr;
    int64_t* consts = nullptr;
    uint32_t *lpc = nullptr, *out_off = nullptr, *ldst = nullptr, *lrev = nullptr, *ltab = nullptr;
    uint32_t* mbytes = nullptr;
    uint64_t* lbw = nullptr;
    uint32_t* iboff = nullptr;
    uint8_t* phd = nullptr;
    uint4* ldh = nullptr;
    int64_t *mregs = nullptr, *nvi = nullptr;
    uint32_t* lsi = nullptr;
};

// dalloc for a run of allocations: the first failure sticks and ends the run
struct Alloc {
    tw_shard* c;
    int rc = TW_OK;
    template <class T>
    void operator()(T*& p, size_t n) {
        if (rc == TW_OK) rc = dalloc(c, &p, n);
    }
};

// Stage "describe": the mode, Dev's dimensions, the geometry and its LDS
// bytes; every instantiation launch_run can pick is told them.
static int load_describe(tw_shard* c, const tw_scenario_desc* s, const LoadMode& m, const LpbPlan& plan) {
    const bool lp = m.lp(), lpb = m.lpb();
    Dev& d = c->d;
    d = Dev{};
    c->lpm.lp = lp;
    c->lpm.lpb = lpb;
    c->lpm.n_rep = lpb ? s->n_replicas : 1u;
    c->lpm.heavy_ok = plan.heavy_ok;
    c->lpm.has_ph1 = plan.has_ph1;
    d.rep_lg = m.rep_lg;
    d.lpb = lpb ? 1u : 0u;
    d.R = lp ? m.lp_count : s->n_replicas;
    d.S = s->max_slots; d.Q = s->queue_capacity;
    d.RQ = lp ? 1u : (uint64_t)d.S * d.R;  // quad stride: LP records contiguous (Lane::hrec)
    d.N = lp ? 1 : s->n_nodes;  // per-lane node arrays
    d.Ntot = s->n_nodes;
    d.lp0 = lp ? m.lp_begin : 0;
    d.IB = lpb ? 0u : m.inbox_cap;  // (batched: per-node caps, Dev::ib_off)
    d.out_cap = m.outbox_cap;
    d.lookahead = m.lookahead;
    d.L = s->n_links; d.D = s->link_depth; d.T = s->max_timeouts;
    d.n_insns = s->n_insns; d.n_consts = s->n_consts; d.n_sets = s->n_listener_sets; d.n_kinds = s->n_msg_kinds;
    d.horizon = s->near_horizon_us;
    d.Cr = s->run_capacity;
    if (lp) d.Cr = 0;  // LP nodes keep no far runs (tw_run_kernel<true> has no LDS for them)
    d.max_frames = s->max_frames ? s->max_frames : 2u;
    d.FXQ = d.max_frames > 2 ? (d.max_frames - 2 + 3) / 4 : 0u;
    d.tie_mode = TW_TIE_FIFO;
    d.sc_lp = lp ? 1u : 0u;  // LP lanes: one contiguous scalar block per lane (sc_ix)
    d.has_ph1 = plan.has_ph1 ? 1u : 0u;
    d.dpar = lp && !plan.has_ph1 ? 1u : 0u;  // (phase-1 lanes drain inside the window: one buffer)
    d.ib_total = lpb ? plan.ib_entries : (size_t)d.IB * d.R;
    c->tie_flags.assign(d.R, 0u);
    c->main_pc = s->main_pc;
    c->main_node = s->main_node;
    const size_t prog_lds = 16ull * (d.n_insns + 1) + 8ull * d.n_consts + 4ull * d.n_sets * d.n_kinds;
    c->geo = pick_geometry(lp, d.R, s->run_capacity, getenv("TW_GEOMETRY"), GeoSparse::LDS + prog_lds <= TW_LDS_LIMIT);
    const bool wave = c->geo == TW_GEO_WAVE;
    if (c->geo == TW_GEO_COMPACT) d.Cr = 0;  // far events: the HBM heap only
    if (wave) d.wave_k = (uint32_t)wave_near_k(d.R);
    // (the wave kernel reads the program image through the scalar cache)
    c->lds_bytes = wave ? 0 : with_geo(c, [](auto g) { return g.LDS; }) + prog_lds;
    if (c->lds_bytes > TW_LDS_LIMIT) return TW_ERR_INVALID;
    if (!wave) {
        hipError_t he = hipSuccess;
        with_geo(c, [&](auto g) {
            each_kernel<decltype(g)>([&](RunKernel k, Variant) {
                if (he == hipSuccess)
                    he = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)c->lds_bytes);
            });
        });
        HIPCHK(he);
    }
    return TW_OK;
}

// Stage "allocate": every table of the load, in one fixed order
static int load_alloc(tw_shard* c, const tw_scenario_desc* s, const LoadMode& m, const LpbPlan& plan, LoadTabs& t) {
    const bool lp = m.lp(), lpb = m.lpb(), wave = c->geo == TW_GEO_WAVE;
    Dev& d = c->d;
    const size_t R = d.R;
    const size_t Rt = s->n_replicas;  // replica dimension of the host tables
    const uint32_t rep_lg = d.rep_lg;
    Alloc A{c};
    A(t.insns, (size_t)d.n_insns + 1);  // +1 NOP: the fall-through prefetch may read one past
    A(t.consts, d.n_consts);
    A(t.lpc, (size_t)d.n_sets * d.n_kinds);
    A(t.out_off, (size_t)d.Ntot + 1);
    A(t.ldst, d.L);
    A(t.lrev, d.L);
    if (s->link_table) A(t.ltab, (size_t)d.L * d.D * Rt);
    A(d.scal, (size_t)(lp ? SC_LP_STRIDE : SC_COUNT) * R);
    A(d.slots, (size_t)d.S * R * 4);
    A(d.free_stk, (size_t)d.S * R);
    A(d.far, (size_t)d.Q * R);
    A(d.runs, (size_t)(d.Cr ? TW_RUNS * (size_t)d.Cr : 1) * R);
    A(d.near_spill, (size_t)(wave ? wave_spill_entries(d.wave_k) : with_geo(c, [](auto g) { return g.SPILL; })) * R);
    A(d.dummy, (size_t)TW_DUMMY_REC + R);
    A(d.nvars, (size_t)d.N * 4 * R);
    A(d.hash, (size_t)d.N * R);
    A(d.bind, (size_t)d.N * R);
    A(d.bind_own, (size_t)d.N * R);
    A(d.bind_rel, (size_t)d.N * R);
    A(d.link_ord, (size_t)(d.L ? d.L : 1) * (lp ? (size_t)1 << rep_lg : R));
    A(d.tmo_done, (size_t)(d.T ? d.T : 1) * R);
    A(d.n_active, 1);
    A(c->d_dev, 1);
    if (d.FXQ) A(d.fx, (size_t)d.S * R * d.FXQ);
    if (s->msg_bytes && s->link_bw && d.n_kinds && d.L) {
        A(t.mbytes, d.n_kinds);
        A(t.lbw, d.L);
    }
#ifdef TW_STATS
    A(d.prof, 2 * P_COUNT + TW_BPROF);
#endif
    if (lp) {
        if (plan.has_ph1) A(t.phd, plan.phase.size());
        const size_t ib_entries = d.ib_total;
        if (lpb) {
            A(t.iboff, plan.ib_off.size());
            A(d.spawn, (size_t)TW_SPN * R * 4);
            A(d.spawn_n, R);
        }
        A(d.hash_g, (size_t)d.Ntot << rep_lg);
        A(d.inbox, ib_entries * 2 * 2);  // two buffers (Dev::dpar)
        A(d.due, plan.heavy_ok ? ib_entries * 2 : 2);
        A(d.heavy, plan.heavy_ok ? 2 * R : 2);
        A(d.heavy_n, 2);
        if (lpb) A(d.bat_ctr, 2);
        A(d.pend_min, 1);
        A(d.inbox_n, 2 * R);
        A(d.outbox, (size_t)d.out_cap * 2);
        A(d.out_n, 1);
        A(d.next_t, 1);
        A(d.lp_err, 1);
        A(d.act, 2 * TW_LP_NB * R);
        A(d.act_n, 2 * TW_LP_NB);
        A(d.wake, R);
        A(d.listed, R);
        const size_t nsb = (R + (1u << TW_SUB_LG) - 1) >> TW_SUB_LG;
        A(d.sb_mark, nsb);
        A(d.sb_scan, nsb);
        A(d.sb_min, nsb);
        if (lpb) A(d.inlist, R);
        // per-replica windows (TW_LPB_GLOBAL=1: one window for the whole batch)
        if (lpb && !getenv("TW_LPB_GLOBAL")) {
            A(d.rw, (size_t)RW_COUNT << rep_lg);
            const size_t nk = ((R >> rep_lg) + (1u << TW_CHUNK_LG) - 1) >> TW_CHUNK_LG;
            A(d.cw_min, nk << rep_lg);
            A(d.cw_mark, nk << rep_lg);
        }
        A(c->lpm.foreign, (size_t)d.out_cap * 2);
        A(c->lpm.n_foreign, 1);
        A(c->lpm.staging, (size_t)d.out_cap * 2);
        A(c->ex.win_buf, WN_COUNT);  // d.win stays null: the host-driven loop
        A(c->ex.red_own, RD_COUNT);
    }
    if (s->main_regs && (!lp || lpb)) A(t.mregs, (size_t)s->n_replicas * 4);
    if (s->node_vars) A(t.nvi, (size_t)d.Ntot * 4);
    if (s->node_listen) A(t.lsi, (size_t)d.Ntot);
    if (lp) A(t.ldh, d.L ? d.L : 1);
    return A.rc;
}

// Stage "upload": the descriptor's tables and the plan's into the allocations,
// their pointers into Dev and the context
static int load_upload(tw_shard* c, const tw_scenario_desc* s, const LoadMode& m, const LpbPlan& plan,
                       const LoadTabs& t) {
    const bool lpb = m.lpb();
    Dev& d = c->d;
    const size_t Rt = s->n_replicas;
    hipStream_t st = c->stream;
#ifdef TW_STATS
    HIPCHK(hipMemsetAsync(d.prof, 0, 8 * (2 * P_COUNT + TW_BPROF), st));
#endif
    HIPCHK(hipMemsetAsync(t.insns, 0, sizeof(tw_insn) * (d.n_insns + 1), st));
    HIPCHK(hipMemcpyAsync(t.insns, s->insns, sizeof(tw_insn) * d.n_insns, hipMemcpyHostToDevice, st));
    if (d.n_consts) HIPCHK(hipMemcpyAsync(t.consts, s->consts, 8 * d.n_consts, hipMemcpyHostToDevice, st));
    if (d.n_sets) HIPCHK(hipMemcpyAsync(t.lpc, s->listener_pc, 4ull * d.n_sets * d.n_kinds, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(t.out_off, s->out_off, 4ull * (d.Ntot + 1), hipMemcpyHostToDevice, st));
    if (d.L) {
        HIPCHK(hipMemcpyAsync(t.ldst, s->link_dst, 4ull * d.L, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t.lrev, s->link_rev, 4ull * d.L, hipMemcpyHostToDevice, st));
    }
    if (t.ltab) HIPCHK(hipMemcpyAsync(t.ltab, s->link_table, 4ull * d.L * d.D * Rt, hipMemcpyHostToDevice, st));
    if (t.mregs) HIPCHK(hipMemcpyAsync(t.mregs, s->main_regs, 32ull * s->n_replicas, hipMemcpyHostToDevice, st));
    if (t.iboff) HIPCHK(hipMemcpy(t.iboff, plan.ib_off.data(), 4 * plan.ib_off.size(), hipMemcpyHostToDevice));
    if (t.phd) HIPCHK(hipMemcpy(t.phd, plan.phase.data(), plan.phase.size(), hipMemcpyHostToDevice));
    if (t.ldh) {
        // destination of every link with the heavy bit of its node (a send to a
        // heavy node goes through tw_lp_pack, to a light one straight in)
        std::vector<uint4> h_dh(d.L ? d.L : 1, make_uint4(0, 0, 0, 0));
        for (uint32_t l = 0; l < d.L; ++l) {
            const uint32_t n = s->link_dst[l];
            const uint32_t cap = lpb ? m.cap(n) : d.IB;
            const bool heavy = lpb && cap > TW_LIGHT;
            h_dh[l] = make_uint4(n | (heavy ? 0x80000000u : 0u), lpb ? plan.ib_off[n] : 0u, cap, 0u);
        }
        HIPCHK(hipMemcpy(t.ldh, h_dh.data(), 16 * h_dh.size(), hipMemcpyHostToDevice));
    }
    if (t.nvi) HIPCHK(hipMemcpyAsync(t.nvi, s->node_vars, 32ull * d.Ntot, hipMemcpyHostToDevice, st));
    if (t.lsi) HIPCHK(hipMemcpyAsync(t.lsi, s->node_listen, 4ull * d.Ntot, hipMemcpyHostToDevice, st));
    if (t.mbytes) {
        HIPCHK(hipMemcpyAsync(t.mbytes, s->msg_bytes, 4ull * d.n_kinds, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t.lbw, s->link_bw, 8ull * d.L, hipMemcpyHostToDevice, st));
    }
    d.insns = t.insns; d.consts = t.consts; d.lpc = t.lpc; d.out_off = t.out_off; d.link_dst = t.ldst; d.link_rev = t.lrev;
    d.link_table = t.ltab;
    d.ib_off = t.iboff;
    d.phase = t.phd;
    d.link_dsth = t.ldh;
    d.msg_bytes = t.mbytes;
    d.link_bw = t.lbw;
    c->main_regs = t.mregs;
    c->nv_init = t.nvi;
    c->listen_init = t.lsi;
    return TW_OK;
}

// a classifier's bytes as a device table
static int upload_bytes(tw_shard* c, const std::vector<uint8_t>& h, const uint8_t** out) {
    uint8_t* p = nullptr;
    int e = dalloc(c, &p, h.size());
    if (e) return e;
    HIPCHK(hipMemcpy(p, h.data(), h.size(), hipMemcpyHostToDevice));
    *out = p;
    return TW_OK;
}

// Stage "feature tables": the wave kernel's pc classes, tw_lp_due's batchable
// handlers, the sweeps' kill stubs, the prefix's T0
static int load_features(tw_shard* c, const tw_scenario_desc* s, const LoadMode& m) {
    Dev& d = c->d;
    if (c->geo == TW_GEO_WAVE) {
        std::vector<uint8_t> cls;
        classify_pcs(s, cls);
        int e = upload_bytes(c, cls, &d.pc_cls);
        if (e) return e;
    }
    if (m.lpb() && !c->lpm.has_ph1 && d.D == 1 && d.n_sets && !(getenv("TW_LP_BATCH") && getenv("TW_LP_BATCH")[0] == '0')) {
        std::vector<uint8_t> bat;
        classify_batch(s, bat);
        bool any = false;
        for (uint8_t x : bat) any = any || x;
        if (any) {
            int e = upload_bytes(c, bat, &d.lpc_bat);
            if (e) return e;
        }
    }
    if (far_run_geo(c) && d.Cr) {
        // kill stubs and their wake times (sweep_classify.hpp).
        // The scratch is optional: without it the context runs without sweeps
        SweepPlan plan = sweep_classify(s->insns, s->n_insns, s->consts, s->n_consts);
        uint32_t* stub = nullptr;
        uint32_t* acc = nullptr;
        unsigned long long* stats = nullptr;
        if (!plan.times.empty() && (c->sw.h || hipHostMalloc((void**)&c->sw.h, 8 * SWS_COUNT) == hipSuccess) &&
            dalloc(c, &stub, plan.stub.size()) == TW_OK && dalloc(c, &acc, sweep_acc_words(d.R)) == TW_OK &&
            dalloc(c, &stats, SWS_COUNT) == TW_OK) {
            HIPCHK(hipMemcpy(stub, plan.stub.data(), 4 * plan.stub.size(), hipMemcpyHostToDevice));
            HIPCHK(hipMemsetAsync(stats, 0, 8 * SWS_COUNT, c->stream));
            c->sw.tab.stub = stub;
            c->sw.tab.acc = acc;
            c->sw.tab.stats = stats;
            c->sw.tab.near_cap = TW_NEAR_CAP;
            c->sw.times = plan.times;
            c->sw.stub_h = plan.stub;
        } else {
            (void)hipGetLastError();  // (a failed allocation is not an error of the load)
        }
    }
    // the send-free prefix (prefix_classify.hpp): replica contexts only
    c->px.t0 = m.lp() ? 0 : prefix_t0(s->insns, s->n_insns, s->consts, s->n_consts, s->main_pc);
    // (an image that never sends ends inside its prefix: the pilot would run the
    // first workgroup's replicas to the end, without sweeps, and be refused)
    if (c->px.t0 == INT64_MAX) c->px.t0 = 0;
    return TW_OK;
}

// the stages behind the unload
static int load_stages(tw_shard* c, const tw_scenario_desc* s, const LoadMode& m, const LpbPlan& plan) {
    if (plan.status) return plan.status;
    LoadTabs t;
    int rc = load_describe(c, s, m, plan);
    if (!rc) rc = load_alloc(c, s, m, plan, t);
    if (!rc) rc = load_upload(c, s, m, plan, t);
    if (!rc) rc = load_features(c, s, m);
    if (rc) return rc;
    c->loaded = true;
    rc = sh_reset(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return TW_OK;
}

// A refusal of the descriptor or of the mode's arguments leaves the previous
// load as it is; from the unload on, every failure leaves the context unloaded.
static int load_common(tw_shard* c, const tw_scenario_desc* s, LoadMode m) {
    if (!c) return TW_ERR_INVALID;
    int v = validate(s);
    if (!v) v = load_mode_check(s, m, LOAD_LIMITS);
    if (v) return v;
    const LpbPlan plan = m.lpb() ? lpb_plan(s, m, LOAD_LIMITS) : LpbPlan{};
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    free_all(c);
    const int rc = load_stages(c, s, m, plan);
    if (rc) free_all(c);
    return rc;
}

int sh_load(tw_shard* c, const tw_scenario_desc* s) { return load_common(c, s, LoadMode{}); }

int sh_lp_load(tw_shard* c, const tw_scenario_desc* s, uint32_t lp_begin, uint32_t lp_count, int64_t lookahead_us,
               uint32_t inbox_cap, uint32_t outbox_cap) {
    LoadMode m;
    m.kind = LoadMode::NODES;
    m.lp_begin = lp_begin; m.lp_count = lp_count;
    m.lookahead = lookahead_us; m.inbox_cap = inbox_cap; m.outbox_cap = outbox_cap;
    return load_common(c, s, m);
}

int sh_lpb_load(tw_shard* c, const tw_scenario_desc* s, int64_t lookahead_us, const uint32_t* node_inbox_cap,
                uint32_t inbox_cap, uint32_t outbox_cap) {
    LoadMode m;
    m.kind = LoadMode::BATCHED;
    m.lookahead = lookahead_us; m.inbox_cap = inbox_cap; m.outbox_cap = outbox_cap;
    m.node_caps = node_inbox_cap;
    return load_common(c, s, m);
}

int sh_reset(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    const Dev& d = c->d;
    const size_t R = d.R;
    hipStream_t st = c->stream;
    c->sw.done = 0;
    HIPCHK(hipMemsetAsync(d.nvars, 0, 32ull * d.N * R, st));
    HIPCHK(hipMemsetAsync(d.hash, 0, 8ull * d.N * R, st));
    HIPCHK(hipMemsetAsync(d.bind, 0, 4ull * d.N * R, st));
    HIPCHK(hipMemsetAsync(d.link_ord, 0, 4ull * (d.L ? d.L : 1) * (c->lpm.lp ? (size_t)1 << d.rep_lg : R), st));
    HIPCHK(hipMemsetAsync(d.tmo_done, 0, (size_t)(d.T ? d.T : 1) * R, st));
    if (c->lpm.lp) {
        HIPCHK(hipMemsetAsync(d.hash_g, 0, 8ull * ((size_t)d.Ntot << d.rep_lg), st));
        HIPCHK(hipMemsetAsync(d.heavy_n, 0, 8, st));
        if (d.bat_ctr) HIPCHK(hipMemsetAsync(d.bat_ctr, 0, 16, st));
        if (d.trace_n) HIPCHK(hipMemsetAsync(d.trace_n, 0, 8ull * c->lpm.n_rep, st));
        if (d.inlist) HIPCHK(hipMemsetAsync(d.inlist, 0, 4ull * R, st));
        HIPCHK(hipMemsetAsync(d.pend_min, 0xFF, 8, st));
        HIPCHK(hipMemsetAsync(d.out_n, 0, 4, st));
        HIPCHK(hipMemsetAsync(d.lp_err, 0, 4, st));
        HIPCHK(hipMemsetAsync(c->lpm.n_foreign, 0, 4, st));
        c->d.act_cur = 0;
        c->d.wid = 0;
        HIPCHK(hipMemsetAsync(d.act_n, 0, 8 * TW_LP_NB, st));
        c->lpm.fresh = c->lpm.lpb;
        c->lpm.trace_bat_run = c->lpm.trace_bat;  // (tw_set_trace_batch: from this reset on)
    }
    if (d.pq_hdr) {
        // empty MinQueues: no element, no node used, every rank a Skip
        std::vector<uint32_t> h((size_t)R * PQ_WORDS, 0u);
        for (size_t r = 0; r < R; ++r)
            for (int k = 0; k < 32; ++k) h[r * PQ_WORDS + PQ_FOREST + k] = 0xFFFFFFFFu;
        HIPCHK(hipMemcpyAsync(d.pq_hdr, h.data(), 4 * h.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    uint32_t blocks = (uint32_t)((R + TW_WG - 1) / TW_WG);
    hipLaunchKernelGGL(tw_init_kernel, dim3(blocks), dim3(TW_WG), 0, st, d, c->main_pc, c->main_node,
                       (const int64_t*)c->main_regs, (const int64_t*)c->nv_init, (const uint32_t*)c->listen_init,
                       c->lpm.lp ? 1 : 0, c->seq0, c->tid0);
    HIPCHK(hipGetLastError());
    if (d.live_gen) {  // every replica's generator back to mkStdGen(seed_base + its index)
        hipLaunchKernelGGL(tw_live_seed_kernel, dim3(blocks), dim3(TW_WG), 0, st, d, c->lv_seed0);
        HIPCHK(hipGetLastError());
    }
    c->px.fresh = true;
    return TW_OK;
}

// tw_set_live_delays on one shard: desc = live_plan's descriptors of the
// loaded scenario's links (null: off), seed0 = the seed of the shard's first
// replica.  Seeds the generators, as the next sh_reset will again.
static_assert(sizeof(LiveLink) == sizeof(uint4), "a SEND loads a link's descriptor as one quad");
int sh_set_live(tw_shard* c, const LiveLink* desc, int64_t seed0) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (c->lpm.lp) return TW_ERR_INVALID;  // (a replica's nodes run in parallel: no execution order to draw in)
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    if (!desc) {
        d.live_desc = nullptr; d.live_gen = nullptr; d.live_n = nullptr;
        return TW_OK;
    }
    if (!c->lv_desc) {
        uint4* ld = nullptr;
        uint2* lg = nullptr;
        uint32_t* ln = nullptr;
        unsigned long long* ls = nullptr;
        Alloc A{c};
        A(ld, d.L);
        A(lg, d.R);
        A(ln, d.R);
        A(ls, 1);
        if (A.rc) return A.rc;  // (what was allocated goes with the load)
        c->lv_desc = ld; c->lv_gen = lg; c->lv_n = ln; c->lv_sum = ls;
    }
    HIPCHK(hipStreamSynchronize(c->stream));  // (a run in flight reads the descriptors)
    if (d.L) HIPCHK(hipMemcpy(c->lv_desc, desc, 16ull * d.L, hipMemcpyHostToDevice));
    d.live_desc = c->lv_desc; d.live_gen = c->lv_gen; d.live_n = c->lv_n;
    c->lv_seed0 = seed0;
    hipLaunchKernelGGL(tw_live_seed_kernel, dim3((uint32_t)((d.R + TW_WG - 1) / TW_WG)), dim3(TW_WG), 0, c->stream, d,
                       seed0);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

// the shard's generator steps since the last reset (0: live delays off)
int sh_live_stats(tw_shard* c, uint64_t* draws) {
    if (!c || !draws) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    *draws = 0;
    const Dev& d = c->d;
    if (!d.live_n) return TW_OK;
    HIPCHK(hipSetDevice(c->device));
    unsigned long long h = 0;
    HIPCHK(hipMemsetAsync(c->lv_sum, 0, 8, c->stream));
    hipLaunchKernelGGL(tw_live_sum_kernel, dim3((uint32_t)((d.R + TW_WG - 1) / TW_WG)), dim3(TW_WG), 0, c->stream, d,
                       c->lv_sum);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, c->lv_sum, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *draws = h;
    return TW_OK;
}


static int lpb_run(tw_shard* c, tw_stats* out);

// one launch of the context's event kernel to t_end (grid: launch_run)
static int launch_event(tw_shard* c, hipStream_t st, int64_t t_end, uint64_t limit, uint32_t budget, uint32_t grid = 0) {
    if (c->geo == TW_GEO_WAVE)
        HIPCHK(wave_launch(c->d, c->d_dev, st, t_end, limit, 1u << 16));
    else
        with_geo(c, [&](auto g) { launch_run<decltype(g)>(c, st, t_end, limit, budget, grid); });
    HIPCHK(hipGetLastError());
    return TW_OK;
}

// A sweep time T of the image (Sweep::times[ix]) that lies within the run
struct Stop { int64_t T; uint32_t ix; };
// ... and, as the stop ahead of a round: the run's segment it ends, the run's own end
// clean: the kill table is this stop's (Prefix::Snap::Clean) and the replicas derive from its snapshot
struct SweepAt { int64_t T, run_end; uint32_t seg; bool clean; };

// One round of tw_run: n launches of the event kernel to t_end, each behind a
// cleared n_active and timed; with a sweep stop ahead, each followed by the
// sweep kernels, timed as a step of their own (fired or not: their time is
// listed behind their launch's, `launches` counts the event kernel's).  Then
// the host's check: n_active and the sweeps' words copied, the stream
// synchronised, the times read (LaunchTimes: in the order recorded).
static int run_round(tw_shard* c, int n, int64_t t_end, uint64_t limit, uint32_t budget, uint32_t grid,
                     const SweepAt* sw, uint32_t* launches) {
    const Dev& d = c->d;
    hipStream_t st = c->stream;
    const Prefix::Snap::Clean& cl = c->px.snap.clean;
    for (int i = 0; i < n; ++i) {
        HIPCHK(hipMemsetAsync(d.n_active, 0, 4, st));
        if (c->lpm.lp) HIPCHK(hipMemsetAsync(d.next_t, 0xFF, 8, st));
        int rc = c->times.timed(st, [&]() -> int { return launch_event(c, st, t_end, limit, budget, grid); });
        if (rc) return rc;
        ++*launches;
        if (!sw) continue;
        rc = c->times.timed(st, [&]() -> int {
            tw::SweepTab tab = c->sw.tab;
            if (sw->clean) {
                tab.kill = cl.kill; tab.kwin = cl.kwin; tab.dirty = cl.dirty; tab.cflags = cl.cflags;
                if (cl.bits && !c->sw.slow) {
                    tab.eff = cl.eff; tab.bits = cl.bits; tab.excl = cl.excl ? 1u : 0u;
                }
            }
            HIPCHK(sweep_launch(d, tab, st, sw->T, limit, sw->run_end, sw->seg));
            return TW_OK;
        }, &c->sw.ms);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(c->h_active, d.n_active, 4, hipMemcpyDeviceToHost, st));
    if (sw) HIPCHK(hipMemcpyAsync(c->sw.h, c->sw.tab.stats, 8 * SWS_COUNT, hipMemcpyDeviceToHost, st));
    // (the dirty bytes and the flag words lie behind one another)
    if (sw && sw->clean) HIPCHK(hipMemcpyAsync(cl.h, cl.dirty, cl.S + 4 * CF_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return c->times.read();
}

// Rows later applies may skip, for the snapshot just taken: the
// kill table of the image's last sweep time from the snapshot's own bytes, the
// claimed slots' row tags, cleared dirty bytes and flag words, in one device
// block.  Optional: without a sweep time behind the prefix, a claimable
// position or the memory, every apply stores every row, as before.
//
// And every row's class (§3v): with the table, the claimed slots' header rows
// and the claimable positions' run entries; with or without it, the rows that
// hold what tw_reset leaves (the reset values read back from the load's own
// device copies).  The classes and the audit's count are a block of their own.
static int build_clean(tw_shard* c, const std::vector<tw::PrefixRow>& rows, const uint64_t* sc) {
    const Dev& d = c->d;
    hipStream_t st = c->stream;
    Prefix::Snap& sn = c->px.snap;
    const bool table = c->sw.tab.stub && !c->sw.times.empty() && c->sw.stub_h.size() == (size_t)d.n_insns + 1 &&
                       c->sw.times.back() > c->px.t0 - 1;
    const uint32_t stop = table ? (uint32_t)c->sw.times.size() - 1u : 0u;
    const int64_t T = table ? c->sw.times[stop] : 0;
    std::vector<uint8_t> snap(sn.bytes);
    std::vector<int64_t> nvi(c->nv_init ? 4ull * d.N : 0);
    std::vector<uint32_t> lsi(c->listen_init ? d.N : 0);
    HIPCHK(hipMemcpyAsync(snap.data(), sn.tab.snap, sn.bytes, hipMemcpyDeviceToHost, st));
    if (!nvi.empty()) HIPCHK(hipMemcpyAsync(nvi.data(), c->nv_init, 8 * nvi.size(), hipMemcpyDeviceToHost, st));
    if (!lsi.empty()) HIPCHK(hipMemcpyAsync(lsi.data(), c->listen_init, 4 * lsi.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const tw::CleanLayout L = tw::clean_layout(d);
    tw::CleanPlan plan;
    if (table)
        plan = tw::clean_build(L, rows.data(), rows.size(), snap.data(), snap.size(), sc + SC_RH0, sc + SC_RC0,
                               c->sw.stub_h.data(), T);
    // what sh_reset's memsets and tw_init_kernel leave in a replica context
    const tw::ResetLayout rs{(uint64_t)(uintptr_t)d.nvars, (uint64_t)(uintptr_t)d.hash, (uint64_t)(uintptr_t)d.bind,
                             (uint64_t)(uintptr_t)d.bind_own, (uint64_t)(uintptr_t)d.bind_rel,
                             (uint64_t)(uintptr_t)d.tmo_done, d.N, d.T, nvi.empty() ? nullptr : nvi.data(),
                             lsi.empty() ? nullptr : lsi.data(), 0xFFFFFFFFu, 0xFFFFFFFEu};
    tw::RowClasses rc = tw::clean_classes(L, rows.data(), rows.size(), snap.data(), snap.size(), plan, &rs);
    if (!c->px.rows_on)  // (TW_TEST_PREFIX_ROWS=0: the rows of §3o alone)
        for (size_t i = 0; i < rc.cls.size(); ++i)
            if (rc.cls[i] > tw::RC_BODY) {
                --rc.n[rc.cls[i]]; ++rc.n[tw::RC_NONE];
                rc.bytes[rc.cls[i]] -= rows[i].es; rc.bytes[tw::RC_NONE] += rows[i].es;
                rc.cls[i] = tw::RC_NONE;
                rc.tag[i] = tw::PCL_NO_SLOT;
            }
    {   // the audit's counts, the list's count, the list (a pair per row and span), the classes
        uint64_t pairs[tw::RC_COUNT] = {0, 0, 0, 0, 0}, all = 0;
        for (size_t i = 0; i < rows.size(); ++i) pairs[rc.cls[i]] += tw::prefix_row_spans(rows[i].dst, rows[i].es, d.R);
        for (uint64_t p : pairs) all += p;
        const bool list = c->px.list_on && c->px.rows_on && all <= 0x7FFFFFFFull;  // (TW_TEST_PREFIX_ROWS=0: as §3o had it)
        const size_t o_cls = 64 + (list ? 8 * (size_t)all : 0);  // (the counts: RC_COUNT words, then the list's)
        void* blk = nullptr;
        if (hipMalloc(&blk, o_cls + rc.cls.size()) != hipSuccess) {
            (void)hipGetLastError();  // (no memory: no skipping, not an error of the run)
            return TW_OK;
        }
        HIPCHK(hipMemset(blk, 0, 64));
        HIPCHK(hipMemcpy((uint8_t*)blk + o_cls, rc.cls.data(), rc.cls.size(), hipMemcpyHostToDevice));
        sn.audit = (unsigned long long*)blk;
        sn.cls = (const uint8_t*)blk + o_cls;
        if (list) {
            sn.tab.list_n = (uint32_t*)((uint8_t*)blk + 48);
            sn.tab.list = (uint2*)((uint8_t*)blk + 64);
            sn.tab.list_cap = (uint32_t)all;
        }
        for (int k = 0; k < tw::RC_COUNT; ++k) {
            sn.class_rows[k] = rc.n[k]; sn.class_bytes[k] = rc.bytes[k]; sn.class_pairs[k] = pairs[k];
        }
        sn.pairs16 = tw::prefix_row_spans(0, 16, d.R);
    }
    if (plan.slots.empty()) return TW_OK;
    const std::vector<uint32_t>& tag = rc.tag;
    const tw::CleanEffects fx = tw::clean_effects(L, rows.data(), rows.size(), snap.data(), snap.size(),
                                                  c->sw.stub_h.data(), plan);
    const size_t S4 = ((size_t)d.S + 3u) & ~(size_t)3u;
    const size_t o_win = sizeof(tw::KillEnt) * plan.ents.size(), o_tag = o_win + sizeof(tw::KillWin) * TW_RUNS,
                 o_dirty = o_tag + 4 * tag.size(),
                 o_eff = (o_dirty + S4 + 4 * CF_COUNT + 15u) & ~(size_t)15u,
                 total = o_eff + sizeof(tw::EffEnt) * fx.eff.size();
    Prefix::Snap::Clean& cl = sn.clean;
    if (hipMalloc(&cl.dev, total) != hipSuccess || hipHostMalloc((void**)&cl.h, S4 + 4 * CF_COUNT) != hipSuccess) {
        (void)hipGetLastError();  // (no memory: no skipping, not an error of the run)
        if (cl.dev) (void)hipFree(cl.dev);
        cl = Prefix::Snap::Clean{};
        return TW_OK;
    }
    uint8_t* b = (uint8_t*)cl.dev;
    HIPCHK(hipMemset(b, 0, total));
    {   // (the table with its positions' verdict bits, §3t)
        std::vector<tw::KillEnt> ents = plan.ents;
        for (size_t i = 0; i < ents.size() && !c->sw.frames; ++i)
            ents[i].pad = (fx.eff[i].flags & tw::EFF_VERDICT) ? tw::KILL_VERDICT : 0u;
        HIPCHK(hipMemcpy(b, ents.data(), o_win, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(b + o_win, plan.win.data(), sizeof(tw::KillWin) * TW_RUNS, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b + o_tag, tag.data(), 4 * tag.size(), hipMemcpyHostToDevice));
    std::memset(cl.h, 0, S4 + 4 * CF_COUNT);
    cl.kill = (const tw::KillEnt*)b;
    cl.kwin = (const tw::KillWin*)(b + o_win);
    cl.tag = (const uint32_t*)(b + o_tag);
    cl.dirty = b + o_dirty;
    cl.cflags = (uint32_t*)(b + o_dirty + S4);
    for (size_t i = 0; i < rc.cls.size(); ++i) {  // (for the host's count of what an apply skips)
        if (rc.cls[i] == tw::RC_HDR) cl.hdr_tags.push_back(rc.tag[i]);
        if (rc.cls[i] == tw::RC_RUN) cl.run_tags.push_back(rc.tag[i]);
    }
    // the effects rows, and a clean bit per table position and replica: without
    // the memory the sweep applies every entry the general way
    HIPCHK(hipMemcpy(b + o_eff, fx.eff.data(), sizeof(tw::EffEnt) * fx.eff.size(), hipMemcpyHostToDevice));
    cl.eff = (const tw::EffEnt*)(b + o_eff);
    cl.excl = fx.exclusive;
    const size_t bits = 8ull * plan.ents.size() * ((d.R + 63u) / 64u);
    if (hipMalloc((void**)&cl.bits, bits) != hipSuccess) {
        (void)hipGetLastError();
        cl.bits = nullptr;
    } else {
        HIPCHK(hipMemset(cl.bits, 0, bits));
    }
    cl.S = (uint32_t)S4;
    cl.stop = stop;
    cl.slots = plan.slots;
    return TW_OK;
}

// The send-free prefix of a fresh run.  With a snapshot cached
// for the context's tie mode and counter bases, its apply goes onto the stream,
// timed (read at the caller's first round: the list's next entry).  Without
// one, the first workgroup alone runs to T0 - 1 -- the pilot: the ordinary
// run's rounds on a grid of one, no sweeps behind them --, replica 0 is
// checked to have run as every replica must (still running, under the event
// cap, no message counted, no send ordinal taken), its parked state becomes
// the snapshot and is applied to every replica, the pilot's own included.  A
// pilot that fails the check is remembered as "no prefix" for the key; its
// replicas are simply ahead of the others and the run goes on as ever.
// *applied: the apply is on the stream.
static int run_prefix(tw_shard* c, uint64_t limit, uint32_t budget, bool verified, uint32_t* launches, bool* applied) {
    const Dev& d = c->d;
    hipStream_t st = c->stream;
    Prefix& px = c->px;
    *applied = false;
    const bool hit = px.snap.have && px.snap.tie == d.tie_mode && px.snap.seq0 == c->seq0 && px.snap.tid0 == c->tid0;
    if (hit && !px.snap.ok) { px.last = TW_PREFIX_REFUSED; return TW_OK; }
    if (hit && limit < px.snap.events) return TW_OK;  // (the cap falls inside the prefix: the ordinary run)
    if (!hit) {
        HIPCHK(hipStreamSynchronize(st));
        px.drop();
        px.snap.have = true;
        px.snap.tie = d.tie_mode; px.snap.seq0 = c->seq0; px.snap.tid0 = c->tid0;
        px.last = TW_PREFIX_REFUSED;
        bool parked = false;
        for (int round = 0; round < (1 << 20) && !parked; ++round) {
            int rc = run_round(c, 4, px.t0 - 1, limit, budget, 1u, nullptr, launches);
            if (rc) return rc;
            parked = *c->h_active == 0;
        }
        if (!parked) return TW_OK;
        // replica 0's scalar block; with D > 1 its send ordinals
        uint64_t sc[SC_COUNT];
        HIPCHK(hipMemcpy2DAsync(sc, 8, d.scal, 8ull * d.R, 8, SC_COUNT, hipMemcpyDeviceToHost, st));
        std::vector<uint32_t> ord(d.D > 1 ? d.L : 0u);
        if (!ord.empty())
            HIPCHK(hipMemcpy2DAsync(ord.data(), 4, d.link_ord, 4ull * d.R, 4, ord.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool ok = sc[SC_STATUS] == TW_REP_RUNNING && sc[SC_EVENTS] < limit && sc[SC_DELIVERED] == 0 &&
                  sc[SC_DROPPED] == 0 && sc[SC_UNDELIV] == 0;
        for (uint32_t o : ord) ok = ok && o == 0;
        std::vector<tw::PrefixRow> rows;
        size_t bytes = 0;
        if (!ok || !prefix_directory(d, sc, TW_NEAR_CAP, rows, bytes)) return TW_OK;
        void *drows = nullptr, *dsnap = nullptr;
        if (hipMalloc(&drows, sizeof(tw::PrefixRow) * rows.size()) != hipSuccess ||
            hipMalloc(&dsnap, bytes ? bytes : 1) != hipSuccess) {
            (void)hipGetLastError();  // (no memory for the snapshot: no prefix, not an error of the run)
            if (drows) (void)hipFree(drows);
            return TW_OK;
        }
        px.snap.tab.rows = (const tw::PrefixRow*)drows;
        px.snap.tab.snap = (uint8_t*)dsnap;
        px.snap.tab.n_rows = (uint32_t)rows.size();
        HIPCHK(hipMemcpy(drows, rows.data(), sizeof(tw::PrefixRow) * rows.size(), hipMemcpyHostToDevice));
        uint32_t mx = 0;
        for (const tw::PrefixRow& r : rows) mx = r.es > mx ? r.es : mx;
        px.snap.max_es = mx;
        px.snap.events = sc[SC_EVENTS];
        px.snap.bytes = bytes;
        HIPCHK(prefix_take(px.snap.tab, st));
        px.snap.ok = true;
        int rc = build_clean(c, rows, sc);
        if (rc) return rc;
    }
    // Rows the last run's sweep proved unwritten are left as they are (§3o):
    // `skip` is the host's side of the validity rule, CF_VALID the device's.
    // The flags are consumed: cleared behind the apply, inside its timed pair.
    const Prefix::Snap::Clean& cl = px.snap.clean;
    // §3v: a cached apply is the first device work behind tw_reset (run_prefix
    // is a fresh tw_run's, and no call between the two writes the arrays
    // tw_reset fills), so the rows that hold tw_reset's values stay as they
    // are, verified or not; the pilot's apply stores everything.
    const bool skip = hit && cl.dev && px.snap.cls && verified;
    const bool rst = hit && px.snap.cls && px.snap.class_rows[tw::RC_RESET] != 0;
    tw::PrefixTab tab = px.snap.tab;
    px.rows_skipped = 0;
    px.rows = Prefix::Rows{};
    if (skip || rst) tab.cls = px.snap.cls;
    tab.reset = rst ? 1u : 0u;
    if (skip) {
        tab.tag = cl.tag; tab.dirty = cl.dirty; tab.cflags = cl.cflags;
        const uint32_t* hf = (const uint32_t*)(cl.h + cl.S);
        if (hf[CF_VALID] == 1u) {
            for (uint32_t s : cl.slots) px.rows_skipped += cl.h[s] ? 0u : 3u;
            for (uint32_t s : cl.run_tags) px.rows.n[1] += cl.h[s] ? 0u : 1u;
            if (hf[CF_HDR_OK] == 1u)
                for (uint32_t s : cl.hdr_tags) px.rows.n[0] += cl.h[s] ? 0u : 1u;
        }
    }
    if (rst) px.rows.n[2] = px.snap.class_rows[tw::RC_RESET];
    px.rows.bytes[0] = 16u * px.rows.n[0];
    px.rows.bytes[1] = 16u * px.rows.n[1];
    px.rows.bytes[2] = rst ? px.snap.class_bytes[tw::RC_RESET] : 0u;
    px.bytes_stored = px.snap.bytes - 16u * px.rows_skipped;
    px.rows.stored = px.bytes_stored - px.rows.bytes[0] - px.rows.bytes[1] - px.rows.bytes[2];
    // the compact form's grid: the pairs of the rows this apply stores, as the host counts them
    uint64_t pairs = 0;
    for (uint64_t p : px.snap.class_pairs) pairs += p;
    pairs -= px.snap.pairs16 * (px.rows_skipped + px.rows.n[0] + px.rows.n[1]) +
             (rst ? px.snap.class_pairs[tw::RC_RESET] : 0u);
    px.rows.form = (tab.list && tab.cls) ? 2u : 1u;
    px.rows.pairs = px.rows.form == 2u ? pairs : 0u;
    int rc = c->times.timed(st, [&]() -> int {
        HIPCHK(prefix_apply(tab, d.R, px.snap.max_es, (uint32_t)pairs, st));
        if (tab.cls && px.audit) {
            HIPCHK(hipMemsetAsync(px.snap.audit, 0, 8 * tw::RC_COUNT, st));
            HIPCHK(prefix_audit(tab, d.R, px.snap.max_es, px.snap.audit, st));
            px.audited = true;
        }
        if (cl.dev) HIPCHK(hipMemsetAsync(cl.dirty, 0, cl.S + 4 * CF_COUNT, st));
        return TW_OK;
    }, &px.ms);
    if (rc) return rc;
    px.last = hit ? TW_PREFIX_APPLIED : TW_PREFIX_PILOTED;
    *applied = true;
    return TW_OK;
}

// tw_run's statistics: reduced on the device from the events column taken at
// the run's start (tw_stats_kernel), with the run's launches and times
static int reduce_stats(tw_shard* c, uint32_t launches, std::chrono::steady_clock::time_point w0, tw_stats* out) {
    const Dev& d = c->d;
    hipStream_t st = c->stream;
    std::memset(out, 0, sizeof(*out));
    HIPCHK(hipMemsetAsync(c->st.out, 0, 64, st));
    hipLaunchKernelGGL(tw_stats_kernel, dim3((uint32_t)((d.R + 255) / 256)), dim3(256), 0, st, d,
                       (const uint64_t*)c->st.ev0, c->st.out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->st.h, c->st.out, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const unsigned long long* h = c->st.h;
    out->events = h[0];
    out->delivered = h[1];
    out->dropped = h[2];
    out->undeliverable = h[3];
    out->max_final_t = (int64_t)h[4];
    out->replicas_done = (uint32_t)h[5];
    out->replicas_error = (uint32_t)h[6];
    out->sends = out->delivered + out->dropped + out->undeliverable;
    out->launches = launches;
    out->kernel_ms = c->times.total;
    out->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    return TW_OK;
}

// tw_run: take the prefix, plan the sweep stops, run rounds until every
// replica is quiet, reduce the statistics.
int sh_run(tw_shard* c, int64_t t_end_us, uint64_t max_events, tw_stats* out) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    const bool was_fresh = c->px.fresh;
    c->px.fresh = false;
    c->px.last = TW_PREFIX_NOT_ELIGIBLE;
    c->px.ms = 0.0;
    // §3o: what the last run verified serves this run's apply alone; the
    // replicas derive from an apply only if this run, fresh, makes one
    const bool verified = c->px.verified && was_fresh;
    c->px.verified = c->px.last_verified = false;
    if (was_fresh) c->px.chain = false;
    c->px.rows_skipped = c->px.bytes_stored = 0;
    c->px.rows = Prefix::Rows{};
    c->px.audited = false;
    if (c->lpm.lpb) {
        // the batched window loop runs every replica to quiescence
        if (t_end_us != INT64_MAX || max_events != UINT64_MAX) return TW_ERR_INVALID;
        return lpb_run(c, out);
    }
    auto w0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const Dev& d = c->d;
    // events before this call (to report per-call deltas; only when asked
    // for: an LP window would otherwise copy 8 B per node every window)
    // (a device-side copy of the events column; tw_stats_kernel reduces the
    // run's statistics on the device at the end)
    if (out) {
        if (!c->st.ev0) HIPCHK(hipMalloc((void**)&c->st.ev0, 8ull * (d.R ? d.R : 1)));
        if (!c->st.out) HIPCHK(hipMalloc((void**)&c->st.out, 64));
        if (!c->st.h) HIPCHK(hipHostMalloc((void**)&c->st.h, 64));
        if (d.sc_lp)  // (the events word of every lane's block: one strided copy)
            HIPCHK(hipMemcpy2DAsync(c->st.ev0, 8, d.scal + SC_EVENTS, 8ull * SC_LP_STRIDE, 8, d.R,
                                    hipMemcpyDeviceToDevice, st));
        else
            HIPCHK(hipMemcpyAsync(c->st.ev0, d.scal + (size_t)SC_EVENTS * d.R, 8ull * d.R, hipMemcpyDeviceToDevice,
                                  st));
    }
    const uint64_t limit = max_events;  // cumulative per-replica cap
    c->times.start();
    if (c->lpm.lp) {
        // a new window: serve the list built since the last call (nodes with a
        // live thread or new records); start an empty one for the next call
        c->d.act_cur ^= 1u;
        HIPCHK(hipMemsetAsync(d.act_n + c->d.act_cur * TW_LP_NB, 0, 4 * TW_LP_NB, st));
        hipLaunchKernelGGL(tw_lp_compact, dim3(compact_blocks(d.R)), dim3(256), 0, st, c->d, c->d.wid, c->d.act_cur);
        HIPCHK(hipGetLastError());
        c->d.wid += 1u;
    }
    // loop iterations (pops) per lane per launch: bounded kernel time
    static const uint32_t budget = [] {
        const char* b = getenv("TW_LAUNCH_BUDGET");
        const long v = b ? strtol(b, nullptr, 10) : 0;
        return v >= 1 && v <= (1L << 24) ? (uint32_t)v : (1u << 14);
    }();
    // launches between host checks: a replica run needs several budgets; an LP
    // window is almost always done after one launch
    const int per_check = c->lpm.lp ? 1 : 4;
    uint32_t launches = 0;
    const bool swept_order = far_run_geo(c) && ordered_ties(c);
    // the send-free prefix: a fresh replica run that reaches T0 - 1
    // starts from the snapshot of that moment instead of popping its way there
    if (was_fresh && c->px.on && swept_order && d.trace_cap == 0 && !c->main_regs && c->px.t0 >= 1 &&
        t_end_us >= c->px.t0 - 1) {
        bool applied = false;
        int rc = run_prefix(c, limit, budget, verified, &launches, &applied);
        if (rc) return rc;
        c->px.chain = applied;
        // (sweep times inside the prefix: the snapshot is past them)
        if (applied)
            for (uint32_t i = 0; i < c->sw.times.size(); ++i)
                if (c->sw.times[i] <= c->px.t0 - 1) c->sw.done |= 1u << i;
    }
    // killThread sweeps: the run is split at every sweep time T of
    // the image that lies within it.  While such a stop is ahead, the event
    // kernel runs to T - 1 (its "parked beyond t_end" path) and every launch is
    // followed by the sweep kernels, which fire once, on the device's own
    // evidence: behind the launch that left every replica parked.  They carry
    // out the kill wakes and victim pops at T of every replica that qualifies;
    // replicas they refuse pop them one by one when the event kernel goes on.
    // No launch and no host round trip is added to a run whose replicas all
    // end in the sweep (C3): the segment's remaining launches find nothing to
    // do, and the sweep reports that no replica has work left.
    std::vector<Stop> stops;
    c->sw.last[0] = c->sw.last[1] = c->sw.last[2] = 0;
    c->sw.path[0] = c->sw.path[1] = 0;
    c->sw.ms = 0.0;
    if (c->sw.on && c->sw.tab.stub && swept_order) {
        for (uint32_t i = 0; i < c->sw.times.size(); ++i) {
            const int64_t T = c->sw.times[i];
            if (T >= 1 && T <= t_end_us && !((c->sw.done >> i) & 1u)) stops.push_back(Stop{T, i});
        }
        if (!stops.empty()) HIPCHK(hipMemsetAsync(c->sw.tab.stats, 0, 8 * SWS_COUNT, st));
    }
    bool quiet = false, checked = false;
    size_t seg = 0;
    const Prefix::Snap::Clean& cl = c->px.snap.clean;
    for (int round = 0; round < (1 << 20) && !quiet; ++round) {
        const bool to_sweep = seg < stops.size();
        // the kill table's stop, over replicas that derive from its snapshot (§3o)
        const bool clean = to_sweep && c->px.chain && c->px.snap.ok && cl.dev && stops[seg].ix == cl.stop;
        const SweepAt at{to_sweep ? stops[seg].T : 0, t_end_us, (uint32_t)seg, clean};
        int rc = run_round(c, per_check, to_sweep ? at.T - 1 : t_end_us, limit, budget, 0, to_sweep ? &at : nullptr,
                           &launches);
        if (rc) return rc;
        if (!to_sweep) {
            quiet = *c->h_active == 0;
        } else if (c->sw.h[SWS_FIRED] > seg) {
            c->sw.done |= 1u << stops[seg].ix;
            for (int k = 0; k < 3; ++k) c->sw.last[k] = c->sw.h[k];
            c->sw.path[0] = c->sw.h[SWS_TERM]; c->sw.path[1] = c->sw.h[SWS_FAST];
            checked = checked || clean;
            ++seg;
            // the last stop swept and no replica has work left before t_end: done
            quiet = seg == stops.size() && c->sw.h[SWS_LEFT] == 0;
        }
    }
    if (out) {
        int rc = reduce_stats(c, launches, w0, out);
        if (rc) return rc;
    }
    // the sweep at the table's time fired, checked every replica and left none
    // with work: the next apply may skip what it did not mark (§3o)
    if (quiet && checked && ((const uint32_t*)(cl.h + cl.S))[CF_VALID] != 0u)
        c->px.verified = c->px.last_verified = true;
    return quiet ? TW_OK : TW_ERR_INCOMPLETE;
}

int sh_read_results(tw_shard* c, tw_replica_result* out, size_t n) {
    if (!c || !out) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    const Dev& d = c->d;
    if (n < (c->lpm.lpb ? c->lpm.n_rep : d.R)) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    if (c->lpm.lpb) {
        const uint32_t nr = c->lpm.n_rep;
        uint64_t* dd = nullptr;
        HIPCHK(hipMallocAsync((void**)&dd, 64ull * nr, c->stream));
        HIPCHK(hipMemsetAsync(dd, 0, 64ull * nr, c->stream));
        hipLaunchKernelGGL(tw_lpb_reduce, dim3((nr + 63) / 64, TW_RED_GROUPS / 4), dim3(256), 0, c->stream, d, dd);
        HIPCHK(hipGetLastError());
        std::vector<uint64_t> h(8ull * nr);
        HIPCHK(hipMemcpyAsync(h.data(), dd, 64ull * nr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipFreeAsync(dd, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t q = 0; q < nr; ++q) {
            tw_replica_result& o = out[q];
            std::memset(&o, 0, sizeof(o));
            o.final_t = (int64_t)h[q]; o.events = h[nr + q]; o.delivered = h[2ull * nr + q];
            o.dropped = h[3ull * nr + q]; o.undeliverable = h[4ull * nr + q]; o.status = (uint32_t)h[5ull * nr + q];
            o.main_exc = (uint32_t)h[6ull * nr + q];  // (the node tag is in the high word)
            o.threads = h[7ull * nr + q];
        }
        return TW_OK;
    }
    const size_t nsc = (size_t)(d.sc_lp ? SC_LP_STRIDE : SC_COUNT) * d.R;
    std::vector<uint64_t> sc(nsc);
    HIPCHK(hipMemcpyAsync(sc.data(), d.scal, 8ull * nsc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    auto F = [&](int f, uint32_t i) { return d.sc_lp ? sc[(size_t)i * SC_LP_STRIDE + f] : sc[(size_t)f * d.R + i]; };
    for (uint32_t i = 0; i < d.R; ++i) {
        out[i].final_t = (int64_t)F(SC_FINAL_T, i); out[i].events = F(SC_EVENTS, i);
        out[i].delivered = F(SC_DELIVERED, i); out[i].dropped = F(SC_DROPPED, i);
        out[i].undeliverable = F(SC_UNDELIV, i); out[i].status = (uint32_t)F(SC_STATUS, i);
        out[i].main_exc = (uint32_t)F(SC_MAIN_EXC, i); out[i].threads = F(SC_THREADS, i);
        out[i].tie_flags = i < c->tie_flags.size() ? c->tie_flags[i] : 0u;
        out[i].reserved = 0;
    }
    return TW_OK;
}

static int digest(tw_shard* c, std::vector<uint64_t>& h) {
    const Dev& d = c->d;
    uint64_t* dd = nullptr;
    HIPCHK(hipMallocAsync((void**)&dd, 8ull * d.R, c->stream));
    hipLaunchKernelGGL(tw_digest_kernel, dim3((d.R + 255) / 256), dim3(256), 0, c->stream, d, dd);
    HIPCHK(hipGetLastError());
    h.resize(d.R);
    HIPCHK(hipMemcpyAsync(h.data(), dd, 8ull * d.R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipFreeAsync(dd, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TW_OK;
}

int sh_tie_audit(tw_shard* c, int64_t t_end_us, uint64_t max_events, uint32_t probes, tw_stats* out) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (c->lpm.lp || probes < 1 || probes > 2) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    std::vector<std::vector<uint64_t>> dg(probes + 1);
    int rc = TW_OK;
    c->px.touch();
    for (uint32_t p = probes; p + 1 > 0 && rc == TW_OK; --p) {  // probes first, the canonical run last
        c->d.tie_mode = p;
        rc = sh_reset(c);
        if (rc == TW_OK) rc = sh_run(c, t_end_us, max_events, p == 0 ? out : nullptr);
        if (rc == TW_OK) rc = digest(c, dg[p]);
        if (p == 0) break;
    }
    c->d.tie_mode = TW_TIE_FIFO;
    c->px.touch();  // (the probes ran under other tie modes)
    if (rc != TW_OK) return rc;
    c->tie_flags.assign(c->d.R, 1u);
    for (uint32_t p = 1; p <= probes; ++p)
        for (uint32_t i = 0; i < c->d.R; ++i)
            if (dg[p][i] != dg[0][i]) c->tie_flags[i] |= 1u << p;
    return TW_OK;
}

int sh_geometry(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    return c->lpm.lpb ? TW_GEO_LPB : c->lpm.lp ? TW_GEO_LP : c->geo;
}

// The equal-timestamp order of later runs (include/timewarp.h tw_set_tie_mode).
// TW_TIE_PQUEUE runs the wave kernel with each replica's queue as pqueue's
// binomial MinQueue (wave.hip); its node links, free stack, rebuild scratch
// and header are allocated here on first use.
int sh_set_tie_mode(tw_shard* c, uint32_t mode) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (mode > TW_TIE_FORKFIRST) return TW_ERR_INVALID;
    // a forked child first: the lane-per-replica kernels (their fork_in_place);
    // the wave and logical-process kernels keep the other orders
    if (mode == TW_TIE_FORKFIRST && (c->lpm.lp || c->geo == TW_GEO_WAVE)) return TW_ERR_INVALID;
    if (mode == TW_TIE_PQUEUE) {
        if (c->lpm.lp || c->geo != TW_GEO_WAVE) return TW_ERR_INVALID;  // the wave kernel only
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        Dev& d = c->d;
        const size_t n = (size_t)d.Q * d.R;
        int e;
        if (!d.pq_link) {
            if ((e = dalloc(c, &d.pq_link, n)) != TW_OK) return e;
            if ((e = dalloc(c, &d.pq_free, n)) != TW_OK) return e;
            if ((e = dalloc(c, &d.pq_scr, n)) != TW_OK) return e;
            if ((e = dalloc(c, &d.pq_hdr, (size_t)d.R * PQ_WORDS)) != TW_OK) return e;
        }
    }
    c->d.tie_mode = mode;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->px.drop();
    return TW_OK;
}

int sh_set_counter_base(tw_shard* c, uint32_t seq0, uint32_t tid0) {
    if (!c || tid0 == 0) return TW_ERR_INVALID;
    c->seq0 = seq0;
    c->tid0 = tid0;
    c->px.touch();
    if (c->px.snap.have) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->px.drop();
    }
    return TW_OK;
}

// The send-free prefix of later tw_run calls (include/timewarp.h tw_set_prefix);
// on after every tw_load.
int sh_set_prefix(tw_shard* c, int on) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    c->px.on = on != 0;
    c->px.touch();
    return TW_OK;
}

int sh_prefix_stats(tw_shard* c, int64_t* t0, uint64_t* events, uint64_t* bytes, uint32_t* last, double* ms) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (t0) *t0 = c->px.t0;
    if (events) *events = c->px.snap.ok ? c->px.snap.events : 0;
    if (bytes) *bytes = c->px.snap.ok ? c->px.snap.bytes : 0;
    if (last) *last = c->px.last;
    if (ms) *ms = c->px.ms;
    return TW_OK;
}

int sh_prefix_clean_stats(tw_shard* c, uint32_t* claimed, uint64_t* rows_skipped, uint64_t* bytes_stored,
                          uint32_t* verified, uint64_t* audit) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    const Prefix::Snap::Clean& cl = c->px.snap.clean;
    if (claimed) *claimed = c->px.snap.ok ? (uint32_t)cl.slots.size() : 0u;
    if (rows_skipped) *rows_skipped = c->px.rows_skipped;
    if (bytes_stored) *bytes_stored = c->px.bytes_stored;
    if (verified) *verified = c->px.last_verified ? 1u : 0u;
    if (audit) {
        unsigned long long n = 0;
        if (c->px.audited && c->px.snap.audit) {
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipMemcpyAsync(&n, c->px.snap.audit, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        *audit = n;
    }
    return TW_OK;
}

int sh_prefix_rows_stats(tw_shard* c, tw_prefix_rows* out) {
    if (!c || !out) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    std::memset(out, 0, sizeof(*out));
    const Prefix& px = c->px;
    out->rows_hdr = px.rows.n[0]; out->rows_run = px.rows.n[1]; out->rows_reset = px.rows.n[2];
    out->bytes_hdr = px.rows.bytes[0]; out->bytes_run = px.rows.bytes[1]; out->bytes_reset = px.rows.bytes[2];
    out->bytes_stored = px.rows.stored;
    out->apply_form = px.rows.form;
    out->host_pairs = px.rows.pairs;
    // the device's own counts: the list it wrote, and (hook on) the rows it skipped by class
    if (px.snap.ok && px.snap.audit && px.rows.form) {
        unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpyAsync(h, px.snap.audit, 64, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (px.rows.form == 2u) out->list_pairs = (uint32_t)h[6];
        if (px.audited)
            for (int k = 1; k < 5; ++k) out->audit_rows[k] = h[k];
    }
    if (px.snap.ok && px.snap.cls)
        for (int k = 0; k < 5; ++k) { out->class_rows[k] = px.snap.class_rows[k]; out->class_bytes[k] = px.snap.class_bytes[k]; }
    return TW_OK;
}

// The killThread sweep of later tw_run calls (include/timewarp.h tw_set_sweep);
// on after every tw_load.
int sh_set_sweep(tw_shard* c, int on) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    c->sw.on = on != 0;
    c->px.touch();
    return TW_OK;
}

int sh_sweep_stats(tw_shard* c, uint64_t* killers, uint64_t* victims, uint64_t* refused, double* ms) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (killers) *killers = c->sw.last[0];
    if (victims) *victims = c->sw.last[1];
    if (refused) *refused = c->sw.last[2];
    if (ms) *ms = c->sw.ms;
    return TW_OK;
}

int sh_sweep_path_stats(tw_shard* c, uint64_t* terminal, uint64_t* fast, uint64_t* slow) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (terminal) *terminal = c->sw.path[0];
    if (fast) *fast = c->sw.path[1];
    if (slow) *slow = c->sw.last[0] - c->sw.path[1];
    return TW_OK;
}

int sh_read_hashes(tw_shard* c, uint64_t* out, size_t n) {
    if (!c || !out) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    const Dev& d = c->d;
    if (n < (size_t)d.R * d.N) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    if (c->lpm.lpb) {  // hash_g is [node][replica] over the batch too
        std::vector<uint64_t> tmp((size_t)d.Ntot << d.rep_lg);
        HIPCHK(hipMemcpyAsync(tmp.data(), d.hash_g, 8 * tmp.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t node = 0; node < d.Ntot; ++node)
            for (uint32_t q = 0; q < c->lpm.n_rep; ++q) out[(size_t)q * d.Ntot + node] = tmp[((size_t)node << d.rep_lg) | q];
        return TW_OK;
    }
    std::vector<uint64_t> tmp((size_t)d.R * d.N);  // device layout [node][replica]
    HIPCHK(hipMemcpyAsync(tmp.data(), d.hash, 8ull * d.R * d.N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint32_t node = 0; node < d.N; ++node)
        for (uint32_t r = 0; r < d.R; ++r) out[(size_t)r * d.N + node] = tmp[(size_t)node * d.R + r];
    return TW_OK;
}

static int lp_scatter(tw_shard* c, const uint4* recs, uint32_t n, bool to_foreign) {
    const Dev& d = c->d;
    if (n == 0) return TW_OK;
    uint32_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(tw_lp_scatter, dim3(blocks), dim3(256), 0, c->stream, d, recs, n,
                       to_foreign ? c->lpm.foreign : nullptr, c->lpm.n_foreign, d.out_cap);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

int sh_lp_window(tw_shard* c, int64_t t_end_excl, int64_t* next_t, uint64_t* n_foreign) {
    if (!c || !next_t) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp) return TW_ERR_STATE;
    tw_stats st{};
    int rc = sh_run(c, t_end_excl - 1, UINT64_MAX, nullptr);
    if (rc) return rc;
    (void)st;
    const Dev& d = c->d;
    hipStream_t s = c->stream;
    uint32_t nout = 0;
    HIPCHK(hipMemcpyAsync(&nout, d.out_n, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nout > d.out_cap) nout = d.out_cap;
    rc = lp_scatter(c, d.outbox, nout, true);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d.out_n, 0, 4, s));
    uint64_t nt = 0;
    uint32_t nf = 0, err = 0;
    HIPCHK(hipMemcpyAsync(&nt, d.next_t, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nf, c->lpm.n_foreign, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d.lp_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err) return TW_ERR_REPLICA;
    *next_t = nt > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)nt;
    if (n_foreign) *n_foreign = nf;
    return TW_OK;
}

int sh_lp_take_outbox(tw_shard* c, tw_lp_record* out, size_t cap, size_t* n) {
    if (!c || !n) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp) return TW_ERR_STATE;
    hipStream_t s = c->stream;
    uint32_t nf = 0;
    HIPCHK(hipMemcpyAsync(&nf, c->lpm.n_foreign, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (nf > cap || !out) { *n = nf; return nf > cap ? TW_ERR_INVALID : TW_OK; }
    if (nf) HIPCHK(hipMemcpyAsync(out, c->lpm.foreign, 32ull * nf, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemsetAsync(c->lpm.n_foreign, 0, 4, s));
    HIPCHK(hipStreamSynchronize(s));
    *n = nf;
    return TW_OK;
}

int sh_lp_inject(tw_shard* c, const tw_lp_record* recs, size_t n, int64_t* next_t) {
    if (!c || (n && !recs)) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp) return TW_ERR_STATE;
    const Dev& d = c->d;
    if (n > d.out_cap) return TW_ERR_INVALID;
    hipStream_t s = c->stream;
    if (n) {
        HIPCHK(hipMemcpyAsync(c->lpm.staging, recs, 32ull * n, hipMemcpyHostToDevice, s));
        int rc = lp_scatter(c, c->lpm.staging, (uint32_t)n, false);
        if (rc) return rc;
    }
    uint64_t nt = 0;
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&nt, d.next_t, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d.lp_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err) return TW_ERR_REPLICA;
    if (next_t) *next_t = nt > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)nt;
    return TW_OK;
}

int sh_lp_results(tw_shard* c, tw_replica_result* agg, uint64_t* node_hashes, size_t n_nodes) {
    if (!c || !agg) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp) return TW_ERR_STATE;
    const Dev& d = c->d;
    std::vector<tw_replica_result> rr(d.R);
    int rc = sh_read_results(c, rr.data(), rr.size());
    if (rc) return rc;
    std::memset(agg, 0, sizeof(*agg));
    agg->status = TW_REP_DONE;
    for (auto& x : rr) {
        agg->final_t = x.final_t > agg->final_t ? x.final_t : agg->final_t;
        agg->events += x.events; agg->delivered += x.delivered; agg->dropped += x.dropped;
        agg->undeliverable += x.undeliverable; agg->threads += x.threads;
        if (x.main_exc) agg->main_exc = x.main_exc;
        if (x.status >= TW_REP_ABORTED) agg->status = x.status;
    }
    if (node_hashes) {
        if (n_nodes < d.Ntot) return TW_ERR_INVALID;
        HIPCHK(hipMemcpyAsync(node_hashes, d.hash_g, 8ull * d.Ntot, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return TW_OK;
}

int sh_set_stream(tw_shard* c, void* hs) {
    if (!c) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // finish what was queued on the old one
    c->px.touch();
    c->stream = hs ? (hipStream_t)hs : c->own_stream;
    return TW_OK;
}

// The exchange of the device loop over `world` ranks; this shard is `rank`,
// owning nodes [starts[rank], starts[rank + 1]).  send/recv: world blocks of
// (cap + 1) records (header + records); red: RD_COUNT int64.  Also sizes the
// carry buffer (records beyond a tick's block size wait there).
static int exchange_common(tw_shard* c, uint32_t world, uint32_t rank, const uint32_t* starts, uint32_t cap) {
    if (!c || world == 0 || rank >= world || !starts) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp) return TW_ERR_STATE;
    if (world > 1 && cap == 0) return TW_ERR_INVALID;
    for (uint32_t g = 0; g < world; ++g)
        if (starts[g] > starts[g + 1]) return TW_ERR_INVALID;
    if (starts[rank] != c->d.lp0 || starts[rank + 1] != c->d.lp0 + c->d.R) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->ex.drop(c->d);
    HIPCHK(hipMalloc((void**)&c->ex.starts, 4ull * (world + 1)));
    HIPCHK(hipMemcpy(c->ex.starts, starts, 4ull * (world + 1), hipMemcpyHostToDevice));
    if (world > 1) {
        // a tick's foreign records beyond the block size: at most a tick's outbox
        const uint32_t cc = c->d.out_cap < (1u << 20) ? c->d.out_cap : (1u << 20);
        const size_t bytes = 2ull * cc * 32 + 256;
        HIPCHK(hipMalloc(&c->ex.carry, bytes));
        HIPCHK(hipMemsetAsync(c->ex.carry, 0, bytes, c->stream));
        c->ex.set_carry(c->d, cc);
    }
    c->ex.world = world;
    c->ex.rank = rank;
    c->ex.cap = cap;
    c->ex.cap_eff = c->ex.cap;
    return TW_OK;
}

int sh_lp_exchange_setup(tw_shard* c, uint32_t world, uint32_t rank, const uint32_t* starts, void* send, void* recv,
                         uint32_t cap, int64_t* red) {
    if (c && world > 1 && (!send || !recv || !red)) return TW_ERR_INVALID;
    int rc = exchange_common(c, world, rank, starts, cap);
    if (rc) return rc;
    c->ex.send = world > 1 ? (uint4*)send : nullptr;
    c->ex.recv = world > 1 ? (uint4*)recv : nullptr;
    c->ex.red = world > 1 ? red : c->ex.red_own;
    if (world > 1) HIPCHK(hipMemsetAsync(send, 0, 32ull * world * (cap + 1), c->stream));
    return TW_OK;
}

// The same with library-owned buffers (the library-driven loop of abi.hip:
// RCCL send/recv or device copies between shards move the blocks).
int sh_lp_exchange_own(tw_shard* c, uint32_t world, uint32_t rank, const uint32_t* starts, uint32_t cap) {
    int rc = exchange_common(c, world, rank, starts, world > 1 ? cap : 1u);
    if (rc) return rc;
    const size_t blk = 32ull * world * ((size_t)c->ex.cap + 1);
    HIPCHK(hipMalloc(&c->ex.own, 2 * blk + 8ull * RD_COUNT));
    HIPCHK(hipMemsetAsync(c->ex.own, 0, 2 * blk + 8ull * RD_COUNT, c->stream));
    // (one rank too: its import, fill and the all-reduce of the words then go
    // through the transport -- a one-rank RCCL communicator -- like any rank's)
    c->ex.send = (uint4*)c->ex.own;
    c->ex.recv = (uint4*)((char*)c->ex.own + blk);
    c->ex.red = (int64_t*)((char*)c->ex.own + 2 * blk);
    return TW_OK;
}

void sh_lp_exchange_info(tw_shard* c, ShardXchg* x) {
    x->device = c->device;
    x->stream = c->stream;
    x->send = c->ex.send;
    x->recv = c->ex.recv;
    x->red = c->ex.red;
    x->world = c->ex.world;
    x->stride = c->ex.cap;
    x->cap_eff = c->ex.cap_eff;
}
int sh_lp_set_block(tw_shard* c, uint32_t cap_eff) {
    if (!c || cap_eff == 0 || cap_eff > c->ex.cap) return TW_ERR_INVALID;
    c->ex.cap_eff = cap_eff;
    return TW_OK;
}
// WN_XMAX after a tw_lp_progress (the largest per-rank demand of one tick since
// the last clear); clear it on the device (stream-ordered)
int64_t sh_lp_xmax(tw_shard* c) { return c->ex.h_win ? c->ex.h_win[WN_XMAX] : 0; }
int sh_lp_clear_xmax(tw_shard* c) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(c->ex.win_buf + WN_XMAX, 0, 8, c->stream));
    return TW_OK;
}


// A fresh window's start (every tick launches it; the kernels return unless
// the window is fresh): the heavy lanes' due runs (tw_lp_due), the work list
// from the last window's marks (tw_lpb_compact / tw_lp_compact), then the
// due runs' batchable prefixes (tw_lp_batch: its replies' marks are the next
// window's, so after the list).  (Tried both in one pass over each heavy
// lane's records: C5 1,463 -> 1,708 ms per step -- one 89-KB workgroup per CU
// ran the batch's dry runs that the separate tw_lp_batch runs three workgroups
// per CU wide)
static int lp_window_start(tw_shard* c) {
    // (tracing on: tw_lp_batch runs handlers without Lane and would record
    // nothing -- every due record stays on the lane's chain, unless
    // tw_set_trace_batch asked for tw_lp_batch<true>, which records)
    const bool tr = c->d.trace_cap != 0;
    const bool bat = c->lpm.heavy_ok && c->d.lpc_bat && (!tr || c->lpm.trace_bat_run);
    if (c->lpm.heavy_ok) {
        hipLaunchKernelGGL(tw_lp_due, dim3(TW_DUE_GRID), dim3(256), 0, c->stream, c->dwin());
        HIPCHK(hipGetLastError());
    }
    if (c->d.rw) {  // per-replica windows: tiles of 64 replicas x one chunk of nodes, four per workgroup
        const uint32_t nk = ((c->d.R >> c->d.rep_lg) + (1u << TW_CHUNK_LG) - 1u) >> TW_CHUNK_LG;
        const uint32_t tiles = nk * (((1u << c->d.rep_lg) + 63u) >> 6);
        hipLaunchKernelGGL(tw_lpb_compact, dim3((tiles + 3) / 4), dim3(256), 0, c->stream, c->dwin());
    } else {
        hipLaunchKernelGGL(tw_lp_compact, dim3(compact_blocks(c->d.R)), dim3(256), 0, c->stream, c->dwin(), 0u, 0u);
    }
    HIPCHK(hipGetLastError());
    if (bat) {
        hipLaunchKernelGGL(tr ? tw_lp_batch<true> : tw_lp_batch<false>, dim3(TW_DUE_GRID), dim3(TW_BAT_T), 0,
                           c->stream, c->dwin());
        HIPCHK(hipGetLastError());
    }
    return TW_OK;
}

int sh_lp_loop_begin(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp) return TW_ERR_STATE;
    if (const char* b = getenv("TW_LP_TICK_BUDGET")) {
        const long v = strtol(b, nullptr, 10);
        c->lp_budget = v >= 1 && v <= (1 << 20) ? (uint32_t)v : (1u << 14);
    }
    if (const char* b = getenv("TW_LP_GRID")) {  // (tests: the grid-stride walk on small contexts)
        const long v = strtol(b, nullptr, 10);
        c->lp_grid = v >= 1 && v <= (1 << 20) ? (uint32_t)v : TW_LP_GRID;
    }
    HIPCHK(hipSetDevice(c->device));
    if (!c->ex.red) c->ex.red = c->ex.red_own;  // world 1 without an explicit setup
    c->d.act_cur = 0;
    c->d.wid = 0;
    hipLaunchKernelGGL(tw_lp_begin, dim3(1), dim3(1), 0, c->stream, c->dwin(), c->d.lookahead);
    HIPCHK(hipGetLastError());
    // the record blocks' counts (tw_lp_ctl clears them every tick; a loop that
    // stopped inside a tick -- a failure on some rank -- may have left some)
    for (uint32_t g = 0; c->ex.send && g < c->ex.world; ++g)
        HIPCHK(hipMemsetAsync(c->ex.send + (size_t)g * (c->ex.cap + 1) * 2, 0, sizeof(uint4), c->stream));
    if (c->d.rw) {  // every replica's first window starts at 0; minima empty
        const size_t nrep = (size_t)1 << c->d.rep_lg;
        HIPCHK(hipMemsetAsync(c->d.rw + RW_T * nrep, 0, 8 * nrep, c->stream));
        HIPCHK(hipMemsetAsync(c->d.rw + RW_TICK * nrep, 0xFF, 8 * nrep * (RW_COUNT - RW_TICK), c->stream));
    }
    HIPCHK(hipMemsetAsync(c->d.lp_err, 0, 4, c->stream));
    int rc = lp_window_start(c);
    if (rc) return rc;
    c->ex.loop_ready = true;
    return TW_OK;
}

static uint32_t lp_grid(uint32_t n) {
    const uint32_t b = (n + 255) / 256;
    return b < 1 ? 1 : b > 2048 ? 2048 : b;
}

int sh_lp_tick(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp || !c->ex.loop_ready) return TW_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const Dev d = c->dwin();
    // the window comes from the device (tw_run_kernel reads c.win); launch
    // arguments are captured at enqueue, so d.win is set only around it
    c->d.win = c->ex.win_buf;
    launch_run<GeoLP>(c, st, 0, UINT64_MAX, c->lp_budget);
    c->d.win = nullptr;
    HIPCHK(hipGetLastError());
    if (c->ex.world > 1 && d.carry) {  // the previous tick's carry claims block slots first
        hipLaunchKernelGGL(tw_lp_pack_carry, dim3(lp_grid(d.carry_cap)), dim3(256), 0, st, d, c->ex.send,
                           (const uint32_t*)c->ex.starts, c->ex.world, c->ex.cap, c->ex.cap_eff);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(tw_lp_pack, dim3(lp_grid(d.out_cap)), dim3(256), 0, st, d, c->ex.send,
                       (const uint32_t*)c->ex.starts, c->ex.world, c->ex.cap, c->ex.cap_eff);
    HIPCHK(hipGetLastError());
    return TW_OK;
}

int sh_lp_tick_import(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp || !c->ex.loop_ready) return TW_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // (no exchange buffers -- one rank of a caller-driven loop: tw_lp_ctl
    // fills the words itself)
    if (c->ex.send) {
        hipLaunchKernelGGL(tw_lp_import, dim3(lp_grid(c->ex.world * c->ex.cap_eff)), dim3(256), 0, st, c->dwin(),
                           (const uint4*)c->ex.recv, c->ex.world, c->ex.cap, c->ex.cap_eff);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(tw_lp_fill, dim3(1), dim3(1), 0, st, c->dwin(), c->ex.red, (const uint4*)c->ex.send,
                           c->ex.world, c->ex.cap);
        HIPCHK(hipGetLastError());
    }
    return TW_OK;
}

int sh_lp_tick_end(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp || !c->ex.loop_ready) return TW_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(tw_lp_ctl, dim3(1), dim3(1), 0, c->stream, c->dwin(), c->ex.red, c->ex.send, c->ex.world,
                       c->ex.cap, c->ex.send ? 1u : 0u);
    HIPCHK(hipGetLastError());
    if (c->d.rw) {
        const uint32_t nrep = 1u << c->d.rep_lg;
        hipLaunchKernelGGL(tw_lpb_rctl, dim3((nrep + 255) / 256), dim3(256), 0, c->stream, c->dwin());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(tw_lpb_fin, dim3(1), dim3(1), 0, c->stream, c->dwin());
        HIPCHK(hipGetLastError());
    }
    return lp_window_start(c);
}

// the window words + lp_err into the pinned host copy (stream-ordered)
static int lp_progress_copy(tw_shard* c) {
    int64_t* w = c->ex.h_win;  // pinned: plain DMA copies, no staging blit
    HIPCHK(hipMemcpyAsync(w, c->ex.win_buf, 8 * WN_COUNT, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(w + WN_COUNT, c->d.lp_err, 4, hipMemcpyDeviceToHost, c->stream));
    return TW_OK;
}
static int lp_progress_read(tw_shard* c, tw_lp_state* out) {
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t* w = c->ex.h_win;
    const uint32_t err = (uint32_t)w[WN_COUNT];
    out->windows = (uint64_t)w[WN_WINDOWS];
    out->ticks = (uint64_t)w[WN_TICKS];
    out->t = w[WN_T];
    out->done = (w[WN_FLAGS] & WN_DONE) ? 1u : 0u;
    out->err = err;
    return TW_OK;
}
static int lp_host_alloc(tw_shard* c) {
    if (!c->ex.h_win) HIPCHK(hipHostMalloc((void**)&c->ex.h_win, 8 * (WN_COUNT + 1)));
    return TW_OK;
}

int sh_lp_progress(tw_shard* c, tw_lp_state* out) {
    if (!c || !out) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp || !c->ex.loop_ready) return TW_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    int rc = lp_host_alloc(c);
    if (rc) return rc;
    c->ex.h_win[WN_COUNT] = 0;  // lp_err fills its low 4 bytes
    rc = lp_progress_copy(c);
    return rc ? rc : lp_progress_read(c, out);
}

#define TW_GRAPH_TICKS 16
// the launch arguments a captured tick graph depends on
static std::vector<unsigned char> tick_key(const tw_shard* c) {
    struct K {
        Dev d;
        hipStream_t st;
        int64_t *win, *h_win, *red;
        uint4 *send, *recv;
        uint32_t *starts, budget, grid, world, cap, cap_eff;
        size_t lds;
        bool heavy, trace_bat;
    } k;
    std::memset(&k, 0, sizeof(k));
    std::memcpy(&k.d, &c->d, sizeof(Dev));
    k.st = c->stream;
    k.win = c->ex.win_buf;
    k.h_win = c->ex.h_win;
    k.red = c->ex.red;
    k.send = c->ex.send;
    k.recv = c->ex.recv;
    k.starts = c->ex.starts;
    k.budget = c->lp_budget;
    k.grid = c->lp_grid;
    k.world = c->ex.world;
    k.cap = c->ex.cap;
    k.cap_eff = c->ex.cap_eff;
    k.lds = c->lds_bytes;
    k.heavy = c->lpm.heavy_ok;
    k.trace_bat = c->lpm.trace_bat_run;
    std::vector<unsigned char> v(sizeof(K));
    std::memcpy(v.data(), &k, sizeof(K));
    return v;
}
// TW_GRAPH_TICKS ticks and the progress copy, captured once per set of launch
// arguments (every kernel of a tick reads its window from the device, so the
// same graph serves every batch; ticks after the loop is done return at once)
static int tick_graph_ready(tw_shard* c) {
    std::vector<unsigned char> key = tick_key(c);
    if (c->tg.exec && key == c->tg.key) return TW_OK;
    c->tg.unload();
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = TW_OK;
    for (int i = 0; i < TW_GRAPH_TICKS && !rc; ++i) {
        rc = sh_lp_tick(c);
        if (!rc) rc = sh_lp_tick_import(c);
        if (!rc) rc = sh_lp_tick_end(c);
    }
    if (!rc) rc = lp_progress_copy(c);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (rc || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc ? rc : TW_ERR_HIP;
    }
    const hipError_t ei = hipGraphInstantiate(&c->tg.exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
        c->tg.exec = nullptr;
        return TW_ERR_HIP;
    }
    c->tg.key = std::move(key);
    return TW_OK;
}

int sh_lp_run_windows(tw_shard* c, uint64_t max_ticks, tw_lp_state* out) {
    if (!c || !out) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lp || !c->ex.loop_ready) return TW_ERR_STATE;
    if (c->ex.world != 1) return TW_ERR_STATE;
    HIPCHK(hipSetDevice(c->device));
    int rc = lp_host_alloc(c);
    if (rc) return rc;
    const char* ng = getenv("TW_NO_GRAPH");  // (A/B: launch every kernel from the host)
    const bool graph = !(ng && *ng && *ng != '0');
    for (uint64_t done_ticks = 0; done_ticks < max_ticks;) {
        const uint64_t batch =
            max_ticks - done_ticks < TW_GRAPH_TICKS ? max_ticks - done_ticks : (uint64_t)TW_GRAPH_TICKS;
        c->ex.h_win[WN_COUNT] = 0;  // lp_err fills its low 4 bytes
        if (graph && batch == TW_GRAPH_TICKS) {
            rc = tick_graph_ready(c);
            if (rc) return rc;
            HIPCHK(hipGraphLaunch(c->tg.exec, c->stream));
        } else {
            for (uint64_t i = 0; i < batch; ++i) {
                rc = sh_lp_tick(c);
                if (!rc) rc = sh_lp_tick_import(c);
                if (!rc) rc = sh_lp_tick_end(c);
                if (rc) return rc;
            }
            rc = lp_progress_copy(c);
            if (rc) return rc;
        }
        done_ticks += batch;
        rc = lp_progress_read(c, out);
        if (rc) return rc;
        if (out->err) return TW_ERR_REPLICA;
        if (out->done) return TW_OK;
    }
    return TW_ERR_INCOMPLETE;
}

// Batched LP: tw_run = the whole device window loop (one host sync per 16 ticks)
static int lpb_run(tw_shard* c, tw_stats* out) {
    auto w0 = std::chrono::steady_clock::now();
    // the run's counts are the results minus those before it: zero right
    // after tw_reset (no reduction pass needed)
    std::vector<tw_replica_result> before;
    if (out) {
        before.resize(c->lpm.n_rep);
        if (c->lpm.fresh) {
            std::memset(before.data(), 0, sizeof(tw_replica_result) * before.size());
        } else {
            int rc = sh_read_results(c, before.data(), before.size());
            if (rc) return rc;
        }
    }
    c->lpm.fresh = false;
    int rc = sh_lp_loop_begin(c);
    if (rc) return rc;
    c->times.start();
    tw_lp_state ls{};
    int rcw = TW_OK;  // (the loop's own result: its time is taken either way)
    rc = c->times.timed(c->stream, [&]() -> int { rcw = sh_lp_run_windows(c, 1ull << 40, &ls); return TW_OK; });
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    rc = c->times.read();
    if (rc) return rc;
    c->lpm.windows = ls.windows;
    c->lpm.ticks = ls.ticks;
    if (rcw) return rcw;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        std::vector<tw_replica_result> rr(c->lpm.n_rep);
        rc = sh_read_results(c, rr.data(), rr.size());
        if (rc) return rc;
        for (uint32_t i = 0; i < c->lpm.n_rep; ++i) {
            out->events += rr[i].events - before[i].events;
            out->delivered += rr[i].delivered - before[i].delivered;
            out->dropped += rr[i].dropped - before[i].dropped;
            out->undeliverable += rr[i].undeliverable - before[i].undeliverable;
            if (rr[i].final_t > out->max_final_t) out->max_final_t = rr[i].final_t;
            if (rr[i].status == TW_REP_DONE) ++out->replicas_done;
            if (rr[i].status >= TW_REP_ERR_SLOTS) ++out->replicas_error;
        }
        out->sends = out->delivered + out->dropped + out->undeliverable;
        out->launches = 1;  // the window loop, timed as one (tw_last_launch_ms)
        out->kernel_ms = c->times.total;
        out->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    }
    return TW_OK;
}

int sh_lpb_windows(tw_shard* c, uint64_t* windows, uint64_t* ticks) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lpb) return TW_ERR_STATE;
    if (windows) *windows = c->lpm.windows;
    if (ticks) *ticks = c->lpm.ticks;
    return TW_OK;
}

int sh_lpb_batch(tw_shard* c, uint64_t* batched, uint64_t* due) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded || !c->lpm.lpb) return TW_ERR_STATE;
    unsigned long long h[2] = {0, 0};
    if (c->d.bat_ctr) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipMemcpyAsync(h, c->d.bat_ctr, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (batched) *batched = h[0];
    if (due) *due = h[1];
    return TW_OK;
}

// Diagnostic build only (-DTW_STATS): copy the P_COUNT counters out,
// optionally zeroing them; the product build has none (TW_ERR_STATE).
int sh_prof_read(tw_shard* c, unsigned long long* out, size_t cap, int reset) {
#ifdef TW_STATS
    if (!c || !out || !c->loaded || !c->d.prof) return TW_ERR_STATE;
    const size_t all = (size_t)2 * P_COUNT + TW_BPROF;  // all lanes, heavy LP lanes, tw_lp_batch's phases
    size_t n = cap < all ? cap : all;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(out, c->d.prof, 8 * n, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(c->d.prof, 0, 8 * all));
    return (int)n;
#else
    (void)c; (void)out; (void)cap; (void)reset;
    return TW_ERR_STATE;
#endif
}

uint32_t sh_replicas(tw_shard* c) { return c->lpm.lpb ? c->lpm.n_rep : c->d.R; }
uint32_t sh_nodes(tw_shard* c) { return c->lpm.lpb ? c->d.Ntot : c->d.N; }
bool sh_is_lp(tw_shard* c) { return c->lpm.lp; }
bool sh_loaded(tw_shard* c) { return c->loaded; }
uint32_t sh_links(tw_shard* c) { return c->d.L; }
int sh_device(tw_shard* c) { return c->device; }

int sh_set_trace(tw_shard* c, uint32_t cap) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    // node-partitioned (tw_lp_load): LP lanes are nodes -- no replica execution
    // order to record, and one counter for all lanes.  Batched LP records per
    // replica, in claim order (Lane::trace_rec)
    if (c->lpm.lp && !c->lpm.lpb) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->px.touch();
    trace_release(c->d);
    if (cap) {
        // (batched LP: d.R counts lanes)
        const size_t nrep = c->lpm.lpb ? c->lpm.n_rep : c->d.R;
        HIPCHK(hipMalloc(&c->d.trace, (size_t)cap * nrep * 32));
        if (c->lpm.lpb) {
            if (hipMalloc(&c->d.trace_n, 8 * nrep) != hipSuccess) {
                (void)hipGetLastError();
                trace_release(c->d);
                return TW_ERR_OOM;
            }
            HIPCHK(hipMemsetAsync(c->d.trace_n, 0, 8 * nrep, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        c->d.trace_cap = cap;
    }
    return TW_OK;
}

int sh_set_trace_batch(tw_shard* c, int on) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (!c->lpm.lpb) return TW_ERR_INVALID;  // (tw_lp_batch serves batched LP contexts only)
    c->lpm.trace_bat = on != 0;
    return TW_OK;
}

int sh_read_trace(tw_shard* c, uint32_t replica, tw_trace_rec* out, size_t cap, uint64_t* n_emitted) {
    if (!c || (cap && !out)) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    const Dev& d = c->d;
    if (c->lpm.lp && !c->lpm.lpb) return TW_ERR_INVALID;
    const size_t nrep = c->lpm.lpb ? c->lpm.n_rep : d.R;  // the records' replica stride (batched LP: d.R counts lanes)
    if (replica >= nrep) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    uint64_t n = 0;
    if (!c->lpm.lpb)
        HIPCHK(hipMemcpyAsync(&n, d.scal + (size_t)SC_TRACE_N * d.R + replica, 8, hipMemcpyDeviceToHost, c->stream));
    else if (d.trace_n)
        HIPCHK(hipMemcpyAsync(&n, d.trace_n + replica, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_emitted) *n_emitted = n;
    size_t k = n < d.trace_cap ? (size_t)n : (size_t)d.trace_cap;
    if (k > cap) k = cap;
    if (k) {
        // records of one replica are strided by R: one 2D copy
        std::vector<uint4> buf(2 * k);
        HIPCHK(hipMemcpy2DAsync(buf.data(), 32, d.trace + (size_t)replica * 2, nrep * 32, 32, k,
                                hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->lpm.lpb) {
            // claim order says nothing: the canonical order (t, node, tag, val)
            struct Q2 { uint4 a, b; };
            Q2* q = reinterpret_cast<Q2*>(buf.data());
            auto key = [](const Q2& x) {
                return std::make_tuple((int64_t)(((uint64_t)x.a.y << 32) | x.a.x), x.a.z, x.a.w,
                                       (int64_t)(((uint64_t)x.b.y << 32) | x.b.x));
            };
            std::sort(q, q + k, [&](const Q2& x, const Q2& y) { return key(x) < key(y); });
        }
        for (size_t i = 0; i < k; ++i) {
            const uint4 a = buf[2 * i], b = buf[2 * i + 1];
            out[i].t = (int64_t)(((uint64_t)a.y << 32) | a.x);
            out[i].val = (int64_t)(((uint64_t)b.y << 32) | b.x);
            out[i].node = a.z;
            out[i].tag = a.w;
        }
    }
    return TW_OK;
}

// ---- node-partitioned contexts (tw_lp_set_trace ...): one replica, whose
// records of this shard's node block sit as [n][1][2] quads under one counter
int sh_lp_kind(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    return (!c->lpm.lp || c->lpm.lpb) ? TW_ERR_INVALID : TW_OK;
}

int sh_lp_trace_state(tw_shard* c) {
    int rc = sh_lp_kind(c);
    if (rc) return rc;
    if (!c->d.trace || !c->d.trace_cap || !c->d.trace_n) return TW_ERR_STATE;
    return TW_OK;
}

int sh_lp_set_trace(tw_shard* c, uint32_t cap) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    if (!c->lpm.lp || c->lpm.lpb) return TW_ERR_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    trace_release(c->d);  // (Dev is the tick graph's key: the next tick captures the other variant)
    if (cap) {
        if (hipMalloc(&c->d.trace, (size_t)cap * 32) != hipSuccess || hipMalloc(&c->d.trace_n, 8) != hipSuccess) {
            (void)hipGetLastError();  // (not sticky: the context stays usable, tracing off)
            trace_release(c->d);
            return TW_ERR_OOM;
        }
        HIPCHK(hipMemsetAsync(c->d.trace_n, 0, 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->d.trace_cap = cap;
    }
    return TW_OK;
}

int sh_lp_trace_count(tw_shard* c, uint64_t* n) {
    int rc = sh_lp_trace_state(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(n, c->d.trace_n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return TW_OK;
}

int sh_lp_trace_fetch(tw_shard* c, tw_trace_rec* out, size_t k) {
    int rc = sh_lp_trace_state(c);
    if (rc) return rc;
    if (k > c->d.trace_cap) return TW_ERR_INVALID;
    if (!k) return TW_OK;
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint4> buf(2 * k);
    HIPCHK(hipMemcpyAsync(buf.data(), c->d.trace, k * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < k; ++i) {
        const uint4 a = buf[2 * i], b = buf[2 * i + 1];
        out[i].t = (int64_t)(((uint64_t)a.y << 32) | a.x);
        out[i].val = (int64_t)(((uint64_t)b.y << 32) | b.x);
        out[i].node = a.z;
        out[i].tag = a.w;
    }
    return TW_OK;
}

const uint4* sh_lp_trace_dev(tw_shard* c) { return c->d.trace; }
hipStream_t sh_stream(tw_shard* c) { return c->stream; }

int sh_measure_state(tw_shard* c) {
    if (!c) return TW_ERR_INVALID;
    if (!c->loaded) return TW_ERR_STATE;
    // as sh_set_trace: node-partitioned contexts keep no TRACE records.  A
    // batched LP context with tracing off keeps answering TW_ERR_INVALID too
    // (what it answered before it could trace), not TW_ERR_STATE
    if (c->lpm.lp && (!c->lpm.lpb || !c->d.trace || !c->d.trace_cap || !c->d.trace_n)) return TW_ERR_INVALID;
    if (!c->d.trace || !c->d.trace_cap) return TW_ERR_STATE;
    return TW_OK;
}

int sh_measure(tw_shard* c, const tw_measure_spec* spec, const MeasureCfg& cfg, tw_measure_out* total, uint64_t* hist,
               tw_measure_out* per, double* kernel_ms, double* phase_ms, MeasureEmit* emit) {
    int rc = sh_measure_state(c);
    if (rc) return rc;
    const Dev& d = c->d;
    if (c->lpm.lpb)  // (one count per replica in trace_n; d.R counts lanes)
        return measure_run(c->device, c->stream, d.trace, d.trace_n, c->lpm.n_rep, d.trace_cap, spec, cfg, total, hist, per,
                           kernel_ms, phase_ms, emit);
    return measure_run(c->device, c->stream, d.trace, d.scal + (size_t)SC_TRACE_N * d.R, d.R, d.trace_cap, spec, cfg,
                       total, hist, per, kernel_ms, phase_ms, emit);
}

int sh_measure_series(tw_shard* c, const tw_series_spec* spec, const MeasureCfg& cfg, uint64_t max_entries,
                      tw_series_out* total, uint64_t* count, tw_series_stat* stat, tw_series_out* per,
                      uint64_t* per_count, double* phase_ms) {
    int rc = sh_measure_state(c);
    if (rc) return rc;
    const Dev& d = c->d;
    // (FIRST's table: a record's node is one of the scenario's, d.Ntot of them per replica)
    if (c->lpm.lpb)
        return series_run(c->device, c->stream, d.trace, d.trace_n, c->lpm.n_rep, d.trace_cap, d.Ntot, max_entries, spec,
                          cfg, total, count, stat, per, per_count, phase_ms);
    return series_run(c->device, c->stream, d.trace, d.scal + (size_t)SC_TRACE_N * d.R, d.R, d.trace_cap, d.Ntot,
                      max_entries, spec, cfg, total, count, stat, per, per_count, phase_ms);
}

int sh_lp_measure_series(tw_shard* c, const tw_series_spec* spec, const MeasureCfg& cfg, uint64_t max_entries,
                         tw_series_out* total, uint64_t* count, double* phase_ms) {
    int rc = sh_lp_trace_state(c);
    if (rc) return rc;
    const Dev& d = c->d;
    // one replica; the records carry the scenario's node numbers, so the table
    // spans all of them although only this shard's block occurs
    return series_run(c->device, c->stream, d.trace, d.trace_n, 1, d.trace_cap, d.Ntot, max_entries, spec, cfg, total,
                      count, nullptr, nullptr, nullptr, phase_ms);
}

int sh_last_launch_ms(tw_shard* c, double* out, size_t cap) {
    if (!c || !out) return TW_ERR_INVALID;
    const std::vector<double>& ms = c->times.ms;
    size_t n = ms.size() < cap ? ms.size() : cap;
    for (size_t i = 0; i < n; ++i) out[i] = ms[i];
    return (int)n;
}

}  // namespace tw
