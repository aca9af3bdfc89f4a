// run_state.hpp -- host-only state of a context (engine.hip's tw_shard): the
// timed launches, the killThread sweeps, the send-free prefix, the run's
// statistics buffers, the LP modes, the device loop's exchange and its tick
// graph.  Each feature's state is one member of tw_shard and knows how to reset
// itself: a field added here goes back to its default at a tw_load unless
// `unload` carries it over, and a feature that owns device or pinned memory
// frees it here and nowhere else (DESIGN §3p has the table).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/timewarp.h"
#include "prefix_dev.hpp"
#include "sweep_dev.hpp"

#define HIPCHK(x)                                     \
    do {                                              \
        hipError_t _e = (x);                          \
        if (_e != hipSuccess) {                       \
            fprintf(stderr, "timewarp: %s failed: %s\n", #x, hipGetErrorString(_e)); \
            return _e == hipErrorOutOfMemory ? TW_ERR_OOM : TW_ERR_HIP; \
        }                                             \
    } while (0)

// Device times of a tw_run, measured between HIP events.  `timed` records a
// begin / end pair around whatever `enqueue` puts on the stream; after the
// caller's next sync, `read` takes the elapsed times in the order they were
// recorded, appends each to `ms` (tw_last_launch_ms: observable order, DESIGN
// §3n) and adds it to `total` (tw_stats.kernel_ms) and to the pair's `also`.
struct LaunchTimes {
    std::vector<double> ms;
    double total = 0.0;
    std::vector<hipEvent_t> pool;   // pairs, reused by every run
    std::vector<double*> pending;   // `also` of the pairs recorded since the last read

    void start() {
        ms.clear();
        total = 0.0;
        pending.clear();
    }
    template <class F>
    int timed(hipStream_t st, F&& enqueue, double* also = nullptr) {
        const size_t i = 2 * pending.size();
        while (pool.size() < i + 2) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            pool.push_back(e);
        }
        HIPCHK(hipEventRecord(pool[i], st));
        const int rc = enqueue();
        if (rc) return rc;
        HIPCHK(hipEventRecord(pool[i + 1], st));
        pending.push_back(also);
        return TW_OK;
    }
    int read() {
        for (size_t k = 0; k < pending.size(); ++k) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, pool[2 * k], pool[2 * k + 1]));
            ms.push_back(t);
            total += t;
            if (pending[k]) *pending[k] += t;
        }
        pending.clear();
        return TW_OK;
    }
    void destroy() {
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

// killThread sweeps (sweep.hip): the classifier's tables and the
// sweep kernels' scratch (tab.stub null: no kill stub in the image, or no
// memory for the scratch; the device memory is the context's, freed with its
// other allocations), the image's sweep times, which of them were swept since
// the last tw_reset, and the last tw_run's counts
struct Sweep {
    bool on = true;                     // tw_set_sweep; on after every load
    tw::SweepTab tab{};
    std::vector<int64_t> times;
    std::vector<uint32_t> stub_h;       // host copy of tab.stub (the kill table's builder reads it)
    uint32_t done = 0;
    unsigned long long* h = nullptr;    // pinned; outlives loads
    uint64_t last[3] = {0, 0, 0};
    uint64_t path[2] = {0, 0};          // ... its terminal replicas and effects-table entries (§3t)
    double ms = 0.0;                    // device time of the last tw_run's sweeps
    bool slow = false;                  // the testing hook TW_TEST_SWEEP_SLOW (read when the context is made)
    bool frames = false;                // ... and TW_TEST_SWEEP_FRAMES

    void unload() {
        Sweep z;
        z.h = h; z.ms = ms; z.slow = slow; z.frames = frames;
        for (int k = 0; k < 3; ++k) z.last[k] = last[k];
        for (int k = 0; k < 2; ++k) z.path[k] = path[k];
        *this = z;
    }
    void destroy() {
        unload();
        if (h) (void)hipHostFree(h);
        h = nullptr;
    }
};

// the send-free prefix (prefix.hip): the image's bound T0
// (prefix_classify.hpp; < 1: none), whether a tw_reset came since the last
// tw_run, and the one cached snapshot with its key -- tie mode and counter
// bases -- or, ok false, the pilot's refusal for that key.  The snapshot's
// device memory is its own (not among the context's allocations).
struct Prefix {
    bool on = true;                     // tw_set_prefix; on after every load
    bool fresh = false;
    int64_t t0 = 0;
    struct Snap {
        bool have = false, ok = false;
        uint32_t tie = 0, seq0 = 0, tid0 = 0;
        tw::PrefixTab tab{};
        uint32_t max_es = 0;
        uint64_t events = 0;            // events of a replica at the snapshot
        size_t bytes = 0;               // the snapshot's bytes per replica
        // Every row's class (prefix_clean.hpp RC_*) behind the
        // audit's count and the compact form's list (tab.list*), one device
        // block (audit null: none, every apply stores every row); the rows,
        // bytes per replica and (row, span) pairs of each class, and the
        // pairs of one 16-byte row
        unsigned long long* audit = nullptr;
        const uint8_t* cls = nullptr;
        uint64_t class_rows[tw::RC_COUNT] = {0, 0, 0, 0, 0}, class_bytes[tw::RC_COUNT] = {0, 0, 0, 0, 0};
        uint64_t class_pairs[tw::RC_COUNT] = {0, 0, 0, 0, 0}, pairs16 = 0;
        // Rows the apply may leave unstored (prefix_clean.hpp): the
        // kill table of sweep time T = Sweep::times[stop], built from this
        // snapshot; `dev` null: none.  One device block (table, windows, row
        // tags, dirty bytes, flag words) and the pinned copy of the dirty
        // bytes and flag words a verifying run leaves.
        struct Clean {
            void* dev = nullptr;
            const tw::KillEnt* kill = nullptr;
            const tw::KillWin* kwin = nullptr;
            const uint32_t* tag = nullptr;
            uint8_t* dirty = nullptr;           // [S], then the CF_COUNT flag words
            uint32_t* cflags = nullptr;
            uint8_t* h = nullptr;               // pinned: [S] dirty bytes + flag words
            std::vector<uint32_t> hdr_tags, run_tags;  // the tag of every RC_HDR / RC_RUN row
            // the sweep's terminal path (§3t): the effects rows (in `dev`) and the
            // clean bits, a block of their own; bits null: no memory, no such path
            const tw::EffEnt* eff = nullptr;
            unsigned long long* bits = nullptr;
            bool excl = false;
            uint32_t S = 0, stop = 0;
            std::vector<uint32_t> slots;        // the claimed slots
        } clean;
    } snap;
    uint32_t last = TW_PREFIX_NOT_ELIGIBLE;  // what the last tw_run did
    double ms = 0.0;                    // device time of the last tw_run's apply
    // §3o's validity rule.  chain: every replica's state derives from an apply
    // of this snapshot since the last tw_reset and only tw_run has written it
    // since; such a run's sweep at the table's time checks the replicas.
    // verified: the last tw_run's sweep published CF_VALID and nothing but
    // tw_reset and read-only calls came since: the next apply may skip rows.
    bool chain = false, verified = false;
    bool audit = false;                 // the testing hook TW_TEST_PREFIX_AUDIT (read when the context is made)
    // of the last apply: rows left unstored, bytes stored per replica; whether the last tw_run verified
    uint64_t rows_skipped = 0, bytes_stored = 0;
    // ... and of §3v's classes (header, run-entry and reset-valued rows, in
    // this order): rows and bytes per replica left unstored, bytes stored
    // form: 1 the grid over every row and span, 2 the compact list, over `pairs` workgroups
    struct Rows { uint64_t n[3] = {0, 0, 0}, bytes[3] = {0, 0, 0}, stored = 0, pairs = 0; uint32_t form = 0; } rows;
    bool rows_on = true;                // the testing hook TW_TEST_PREFIX_ROWS (read when the context is made)
    bool list_on = true;                // ... and TW_TEST_PREFIX_LIST: the apply's compact form
    bool last_verified = false;
    bool audited = false;               // the last apply ran the hook's audit (its counts: Snap::audit)

    // anything but tw_reset, tw_run and a read-only call: the flags no longer
    // describe the replicas
    void touch() { chain = verified = false; }
    // forget the cached snapshot (tw_load, tw_set_tie_mode, tw_set_counter_base)
    void drop() {
        if (snap.tab.rows) (void)hipFree((void*)snap.tab.rows);
        if (snap.tab.snap) (void)hipFree(snap.tab.snap);
        if (snap.audit) (void)hipFree(snap.audit);
        if (snap.clean.dev) (void)hipFree(snap.clean.dev);
        if (snap.clean.bits) (void)hipFree(snap.clean.bits);
        if (snap.clean.h) (void)hipHostFree(snap.clean.h);
        snap = Snap{};
        touch();
    }
    void unload() {
        drop();
        Prefix z;
        z.last = last; z.ms = ms; z.audit = audit; z.rows_on = rows_on; z.list_on = list_on;
        *this = z;
    }
};

// tw_run's statistics reduced on the device (tw_stats_kernel): the events
// column at the run's start, the 8 result words (both the feature's own,
// allocated by the first run that asks for statistics) and their pinned copy
struct StatBuf {
    uint64_t* ev0 = nullptr;
    unsigned long long* out = nullptr;
    unsigned long long* h = nullptr;    // pinned; outlives loads

    void unload() {
        if (ev0) (void)hipFree(ev0);
        if (out) (void)hipFree(out);
        ev0 = nullptr;
        out = nullptr;
    }
    void destroy() {
        unload();
        if (h) (void)hipHostFree(h);
        h = nullptr;
    }
};

// The TRACE buffer (tw_set_trace).  Dev holds its pointers, for the kernels;
// the buffer is its own (not among the context's allocations) and this is its
// one release: a new tw_set_trace, and every unload.
inline void trace_release(tw::Dev& d) {
    if (d.trace) (void)hipFree(d.trace);
    if (d.trace_n) (void)hipFree(d.trace_n);
    d.trace = nullptr;
    d.trace_n = nullptr;
    d.trace_cap = 0;
}

// The LP modes (tw_lp_load, tw_lpb_load): what the load decided and the
// host-driven window's buffers (among the context's allocations)
struct LpMode {
    bool lp = false;
    bool lpb = false;               // batched LP (tw_lpb_load): R = nodes x replicas
    uint32_t n_rep = 1;             // replicas batched per node
    bool heavy_ok = false;          // some node's inbox can exceed TW_LIGHT (tw_lp_due runs)
    bool has_ph1 = false;           // two-phase windows (Dev::phase)
    bool fresh = false;             // tw_reset since the last batched-LP tw_run: every counter is 0
    // tw_set_trace_batch (off after every load), and its value at the last
    // tw_reset: what lp_window_start launches while tracing is on
    bool trace_bat = false, trace_bat_run = false;
    uint64_t windows = 0, ticks = 0;  // of the last batched-LP tw_run; outlive loads, like the sweeps' counts
    uint4* foreign = nullptr;       // [out_cap][2]
    uint32_t* n_foreign = nullptr;
    uint4* staging = nullptr;       // inject staging [out_cap][2]

    void unload() {
        LpMode z;
        z.windows = windows; z.ticks = ticks;
        *this = z;
    }
};

// device-driven windows (tw_lp_exchange_setup / sh_lp_exchange_own): blocks of
// `cap` records (the stride) of which the first cap_eff go over the wire this
// tick (<= cap; the library loop adapts it).  The exchange owns `starts`, `own`
// and `carry`; `send`, `recv` and `red` point into `own` or are the caller's;
// win_buf and red_own are among the context's allocations.
struct Exchange {
    uint32_t world = 1, rank = 0, cap = 0, cap_eff = 0;
    uint32_t* starts = nullptr;       // device, world + 1
    uint4* send = nullptr;            // caller's device buffers (or own's)
    uint4* recv = nullptr;
    int64_t* red = nullptr;           // caller's (or red_own, or own's)
    int64_t* red_own = nullptr;
    void* own = nullptr;              // library-owned send | recv | red (sh_lp_exchange_own)
    void* carry = nullptr;            // Dev::carry + carry_n
    int64_t* win_buf = nullptr;       // the device loop's WN_* words
    int64_t* h_win = nullptr;         // pinned host copy of them + lp_err (tw_lp_progress); outlives loads
    bool loop_ready = false;

    // Dev's view of the carry block: counts in its first 256 bytes, then the records
    void set_carry(tw::Dev& d, uint32_t records) const {
        d.carry_n = carry ? (uint32_t*)carry : nullptr;
        d.carry = carry ? (uint4*)((char*)carry + 256) : nullptr;
        d.carry_cap = carry ? records : 0u;
    }
    // forget the ranks and free the blocks the exchange owns (a new setup, unload)
    void drop(tw::Dev& d) {
        if (starts) (void)hipFree(starts);
        if (own) (void)hipFree(own);
        if (carry) (void)hipFree(carry);
        starts = nullptr;
        own = carry = nullptr;
        set_carry(d, 0);
        send = recv = nullptr;
        red = nullptr;
        world = 1;
        rank = cap = cap_eff = 0;
    }
    void unload(tw::Dev& d) {
        drop(d);
        Exchange z;
        z.h_win = h_win;
        *this = z;
    }
    void destroy(tw::Dev& d) {
        unload(d);
        if (h_win) (void)hipHostFree(h_win);
        h_win = nullptr;
    }
};

// sh_lp_run_windows: TW_GRAPH_TICKS ticks + the progress copy captured as one
// hipGraph (a tick is 4-8 short kernels: launched one by one, the host's
// enqueue rate left the device idle between them), re-captured when the
// launch arguments it holds change (key)
struct TickGraph {
    hipGraphExec_t exec = nullptr;
    std::vector<unsigned char> key;

    void unload() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
        key.clear();
    }
};
