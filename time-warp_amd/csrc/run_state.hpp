// run_state.hpp -- host-only state of tw_run's stages (engine.hip): the timed
// launches, the killThread sweeps and the send-free prefix.  Each feature's
// state is one member of tw_shard and knows how to reset itself: a field added
// here goes back to its default at a tw_load unless `unload` carries it over.
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
    uint32_t done = 0;
    unsigned long long* h = nullptr;    // pinned; outlives loads
    uint64_t last[3] = {0, 0, 0};
    double ms = 0.0;                    // device time of the last tw_run's sweeps

    void unload() {
        Sweep z;
        z.h = h; z.ms = ms;
        for (int k = 0; k < 3; ++k) z.last[k] = last[k];
        *this = z;
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
        size_t bytes = 0;               // bytes the apply writes per replica
    } snap;
    uint32_t last = TW_PREFIX_NOT_ELIGIBLE;  // what the last tw_run did
    double ms = 0.0;                    // device time of the last tw_run's apply

    // forget the cached snapshot (tw_load, tw_set_tie_mode, tw_set_counter_base)
    void drop() {
        if (snap.tab.rows) (void)hipFree((void*)snap.tab.rows);
        if (snap.tab.snap) (void)hipFree(snap.tab.snap);
        snap = Snap{};
    }
    void unload() {
        drop();
        Prefix z;
        z.last = last; z.ms = ms;
        *this = z;
    }
};
