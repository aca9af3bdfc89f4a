// sweep_dev.hpp — what engine.hip and sweep.hip share of the killThread sweep
// (DESIGN §3l): the sweep kernels' own tables, passed as a kernel argument
// of their own (Dev, the event kernels' argument, is unchanged).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tw_dev.hpp"
#include "prefix_clean.hpp"

namespace tw {

// per-replica accumulator words, [SW_*][R] u32, cleared by the scan:
// SW_BAD 0 swept so far / 1 refused / 2 nothing to sweep; killers, throwTos
// that hit a live victim, victims claimed, slots freed, the replica's next
// event outside the swept prefixes (two words), prefix length per run; then
// SW_NOTAB: some entry's refs came from its registers, not from the kill table
// (clear: the replica is table-bound, §3t); SW_FAST: entries applied from the
// effects table alone
enum { SW_BAD, SW_K, SW_H, SW_V, SW_FREE, SW_XLO, SW_XHI, SW_PL0, SW_NOTAB = SW_PL0 + TW_RUNS, SW_FAST, SW_COUNT };
// Sweep words of a tw_run, SweepTab::stats: kill wakes, victims and refused
// replicas; how many of the run's stops have been swept; replicas a later
// launch still has work for, as of the last sweep; replicas swept on the
// terminal path and entries applied from the effects table alone (§3t)
enum { SWS_KILLERS, SWS_VICTIMS, SWS_REFUSED, SWS_FIRED, SWS_LEFT, SWS_TERM, SWS_FAST, SWS_COUNT };

struct SweepTab {
    const uint32_t* stub;       // [n_insns + 1] stub word of each resume pc (sweep_classify.hpp)
    uint32_t* acc;              // [SW_COUNT][R]
    unsigned long long* stats;  // [SWS_COUNT]
    uint32_t near_cap;          // entries of the near spill per replica
    // The kill table of this sweep's time and the flags it proves clean rows
    // with (prefix_clean.hpp); kill null: none, the sweep as ever.
    const KillEnt* kill;        // the table's positions
    const KillWin* kwin;        // [TW_RUNS] each run's window of them
    uint8_t* dirty;             // [S] a claimed slot some replica's words did not match
    uint32_t* cflags;           // [CF_COUNT] (prefix_dev.hpp)
    // The table's effects rows and the clean bits validate publishes for apply
    // (DESIGN §3t); bits null: no terminal path, the sweep as in §3o.
    const EffEnt* eff;          // parallel to `kill`
    unsigned long long* bits;   // [table position][R / 64]: one ballot per wave and position
    uint32_t excl;              // every claimable position is exclusive
};

// The parked layout the event kernel's epilogue leaves (shared with prefix.hip):
// element index of replica 0's entry `pos` of far run j, and of quad q of the
// thread record in `slot`; replica r's lies r elements on.
__host__ __device__ __forceinline__ size_t run_row(const Dev& c, uint32_t j, uint32_t pos) {
    return ((size_t)j * c.Cr + pos) * c.R;
}
__host__ __device__ __forceinline__ size_t rec_row(const Dev& c, uint32_t slot, uint32_t q) {
    return (size_t)q * c.RQ + (size_t)slot * c.R;
}

size_t sweep_acc_words(uint32_t R);
// The sweep at time T of the run's stop number `expect`, on stream st, behind an
// event-kernel launch to T - 1: it runs if that launch left every replica
// parked and the stop has not been swept yet, and is a handful of empty
// kernels otherwise.  t_end: the run's, for the count of replicas with work left.
hipError_t sweep_launch(const Dev& d, const SweepTab& t, hipStream_t st, int64_t T, uint64_t max_events, int64_t t_end,
                        uint32_t expect);

}  // namespace tw
