// lp_trace_plan.hpp — the host half of tw_lp_read_trace / tw_lp_measure
// (include/timewarp.h) that needs no HIP.  A node-partitioned context keeps
// its TRACE records per shard (each shard up to the context's cap, under its
// own emitted count); this header turns the shards' counts into the context's
// view of them:
//   * E, the records the context emitted: the sum of the shards' counts;
//   * truncated iff E > cap -- a rule that does not know the shard count
//     (when E <= cap no shard passed the cap, so every shard kept everything);
//   * what each shard kept (min(count, cap)) and where its block starts in
//     the gathered buffer tw_lp_measure joins (the prefix sums);
//   * the canonical order (t, node, tag, val), the k-way merge of the shards'
//     sorted lists into it, and the clipping to the caller's buffer.
// Kept free of HIP so it compiles into a plain host program
// (tests/lp_trace_plan_main.cpp, run under ASan / UBSan).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/timewarp.h"

namespace tw {

struct LpTracePlan {
    uint64_t emitted = 0;        // E
    bool truncated = false;      // E > cap
    std::vector<uint64_t> kept;  // per shard: min(count, cap)
    std::vector<uint64_t> off;   // per shard: first record of its block in the gathered buffer
    uint64_t gathered = 0;       // sum of kept (== E when not truncated)
};

inline LpTracePlan lp_trace_plan(const uint64_t* counts, size_t n_shards, uint64_t cap) {
    LpTracePlan p;
    p.kept.resize(n_shards);
    p.off.resize(n_shards);
    bool wrapped = false;
    for (size_t i = 0; i < n_shards; ++i) {
        if (p.emitted + counts[i] < p.emitted) wrapped = true;  // (counts are 64-bit: not by any run)
        p.emitted += counts[i];
        p.kept[i] = counts[i] < cap ? counts[i] : cap;
        p.off[i] = p.gathered;
        p.gathered += p.kept[i];
    }
    if (wrapped) p.emitted = UINT64_MAX;
    p.truncated = p.emitted > cap;
    return p;
}

// records handed to the caller: min(caller's cap, E, the trace cap)
inline size_t lp_trace_clip(uint64_t emitted, uint64_t trace_cap, size_t caller_cap) {
    uint64_t k = emitted < trace_cap ? emitted : trace_cap;
    return k < (uint64_t)caller_cap ? (size_t)k : caller_cap;
}

// the canonical order (tw_read_trace's for batched LP contexts)
inline bool lp_trace_less(const tw_trace_rec& a, const tw_trace_rec& b) {
    if (a.t != b.t) return a.t < b.t;
    if (a.node != b.node) return a.node < b.node;
    if (a.tag != b.tag) return a.tag < b.tag;
    return a.val < b.val;
}

inline void lp_trace_sort(tw_trace_rec* r, size_t n) { std::sort(r, r + n, lp_trace_less); }

// Merge n_lists lists, each in canonical order, into out: the first
// min(out_cap, sum of lens) records of the merged order.  Equal records come
// out in list order.  Returns the number written.
inline size_t lp_trace_merge(const tw_trace_rec* const* lists, const uint64_t* lens, size_t n_lists, tw_trace_rec* out,
                             size_t out_cap) {
    std::vector<uint64_t> at(n_lists, 0);
    size_t w = 0;
    while (w < out_cap) {
        size_t best = n_lists;
        for (size_t i = 0; i < n_lists; ++i) {
            if (at[i] >= lens[i]) continue;
            if (best == n_lists || lp_trace_less(lists[i][at[i]], lists[best][at[best]])) best = i;
        }
        if (best == n_lists) break;
        out[w++] = lists[best][at[best]++];
    }
    return w;
}

}  // namespace tw
