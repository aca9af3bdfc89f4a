// measure_combine.hpp — the host half of tw_measure (include/timewarp.h) that
// needs no HIP: the spec check, the empty value of a tw_measure_out, and the
// fold of one shard's outputs into the context's (totals and histogram summed,
// min of the mins, max of the maxes, the shard's per-replica block placed at
// its first replica).  Kept free of HIP so it compiles into a plain host
// program (tests/measure_combine_main.cpp, run under ASan / UBSan).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/timewarp.h"

namespace tw {

inline bool measure_spec_ok(const tw_measure_spec* s) {
    return s && s->tag_from != s->tag_to && s->n_bins >= 1 && s->n_bins <= TW_MEASURE_MAX_BINS && s->reserved == 0 &&
           s->bin_us >= 1;
}

inline void measure_empty(tw_measure_out* o) {
    std::memset(o, 0, sizeof(*o));
    o->min_us = INT64_MAX;
    o->max_us = INT64_MIN;
}

inline void measure_add(tw_measure_out* acc, const tw_measure_out* p) {
    acc->pairs += p->pairs;
    acc->open_from += p->open_from;
    acc->open_to += p->open_to;
    acc->repeated += p->repeated;
    acc->truncated += p->truncated;
    acc->underflow += p->underflow;
    acc->overflow += p->overflow;
    if (p->min_us < acc->min_us) acc->min_us = p->min_us;
    if (p->max_us > acc->max_us) acc->max_us = p->max_us;
    acc->sum_us = (int64_t)((uint64_t)acc->sum_us + (uint64_t)p->sum_us);  // two's complement
}

// Fold a shard's outputs (s_total, s_hist[n_bins] or NULL, s_per[s_n] or NULL)
// into the context's (total, hist or NULL, per[n] or NULL); the shard's
// replicas are the context's [rep0, rep0 + s_n).  False when the block does
// not fit in per[n]; nothing is written then.
inline bool measure_combine(tw_measure_out* total, uint64_t* hist, uint32_t n_bins, tw_measure_out* per, size_t n,
                            const tw_measure_out* s_total, const uint64_t* s_hist, const tw_measure_out* s_per,
                            size_t rep0, size_t s_n) {
    if (per && s_per && (rep0 > n || s_n > n - rep0)) return false;
    measure_add(total, s_total);
    if (hist && s_hist)
        for (uint32_t b = 0; b < n_bins; ++b) hist[b] += s_hist[b];
    if (per && s_per && s_n) std::memcpy(per + rep0, s_per, s_n * sizeof(tw_measure_out));
    return true;
}

}  // namespace tw
