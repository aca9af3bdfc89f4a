// measure_series.hpp — the half of tw_measure_series (include/timewarp.h) that
// needs no HIP: the spec check, the bin of a time (series_bin: the one rule the
// kernels of measure_series.hip and the host share), the empty values, the fold
// of one shard's outputs into the context's, and FIRST's chunk plan (how many
// replicas' first-time tables fit the scratch limit at once).  Kept free of HIP
// so it compiles into a plain host program (tests/measure_series_main.cpp, run
// under ASan / UBSan).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/timewarp.h"

#if defined(__HIPCC__)
#define TW_SERIES_HD __host__ __device__
#else
#define TW_SERIES_HD
#endif

namespace tw {

constexpr uint32_t SERIES_UNDER = 0xFFFFFFFFu;  // series_bin: t < t0_us
constexpr uint32_t SERIES_OVER = 0xFFFFFFFEu;   // series_bin: at or behind the last bin's end
// FIRST: entries (replicas x nodes, 8 B each) of one chunk's table at most
constexpr uint64_t SERIES_MAX_ENTRIES = 1ull << 25;
constexpr int SERIES_PHASES = 4;  // join + emit, table fill, binning, latency fold

inline bool series_spec_ok(const tw_series_spec* s) {
    if (!s || s->reserved != 0 || s->n_bins < 1 || s->t0_us < 0 || s->bin_us < 1) return false;
    switch (s->mode) {
        case TW_SERIES_EVENTS:
        case TW_SERIES_FIRST: return s->tag_to == 0 && s->n_bins <= TW_SERIES_MAX_BINS;
        case TW_SERIES_LATENCY: return s->tag_to != s->tag && s->n_bins <= TW_SERIES_MAX_LAT_BINS;
        default: return false;
    }
}

// The bin of time t, SERIES_UNDER or SERIES_OVER.  Compared first, subtracted
// afterwards: t >= t0_us >= 0, so the difference lies in 0 .. INT64_MAX.
TW_SERIES_HD inline uint32_t series_bin(int64_t t, int64_t t0_us, int64_t bin_us, uint32_t n_bins) {
    if (t < t0_us) return SERIES_UNDER;
    const uint64_t i = ((uint64_t)t - (uint64_t)t0_us) / (uint64_t)bin_us;
    return i >= n_bins ? SERIES_OVER : (uint32_t)i;
}

inline void series_empty(tw_series_out* o) {
    std::memset(o, 0, sizeof(*o));
    o->t_min = INT64_MAX;
    o->t_max = INT64_MIN;
}

inline void series_stat_empty(tw_series_stat* s) {
    s->sum_us = 0;
    s->min_us = INT64_MAX;
    s->max_us = INT64_MIN;
}

inline void series_add(tw_series_out* acc, const tw_series_out* p) {
    acc->counted += p->counted;
    acc->underflow += p->underflow;
    acc->overflow += p->overflow;
    acc->truncated += p->truncated;
    if (p->t_min < acc->t_min) acc->t_min = p->t_min;
    if (p->t_max > acc->t_max) acc->t_max = p->t_max;
}

inline void series_stat_add(tw_series_stat* acc, const tw_series_stat* p) {
    acc->sum_us = (int64_t)((uint64_t)acc->sum_us + (uint64_t)p->sum_us);  // two's complement
    if (p->min_us < acc->min_us) acc->min_us = p->min_us;
    if (p->max_us > acc->max_us) acc->max_us = p->max_us;
}

// Fold a shard's outputs into the context's: totals, counts and stats added (min
// of the mins, max of the maxes), the shard's per-replica blocks -- s_per[s_n],
// s_per_count[s_n][n_bins] -- placed at the shard's first replica rep0 of the
// context's n.  Any pair of pointers may be NULL.  False when a block does not
// fit; nothing is written then.
inline bool series_combine(tw_series_out* total, uint64_t* count, tw_series_stat* stat, uint32_t n_bins,
                           tw_series_out* per, uint64_t* per_count, size_t n, const tw_series_out* s_total,
                           const uint64_t* s_count, const tw_series_stat* s_stat, const tw_series_out* s_per,
                           const uint64_t* s_per_count, size_t rep0, size_t s_n) {
    if (((per && s_per) || (per_count && s_per_count)) && (rep0 > n || s_n > n - rep0)) return false;
    series_add(total, s_total);
    if (count && s_count)
        for (uint32_t b = 0; b < n_bins; ++b) count[b] += s_count[b];
    if (stat && s_stat)
        for (uint32_t b = 0; b < n_bins; ++b) series_stat_add(&stat[b], &s_stat[b]);
    if (per && s_per && s_n) std::memcpy(per + rep0, s_per, s_n * sizeof(tw_series_out));
    if (per_count && s_per_count && s_n)
        std::memcpy(per_count + rep0 * n_bins, s_per_count, s_n * (size_t)n_bins * sizeof(uint64_t));
    return true;
}

// FIRST's chunks: `per_chunk` replicas at a time (the last chunk fewer), their
// per_chunk x n_nodes table entries within `limit`.  per_chunk == 0: no plan
// (no nodes, or one replica's nodes alone exceed the limit).
struct SeriesChunks {
    uint32_t per_chunk = 0;
    uint32_t n_chunks = 0;
};

inline SeriesChunks series_chunks(uint32_t n_replicas, uint32_t n_nodes, uint64_t limit) {
    SeriesChunks p;
    if (n_nodes == 0 || limit == 0 || n_nodes > limit) return p;
    const uint64_t fit = limit / n_nodes;  // >= 1
    p.per_chunk = (uint32_t)(fit < n_replicas ? fit : (n_replicas ? n_replicas : 1));
    p.n_chunks = (uint32_t)(((uint64_t)n_replicas + p.per_chunk - 1) / p.per_chunk);
    return p;
}

// chunk k of the plan: replicas [first, first + count)
inline void series_chunk_at(const SeriesChunks& p, uint32_t n_replicas, uint32_t k, uint32_t* first, uint32_t* count) {
    const uint64_t f = (uint64_t)k * p.per_chunk;
    *first = (uint32_t)(f < n_replicas ? f : n_replicas);
    *count = n_replicas - *first < p.per_chunk ? n_replicas - *first : p.per_chunk;
}

}  // namespace tw
