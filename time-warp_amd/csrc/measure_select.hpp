// measure_select.hpp — what tw_measure_quantiles (include/timewarp.h) needs
// that needs no device: the argument checks, the q_ppm -> (index_lo, index_hi)
// arithmetic, the order-preserving key of a signed latency and its digits, the
// common-prefix start of the batch-wide select, and the step "summed digit
// histogram + residual rank -> digit, new residual".  The kernels
// (measure_select.hip) and the host loop (abi.hip) compile the same text, as
// live_mod is (stdgen_dev.hpp); kept free of HIP so it also compiles into a
// plain host program (tests/measure_select_main.cpp, run under ASan / UBSan).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/timewarp.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TW_QS_HD __host__ __device__
#else
#define TW_QS_HD
#endif

namespace tw {

constexpr uint32_t QS_PPM = 1000000u;
constexpr uint32_t QS_DIGIT_BITS = 8, QS_DIGITS = 1u << QS_DIGIT_BITS;
constexpr uint32_t QS_MAX_RANKS = 2 * TW_MEASURE_MAX_QUANTILES;  // a quantile asks for two order statistics
constexpr uint32_t QS_NO_DIGIT = QS_DIGITS;                      // qs_step: the rank is not among the counted

// tw_measure_quantiles' own argument rules (the state and n checks are the ABI's)
inline bool quantile_args_ok(uint32_t tag_from, uint32_t tag_to, const uint32_t* q_ppm, uint32_t n_q) {
    if (tag_from == tag_to || !q_ppm || n_q == 0 || n_q > TW_MEASURE_MAX_QUANTILES) return false;
    for (uint32_t i = 0; i < n_q; ++i)
        if (q_ppm[i] > QS_PPM) return false;
    return true;
}

// pos = q_ppm * (n - 1) for n >= 1, as lo = pos div 10^6 and hi = lo + (pos mod
// 10^6 != 0).  Exact for every n up to 2^64 - 1: with n - 1 = a * 10^6 + b the
// product is (q * a) * 10^6 + q * b, where q * a <= n - 1 and q * b < 10^12, so
// no intermediate wraps and no 128-bit arithmetic is needed.  hi <= n - 1: the
// remainder is 0 at q_ppm == 10^6.
TW_QS_HD inline void qs_index(uint32_t q_ppm, uint64_t n, uint64_t* lo, uint64_t* hi) {
    const uint64_t a = (n - 1) / QS_PPM, b = (n - 1) % QS_PPM;
    const uint64_t qb = (uint64_t)q_ppm * b;
    *lo = (uint64_t)q_ppm * a + qb / QS_PPM;
    *hi = *lo + (qb % QS_PPM != 0 ? 1u : 0u);
}

// signed order as unsigned order: d ^ 2^63
TW_QS_HD inline uint64_t qs_key(int64_t d) { return (uint64_t)d ^ (1ull << 63); }
TW_QS_HD inline int64_t qs_unkey(uint64_t k) { return (int64_t)(k ^ (1ull << 63)); }
// the digit of key k at bit `shift` (a multiple of 8, 0 .. 56)
TW_QS_HD inline uint32_t qs_digit(uint64_t k, uint32_t shift) { return (uint32_t)(k >> shift) & (QS_DIGITS - 1); }
// k agrees with `prefix` in every bit above the digit at `shift`
TW_QS_HD inline bool qs_match(uint64_t k, uint64_t prefix, uint32_t shift) {
    return shift >= 56 || ((k ^ prefix) >> (shift + QS_DIGIT_BITS)) == 0;
}

// The digits that min and max share, most significant first, hold for every
// value between them: the select starts below them.  Returns the number of
// digits still to fix (0: min == max, every value is that one) and the shared
// bits in *prefix (the undecided digits zero).
TW_QS_HD inline uint32_t qs_start(int64_t min_us, int64_t max_us, uint64_t* prefix) {
    const uint64_t a = qs_key(min_us), b = qs_key(max_us);
    uint32_t left = 8;
    while (left > 0 && qs_digit(a, (left - 1) * QS_DIGIT_BITS) == qs_digit(b, (left - 1) * QS_DIGIT_BITS)) --left;
    *prefix = left == 8 ? 0 : (a >> (left * QS_DIGIT_BITS)) << (left * QS_DIGIT_BITS);
    return left;
}

// hist[d]: how many of the values that match the rank's prefix have digit d.
// The rank's value is the *k-th (from 0) of them: its digit is the first d
// whose running count passes *k, and *k becomes its rank among that digit's
// values.  QS_NO_DIGIT when fewer than *k + 1 values were counted (the
// caller's buffers disagree: an error, not a result).
template <typename Count>
TW_QS_HD inline uint32_t qs_step(const Count* hist, uint64_t* k) {
    uint64_t before = 0;
    for (uint32_t d = 0; d < QS_DIGITS; ++d) {
        const uint64_t c = (uint64_t)hist[d];
        if (*k - before < c) {
            *k -= before;
            return d;
        }
        before += c;
    }
    return QS_NO_DIGIT;
}

// The distinct order statistics a call's quantiles ask for among n >= 1
// values: rank[j] ascending, and for quantile i the positions lo_at[i] /
// hi_at[i] of its two in rank[].  At most QS_MAX_RANKS.
struct QsRanks {
    uint32_t n = 0;
    uint64_t rank[QS_MAX_RANKS];
    uint32_t lo_at[TW_MEASURE_MAX_QUANTILES], hi_at[TW_MEASURE_MAX_QUANTILES];
};
inline void qs_ranks(const uint32_t* q_ppm, uint32_t n_q, uint64_t n, QsRanks* out) {
    out->n = 0;
    auto place = [&](uint64_t r) {
        for (uint32_t j = 0; j < out->n; ++j)
            if (out->rank[j] == r) return j;
        out->rank[out->n] = r;
        return out->n++;
    };
    for (uint32_t i = 0; i < n_q; ++i) {
        uint64_t lo, hi;
        qs_index(q_ppm[i], n, &lo, &hi);
        out->lo_at[i] = place(lo);
        out->hi_at[i] = place(hi);
    }
}

// The batch-wide select's host state: every rank's prefix and residual rank,
// all at the same digit.  count(prefix[], residual-free, shift, hist) is the
// caller's pass over the values (the device kernel summed over the shards, or
// a loop over arrays in the host test): hist[j * QS_DIGITS + d] = values
// matching prefix[j] above `shift` whose digit there is d.  False when a pass
// fails or a rank is not among the values.
template <typename CountFn>
inline bool qs_select(const QsRanks& ranks, int64_t min_us, int64_t max_us, CountFn&& count, int64_t* out,
                      uint32_t* passes) {
    uint64_t prefix[QS_MAX_RANKS], k[QS_MAX_RANKS], hist[QS_MAX_RANKS * QS_DIGITS];
    uint64_t p0 = 0;
    uint32_t left = qs_start(min_us, max_us, &p0);
    for (uint32_t j = 0; j < ranks.n; ++j) {
        prefix[j] = p0;
        k[j] = ranks.rank[j];
    }
    if (passes) *passes = 0;
    while (left > 0) {
        const uint32_t shift = (left - 1) * QS_DIGIT_BITS;
        for (uint32_t i = 0; i < ranks.n * QS_DIGITS; ++i) hist[i] = 0;
        if (!count(prefix, ranks.n, shift, hist)) return false;
        for (uint32_t j = 0; j < ranks.n; ++j) {
            const uint32_t d = qs_step(hist + (size_t)j * QS_DIGITS, &k[j]);
            if (d == QS_NO_DIGIT) return false;
            prefix[j] |= (uint64_t)d << shift;
        }
        --left;
        if (passes) ++*passes;
    }
    for (uint32_t j = 0; j < ranks.n; ++j) out[j] = qs_unkey(prefix[j]);
    return true;
}

inline void quantile_empty(tw_quantile* q) {
    q->lo_us = INT64_MAX;
    q->hi_us = INT64_MIN;
}

}  // namespace tw
