// measure_select.hip — tw_measure_quantiles' selects (include/timewarp.h) over
// the latencies that the join's emit variant left in device memory
// (measure.hip: tw_measure_join<true> / tw_measure_join_large<true>; the layout
// is MeasureEmit's, shard.hpp).  Everything that needs no device -- the index
// arithmetic, the sign-biased key and its digits, the digit step -- is
// measure_select.hpp's, compiled here and on the host from the same text.
//   tw_quantile_replicas  one workgroup takes a replica at a time (a fixed
//     grid walks them).  Up to lds_cap latencies (QS_LDS_MAX = 2,048 unless the
//     testing hook lowers it; the LDS join's replicas hold at most 1,024 pairs)
//     are bitonic-sorted in LDS as keys over the next power of two, padded with
//     the largest key (padding sorts last, and only indices below n are read),
//     and each quantile's two indices are read off.  A longer segment is
//     radix-selected, most significant digit first: every order statistic asked
//     for keeps a prefix and a residual rank; a pass counts, for each, the next
//     digit of the keys that match its prefix, in an LDS histogram of 256 bins
//     per order statistic, and one lane per order statistic takes the step.
//   tw_quantile_count     the batch-wide select's pass: a wave takes a replica
//     at a time and counts the digit at `shift` of every key that matches a
//     rank's prefix above it, into the workgroup's LDS histogram, flushed with
//     one global atomic per non-empty bin.  The host (abi.hip) sums the shards'
//     histograms and takes the steps.
// No lane waits for another; every barrier is under a workgroup-uniform
// condition (the replica, its fill count and lds_cap are the workgroup's).
// LDS: 16 KiB of keys + 32 KiB of histogram + 512 B: 3 workgroups per CU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/timewarp.h"
#include "measure_select.hpp"
#include "shard.hpp"

namespace {

using namespace tw;

constexpr uint32_t QS_WG = 256;
constexpr uint32_t QS_GRID = 768;  // 256 CUs x 3 workgroups
static_assert((QS_LDS_MAX & (QS_LDS_MAX - 1)) == 0, "the bitonic sort pads to a power of two within s_key");
static_assert(QS_LDS_MAX * 8 + QS_MAX_RANKS * QS_DIGITS * 4 + QS_MAX_RANKS * 16 + 256 <= 64 * 1024, "static LDS");

struct QsAsk {  // a call's quantiles, by value
    uint32_t n_q;
    uint32_t q_ppm[TW_MEASURE_MAX_QUANTILES];
};
struct QsPass {  // a pass of the batch-wide select, by value
    uint32_t n, shift;
    unsigned long long prefix[QS_MAX_RANKS];
};

// the keys of seg[0 .. n) that match prefix[j] above `shift`, by digit, into
// hist[j][digit]; lane i of `lanes` starts at i
__device__ __forceinline__ void qs_count(const long long* __restrict__ seg, uint32_t n, uint32_t i0, uint32_t lanes,
                                         const unsigned long long* prefix, uint32_t nk, uint32_t shift,
                                         uint32_t* hist) {
    for (uint32_t i = i0; i < n; i += lanes) {
        const uint64_t key = qs_key((int64_t)seg[i]);
        const uint32_t d = qs_digit(key, shift);
        for (uint32_t j = 0; j < nk; ++j)
            if (qs_match(key, prefix[j], shift)) atomicAdd(&hist[j * QS_DIGITS + d], 1u);
    }
}

__global__ __launch_bounds__(QS_WG) void tw_quantile_replicas(const long long* __restrict__ lat,
                                                              const unsigned long long* __restrict__ off,
                                                              const uint32_t* __restrict__ fill, uint32_t R, QsAsk ask,
                                                              uint32_t lds_cap, tw_quantile* __restrict__ out) {
    __shared__ unsigned long long s_key[QS_LDS_MAX];
    __shared__ uint32_t s_hist[QS_MAX_RANKS * QS_DIGITS];
    __shared__ unsigned long long s_prefix[QS_MAX_RANKS];
    __shared__ unsigned long long s_k[QS_MAX_RANKS];
    const uint32_t tid = threadIdx.x;
    const uint32_t nk = 2 * ask.n_q;  // (lo, hi) of every quantile: <= QS_MAX_RANKS

    for (uint32_t r = blockIdx.x; r < R; r += gridDim.x) {
        const unsigned long long at = off[r], room = off[r + 1] - at;
        const uint32_t n = fill[r] < room ? fill[r] : (uint32_t)room;  // (the join filled no more than the segment)
        const long long* seg = lat + at;
        tw_quantile* o = out + (size_t)r * ask.n_q;
        if (n == 0) {
            if (tid < ask.n_q) o[tid] = tw_quantile{INT64_MAX, INT64_MIN};
            continue;
        }
        uint64_t lo = 0, hi = 0;  // lanes below n_q: quantile tid's indices
        if (tid < ask.n_q) qs_index(ask.q_ppm[tid], n, &lo, &hi);
        if (n <= lds_cap) {
            const uint32_t P = n > 1 ? 1u << (32 - __clz(n - 1)) : 1u;  // <= QS_LDS_MAX
            for (uint32_t i = tid; i < P; i += QS_WG) s_key[i] = i < n ? qs_key((int64_t)seg[i]) : ~0ull;
            __syncthreads();
            for (uint32_t k = 2; k <= P; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t i = tid; i < P; i += QS_WG) {
                        const uint32_t x = i ^ j;
                        if (x > i) {
                            const unsigned long long a = s_key[i], b = s_key[x];
                            if ((a > b) == ((i & k) == 0)) {
                                s_key[i] = b;
                                s_key[x] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            if (tid < ask.n_q) o[tid] = tw_quantile{qs_unkey(s_key[lo]), qs_unkey(s_key[hi])};
            __syncthreads();  // (the next replica's keys overwrite these)
            continue;
        }
        // order statistic 2 q is quantile q's lo, 2 q + 1 its hi
        if (tid < ask.n_q) {
            s_prefix[2 * tid] = s_prefix[2 * tid + 1] = 0;
            s_k[2 * tid] = lo;
            s_k[2 * tid + 1] = hi;
        }
        for (uint32_t left = 8; left > 0; --left) {
            const uint32_t shift = (left - 1) * QS_DIGIT_BITS;
            for (uint32_t i = tid; i < nk * QS_DIGITS; i += QS_WG) s_hist[i] = 0;
            __syncthreads();
            qs_count(seg, n, tid, QS_WG, s_prefix, nk, shift, s_hist);
            __syncthreads();
            if (tid < nk) {
                uint64_t k = s_k[tid];
                const uint32_t d = qs_step(s_hist + tid * QS_DIGITS, &k);  // (k < the counted: it is a rank among them)
                s_prefix[tid] |= (unsigned long long)(d & (QS_DIGITS - 1)) << shift;
                s_k[tid] = k;
            }
            __syncthreads();
        }
        if (tid < ask.n_q) o[tid] = tw_quantile{qs_unkey(s_prefix[2 * tid]), qs_unkey(s_prefix[2 * tid + 1])};
        __syncthreads();  // (the next replica resets the prefixes)
    }
}

__global__ __launch_bounds__(QS_WG) void tw_quantile_count(const long long* __restrict__ lat,
                                                           const unsigned long long* __restrict__ off,
                                                           const uint32_t* __restrict__ fill, uint32_t R, QsPass p,
                                                           unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_hist[QS_MAX_RANKS * QS_DIGITS];
    __shared__ unsigned long long s_prefix[QS_MAX_RANKS];
    const uint32_t tid = threadIdx.x;
    const uint32_t used = p.n * QS_DIGITS;
    for (uint32_t i = tid; i < used; i += QS_WG) s_hist[i] = 0;
    if (tid < p.n) s_prefix[tid] = p.prefix[tid];
    __syncthreads();
    const uint32_t waves = QS_WG / 64;
    for (uint64_t r = (uint64_t)blockIdx.x * waves + (tid >> 6); r < R; r += (uint64_t)gridDim.x * waves) {
        const unsigned long long at = off[r], room = off[r + 1] - at;
        const uint32_t n = fill[r] < room ? fill[r] : (uint32_t)room;
        qs_count(lat + at, n, tid & 63u, 64, s_prefix, p.n, p.shift, s_hist);
    }
    __syncthreads();
    for (uint32_t i = tid; i < used; i += QS_WG)
        if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
}

struct QsRes {  // a call's device scratch and events, released on every return path
    void* buf = nullptr;
    hipEvent_t ev[2] = {};
    ~QsRes() {
        if (buf) (void)hipFree(buf);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

#define QSCHK(x)                                                                     \
    do {                                                                             \
        hipError_t _e = (x);                                                         \
        if (_e != hipSuccess) {                                                      \
            fprintf(stderr, "timewarp: %s failed: %s\n", #x, hipGetErrorString(_e)); \
            return _e == hipErrorOutOfMemory ? TW_ERR_OOM : TW_ERR_HIP;              \
        }                                                                            \
    } while (0)

}  // namespace

namespace tw {

int select_replicas(int device, hipStream_t stream, const MeasureEmit& e, uint32_t R, const uint32_t* q_ppm,
                    uint32_t n_q, uint32_t lds_cap, tw_quantile* out, double* ms) {
    if (!q_ppm || n_q == 0 || n_q > TW_MEASURE_MAX_QUANTILES || lds_cap > QS_LDS_MAX || !out) return TW_ERR_INVALID;
    if (ms) *ms = 0.0;
    if (R == 0) return TW_OK;
    if (!e.off || !e.fill || !e.lat) return TW_ERR_STATE;
    QsRes res;
    QSCHK(hipSetDevice(device));
    const size_t bytes = (size_t)R * n_q * sizeof(tw_quantile);
    if (hipMalloc(&res.buf, bytes) != hipSuccess) {
        (void)hipGetLastError();  // (not sticky: the context stays usable)
        return TW_ERR_OOM;
    }
    for (hipEvent_t& ev : res.ev) QSCHK(hipEventCreate(&ev));
    QsAsk ask{};
    ask.n_q = n_q;
    for (uint32_t i = 0; i < n_q; ++i) ask.q_ppm[i] = q_ppm[i];
    QSCHK(hipEventRecord(res.ev[0], stream));
    tw_quantile_replicas<<<R < QS_GRID ? R : QS_GRID, QS_WG, 0, stream>>>(e.lat, e.off, e.fill, R, ask, lds_cap,
                                                                         (tw_quantile*)res.buf);
    QSCHK(hipGetLastError());
    QSCHK(hipEventRecord(res.ev[1], stream));
    std::vector<tw_quantile> h((size_t)R * n_q);
    QSCHK(hipMemcpyAsync(h.data(), res.buf, bytes, hipMemcpyDeviceToHost, stream));
    QSCHK(hipStreamSynchronize(stream));
    float t = 0.f;
    QSCHK(hipEventElapsedTime(&t, res.ev[0], res.ev[1]));
    std::copy(h.begin(), h.end(), out);
    if (ms) *ms = t;
    return TW_OK;
}

int select_count(int device, hipStream_t stream, const MeasureEmit& e, uint32_t R, const uint64_t* prefix,
                 uint32_t n_ranks, uint32_t shift, uint64_t* hist, double* ms) {
    if (!prefix || n_ranks == 0 || n_ranks > QS_MAX_RANKS || shift > 56 || shift % QS_DIGIT_BITS || !hist)
        return TW_ERR_INVALID;
    if (ms) *ms = 0.0;
    if (R == 0) return TW_OK;
    if (!e.off || !e.fill || !e.lat || !e.digits) return TW_ERR_STATE;
    QsRes res;
    QSCHK(hipSetDevice(device));
    for (hipEvent_t& ev : res.ev) QSCHK(hipEventCreate(&ev));
    QsPass p{};
    p.n = n_ranks;
    p.shift = shift;
    for (uint32_t j = 0; j < n_ranks; ++j) p.prefix[j] = prefix[j];
    const size_t bytes = (size_t)n_ranks * QS_DIGITS * 8;
    // a wave per replica; a workgroup's LDS counters are 32-bit: at most 1,024
    // replicas of <= 2^21 pairs each per workgroup
    uint32_t grid = (R + 3) / 4 < QS_GRID ? (R + 3) / 4 : QS_GRID;
    const uint32_t need = (uint32_t)(((uint64_t)R + 1023) >> 10);
    if (grid < need) grid = need;
    QSCHK(hipMemsetAsync(e.digits, 0, bytes, stream));
    QSCHK(hipEventRecord(res.ev[0], stream));
    tw_quantile_count<<<grid, QS_WG, 0, stream>>>(e.lat, e.off, e.fill, R, p, e.digits);
    QSCHK(hipGetLastError());
    QSCHK(hipEventRecord(res.ev[1], stream));
    std::vector<uint64_t> h((size_t)n_ranks * QS_DIGITS);
    QSCHK(hipMemcpyAsync(h.data(), e.digits, bytes, hipMemcpyDeviceToHost, stream));
    QSCHK(hipStreamSynchronize(stream));
    float t = 0.f;
    QSCHK(hipEventElapsedTime(&t, res.ev[0], res.ev[1]));
    for (size_t i = 0; i < h.size(); ++i) hist[i] += h[i];
    if (ms) *ms = t;
    return TW_OK;
}

}  // namespace tw
