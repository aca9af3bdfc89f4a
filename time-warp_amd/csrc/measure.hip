// measure.hip — tw_measure's device pass (include/timewarp.h): the LogReader's
// join of the bench/Network measure events (bench/Network/LogReader/Main.hs:
// 85-119) for every replica of a batch, reduced to the distribution of one
// latency t(tag_to) - t(tag_from).
//
// The TRACE records sit in HBM as [n][R][2] quads (tw_dev.hpp, written by
// Lane::trace_rec and the wave kernel), the same layout under every replica
// geometry, so one implementation serves dense / sparse / half / narrow /
// compact / wave -- and a batched LP context (tw_lpb_load), whose traced event
// kernel keeps the same [n][replicas][2] layout with one emitted count per
// replica (Dev::trace_n); there n is a claim order, no execution order, which
// the join (it groups by id) does not depend on.  Two kernels:
//   tw_measure_count  one lane per replica walks n = 0..kept over the [n][R]
//     layout (the lanes of a wave read neighbouring replicas: 32 B apart) and
//     counts the records whose tag is tag_from or tag_to; a replica that
//     emitted more than the trace cap is marked truncated; a count above
//     TW_MEASURE_MAX_KEYS sets the error word the host reads before the join
//     is launched;
//   tw_measure_join   one workgroup per replica at a time (a fixed grid walks
//     the replicas): gather the matching records as (val, t, side) keys into
//     LDS, bitonic-sort them by (val, side) over the next power of two
//     (padding slots carry a flag: every int64 is a legal id, so no sentinel
//     val exists), classify each id group from its first three keys, and
//     accumulate the replica's tw_measure_out plus a workgroup-private
//     histogram in LDS.  The histogram and the totals are flushed once per
//     workgroup, one global atomic per non-empty bin and per total.
// Everything is integer, so the order of the atomics cannot change a result.
//
// LDS per workgroup: 2048 keys x (8 B val + 8 B t + 1 B flags) = 34 KiB, the
// histogram 4096 x 4 B = 16 KiB, a few accumulators: ~50.1 KiB static, under
// the 64 KiB a workgroup may hold; 3 workgroups per CU of the 160 KiB.
//
// Out of scope: TRACE records of node-partitioned contexts (tw_lp_load:
// tw_set_trace refuses them -- one replica's nodes spread over contexts),
// records of tw_lp_batch (a traced LPB run keeps its due records on the
// lanes' chains instead), replicas with more than TW_MEASURE_MAX_KEYS
// matching records (no global-memory sort path), a job-wide reduction over
// ranks.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/timewarp.h"
#include "measure_combine.hpp"
#include "shard.hpp"

namespace {

constexpr uint32_t MS_WG = 256;
constexpr uint32_t MS_KEYS = TW_MEASURE_MAX_KEYS;
constexpr uint32_t MS_BINS = TW_MEASURE_MAX_BINS;
constexpr uint32_t MS_TRUNC = 0xFFFFFFFFu;  // cnt[r] of a truncated replica
constexpr uint32_t MS_GRID = 768;           // 256 CUs x 3 workgroups
static_assert((MS_KEYS & (MS_KEYS - 1)) == 0, "the bitonic sort pads to a power of two within the LDS arrays");
static_assert(MS_KEYS * 17 + MS_BINS * 4 + 256 <= 64 * 1024, "static LDS of tw_measure_join");

// key flags
constexpr uint8_t KF_TO = 1;   // side: 0 = tag_from, 1 = tag_to
constexpr uint8_t KF_PAD = 2;  // a padding slot: sorts after every key, val / t unset

__global__ __launch_bounds__(MS_WG) void tw_measure_count(const uint4* __restrict__ trace,
                                                          const uint64_t* __restrict__ emitted, uint32_t R,
                                                          uint32_t cap, uint32_t tag_from, uint32_t tag_to,
                                                          uint32_t* __restrict__ cnt, uint32_t* err,
                                                          tw_measure_out* total) {
    const uint32_t r = blockIdx.x * MS_WG + threadIdx.x;
    if (r == 0) {  // (the rest of *total was zeroed by the host's memset)
        total->min_us = INT64_MAX;
        total->max_us = INT64_MIN;
    }
    if (r >= R) return;
    const uint64_t em = emitted[r];
    if (em > cap) {
        cnt[r] = MS_TRUNC;
        return;
    }
    const uint32_t kept = (uint32_t)em;
    uint32_t k = 0;
    for (uint32_t n = 0; n < kept; ++n) {
        const uint32_t tag = trace[((size_t)n * R + r) * 2].w;
        k += (tag == tag_from || tag == tag_to) ? 1u : 0u;
    }
    cnt[r] = k;
    if (k > MS_KEYS) atomicOr(err, 1u);
}

struct MsKeys {
    int64_t val[MS_KEYS];
    int64_t t[MS_KEYS];
    uint8_t fl[MS_KEYS];
};

// key i sorts after key j: padding last, then by val (signed), then tag_from
// before tag_to
__device__ __forceinline__ bool ms_after(const MsKeys& k, uint32_t i, uint32_t j) {
    const uint8_t fi = k.fl[i], fj = k.fl[j];
    if ((fi | fj) & KF_PAD) return (fi & KF_PAD) > (fj & KF_PAD);
    const int64_t vi = k.val[i], vj = k.val[j];
    if (vi != vj) return vi > vj;
    return fi > fj;
}

__global__ __launch_bounds__(MS_WG) void tw_measure_join(const uint4* __restrict__ trace,
                                                         const uint64_t* __restrict__ emitted, uint32_t R,
                                                         uint32_t tag_from, uint32_t tag_to, uint32_t n_bins,
                                                         int64_t lo_us, int64_t bin_us,
                                                         const uint32_t* __restrict__ cnt, tw_measure_out* total,
                                                         unsigned long long* hist, tw_measure_out* per) {
    __shared__ MsKeys K;
    __shared__ uint32_t s_hist[MS_BINS];
    __shared__ uint32_t s_n;       // gather cursor
    __shared__ uint32_t s_cls[4];  // this replica's pairs, open_from, open_to, repeated
    __shared__ long long s_min, s_max;
    __shared__ unsigned long long s_sum;
    __shared__ unsigned long long s_uf, s_of;  // the workgroup's under / overflow
    const uint32_t tid = threadIdx.x;

    for (uint32_t b = tid; b < n_bins; b += MS_WG) s_hist[b] = 0;
    if (tid == 0) s_uf = s_of = 0;
    tw_measure_out wg;  // the workgroup's totals (thread 0)
    wg.pairs = wg.open_from = wg.open_to = wg.repeated = wg.truncated = 0;
    wg.min_us = INT64_MAX;
    wg.max_us = INT64_MIN;
    wg.sum_us = 0;

    // r and cnt[r] depend on the workgroup alone: every branch that holds a
    // barrier below is taken by the whole workgroup or by none of it
    for (uint32_t r = blockIdx.x; r < R; r += gridDim.x) {
        const uint32_t m = cnt[r];
        if (m == MS_TRUNC) {
            if (tid == 0) {
                ++wg.truncated;
                if (per) {
                    tw_measure_out o{};
                    o.truncated = 1;
                    o.min_us = INT64_MAX;
                    o.max_us = INT64_MIN;
                    per[r] = o;
                }
            }
            continue;
        }
        if (tid == 0) {
            s_n = 0;
            s_cls[0] = s_cls[1] = s_cls[2] = s_cls[3] = 0;
            s_min = INT64_MAX;
            s_max = INT64_MIN;
            s_sum = 0;
        }
        __syncthreads();
        if (m != 0 && m <= MS_KEYS) {
            // gather (slot order is arbitrary: the sort follows)
            const uint32_t kept = (uint32_t)emitted[r];
            for (uint32_t n = tid; n < kept; n += MS_WG) {
                const uint4* q = trace + ((size_t)n * R + r) * 2;
                const uint4 a = q[0];
                if (a.w == tag_from || a.w == tag_to) {
                    const uint4 b = q[1];
                    const uint32_t slot = atomicAdd(&s_n, 1u);
                    if (slot < m) {
                        K.val[slot] = (int64_t)(((uint64_t)b.y << 32) | b.x);
                        K.t[slot] = (int64_t)(((uint64_t)a.y << 32) | a.x);
                        K.fl[slot] = a.w == tag_to ? KF_TO : 0;
                    }
                }
            }
            const uint32_t P = m > 1 ? 1u << (32 - __clz(m - 1)) : 1u;  // <= MS_KEYS
            for (uint32_t i = m + tid; i < P; i += MS_WG) K.fl[i] = KF_PAD;
            __syncthreads();
            for (uint32_t k = 2; k <= P; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t i = tid; i < P; i += MS_WG) {
                        const uint32_t x = i ^ j;
                        if (x > i) {
                            const bool up = (i & k) == 0;
                            if (ms_after(K, i, x) == up) {
                                const int64_t v = K.val[i], t = K.t[i];
                                const uint8_t f = K.fl[i];
                                K.val[i] = K.val[x]; K.t[i] = K.t[x]; K.fl[i] = K.fl[x];
                                K.val[x] = v; K.t[x] = t; K.fl[x] = f;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            // the keys are 0..m-1 now (padding behind them); an id's group
            // is from-keys then to-keys, classified by its head
            for (uint32_t i = tid; i < m; i += MS_WG) {
                const int64_t v = K.val[i];
                if (i > 0 && K.val[i - 1] == v) continue;
                const bool has1 = i + 1 < m && K.val[i + 1] == v;
                uint32_t cls;  // 0 pair, 1 open_from, 2 open_to, 3 repeated
                if (K.fl[i] & KF_TO) cls = has1 ? 3u : 2u;
                else if (!has1) cls = 1u;
                else if (!(K.fl[i + 1] & KF_TO)) cls = 3u;
                else cls = (i + 2 < m && K.val[i + 2] == v) ? 3u : 0u;
                atomicAdd(&s_cls[cls], 1u);
                if (cls == 0) {
                    const int64_t d = (int64_t)((uint64_t)K.t[i + 1] - (uint64_t)K.t[i]);
                    __hip_atomic_fetch_min(&s_min, (long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(&s_max, (long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    atomicAdd(&s_sum, (unsigned long long)d);
                    if (d < lo_us) {
                        atomicAdd(&s_uf, 1ull);
                    } else {
                        const uint64_t bin = ((uint64_t)d - (uint64_t)lo_us) / (uint64_t)bin_us;
                        if (bin >= n_bins) atomicAdd(&s_of, 1ull);
                        else atomicAdd(&s_hist[(uint32_t)bin], 1u);
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            tw_measure_out o{};
            o.pairs = s_cls[0]; o.open_from = s_cls[1]; o.open_to = s_cls[2]; o.repeated = s_cls[3];
            o.min_us = s_min; o.max_us = s_max; o.sum_us = (int64_t)s_sum;
            if (per) per[r] = o;
            wg.pairs += o.pairs; wg.open_from += o.open_from; wg.open_to += o.open_to; wg.repeated += o.repeated;
            wg.min_us = o.min_us < wg.min_us ? o.min_us : wg.min_us;
            wg.max_us = o.max_us > wg.max_us ? o.max_us : wg.max_us;
            wg.sum_us = (int64_t)((uint64_t)wg.sum_us + (uint64_t)o.sum_us);
        }
        // (thread 0 resets the accumulators only after reading them, and the
        // others touch them again only behind the next barrier)
    }
    __syncthreads();
    for (uint32_t b = tid; b < n_bins; b += MS_WG)
        if (s_hist[b]) atomicAdd(&hist[b], (unsigned long long)s_hist[b]);
    if (tid == 0) {
        auto add = [](uint64_t* p, uint64_t v) {
            if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
        };
        add(&total->pairs, wg.pairs); add(&total->open_from, wg.open_from); add(&total->open_to, wg.open_to);
        add(&total->repeated, wg.repeated); add(&total->truncated, wg.truncated);
        add(&total->underflow, s_uf); add(&total->overflow, s_of);
        add((uint64_t*)&total->sum_us, (uint64_t)wg.sum_us);
        if (wg.pairs) {
            __hip_atomic_fetch_min((long long*)&total->min_us, (long long)wg.min_us, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max((long long*)&total->max_us, (long long)wg.max_us, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// the call's device scratch and events, released on every return path
struct MsRes {
    void* buf = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~MsRes() {
        if (buf) (void)hipFree(buf);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

#define MSCHK(x)                                                                     \
    do {                                                                             \
        hipError_t _e = (x);                                                         \
        if (_e != hipSuccess) {                                                      \
            fprintf(stderr, "timewarp: %s failed: %s\n", #x, hipGetErrorString(_e)); \
            return _e == hipErrorOutOfMemory ? TW_ERR_OOM : TW_ERR_HIP;              \
        }                                                                            \
    } while (0)

}  // namespace

namespace tw {

int measure_run(int device, hipStream_t stream, const uint4* trace, const uint64_t* emitted, uint32_t R, uint32_t cap,
                const tw_measure_spec* spec, tw_measure_out* total, uint64_t* hist, tw_measure_out* per,
                double* kernel_ms) {
    if (!measure_spec_ok(spec) || !trace || !emitted || cap == 0) return TW_ERR_INVALID;
    if (R == 0) {
        if (total) measure_empty(total);
        if (hist) std::memset(hist, 0, (size_t)spec->n_bins * 8);
        if (kernel_ms) *kernel_ms = 0.0;
        return TW_OK;
    }
    // scratch: err word | total | hist[n_bins] | per[R] (when asked for) | cnt[R]
    const size_t o_total = 8, o_hist = o_total + sizeof(tw_measure_out);
    const size_t o_per = o_hist + (size_t)spec->n_bins * 8;
    const size_t o_cnt = o_per + (per ? (size_t)R * sizeof(tw_measure_out) : 0);
    const size_t bytes = o_cnt + (size_t)R * 4;
    MsRes res;
    MSCHK(hipSetDevice(device));
    MSCHK(hipMalloc(&res.buf, bytes));
    for (hipEvent_t& e : res.ev) MSCHK(hipEventCreate(&e));
    char* base = (char*)res.buf;
    uint32_t* d_err = (uint32_t*)base;
    tw_measure_out* d_total = (tw_measure_out*)(base + o_total);
    unsigned long long* d_hist = (unsigned long long*)(base + o_hist);
    tw_measure_out* d_per = per ? (tw_measure_out*)(base + o_per) : nullptr;
    uint32_t* d_cnt = (uint32_t*)(base + o_cnt);

    MSCHK(hipMemsetAsync(base, 0, o_per, stream));
    MSCHK(hipEventRecord(res.ev[0], stream));
    tw_measure_count<<<(R + MS_WG - 1) / MS_WG, MS_WG, 0, stream>>>(trace, emitted, R, cap, spec->tag_from,
                                                                   spec->tag_to, d_cnt, d_err, d_total);
    MSCHK(hipGetLastError());
    MSCHK(hipEventRecord(res.ev[1], stream));
    uint32_t h_err = 0;
    MSCHK(hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, stream));
    MSCHK(hipStreamSynchronize(stream));
    if (h_err) return TW_ERR_INVALID;  // some replica holds more keys than the join can sort

    // a workgroup's histogram counters are 32-bit: at most 2^20 replicas of
    // <= MS_KEYS / 2 pairs each per workgroup
    uint32_t grid = R < MS_GRID ? R : MS_GRID;
    const uint32_t need = (uint32_t)(((uint64_t)R + (1u << 20) - 1) >> 20);
    if (grid < need) grid = need;
    MSCHK(hipEventRecord(res.ev[2], stream));
    tw_measure_join<<<grid, MS_WG, 0, stream>>>(trace, emitted, R, spec->tag_from, spec->tag_to, spec->n_bins,
                                                spec->lo_us, spec->bin_us, d_cnt, d_total, d_hist, d_per);
    MSCHK(hipGetLastError());
    MSCHK(hipEventRecord(res.ev[3], stream));
    // host copies of the device results: the caller's buffers are written
    // only once everything has succeeded
    std::vector<char> h_head(o_per - o_total);
    std::vector<tw_measure_out> h_per(per ? R : 0);
    MSCHK(hipMemcpyAsync(h_head.data(), base + o_total, h_head.size(), hipMemcpyDeviceToHost, stream));
    if (per) MSCHK(hipMemcpyAsync(h_per.data(), d_per, (size_t)R * sizeof(tw_measure_out), hipMemcpyDeviceToHost, stream));
    MSCHK(hipStreamSynchronize(stream));
    float ms_a = 0.f, ms_b = 0.f;
    MSCHK(hipEventElapsedTime(&ms_a, res.ev[0], res.ev[1]));
    MSCHK(hipEventElapsedTime(&ms_b, res.ev[2], res.ev[3]));
    if (total) std::memcpy(total, h_head.data(), sizeof(tw_measure_out));
    if (hist) std::memcpy(hist, h_head.data() + sizeof(tw_measure_out), (size_t)spec->n_bins * 8);
    if (per) std::memcpy(per, h_per.data(), (size_t)R * sizeof(tw_measure_out));
    if (kernel_ms) *kernel_ms = (double)ms_a + (double)ms_b;
    return TW_OK;
}

}  // namespace tw
