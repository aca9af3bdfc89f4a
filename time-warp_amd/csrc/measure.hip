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
// Replicas with more than TW_MEASURE_MAX_KEYS matching records (accepted once
// tw_set_measure_keys raised the limit) take the partition path behind it: no
// sort, since a class needs only "once / more than once" per side and
// t_to - t_from.  Its kernels, stream-ordered:
//   tw_measure_plan        one lane per replica over cnt[R]: the large
//     replicas, their bucket counts (measure_part.hpp) and bucket bases,
//     claimed with atomics, the totals the host sizes the scratch from, and the
//     "over the limit" flag; large replicas get cnt[r] = MAX_KEYS + 1, which
//     tw_measure_join skips, leaving per[r] as the identity;
//   tw_measure_part<false> counts the keys per (replica, bucket, side);
//   tw_measure_ranges      every bucket claims its key range with one atomicAdd;
//   tw_measure_part<true>  scatters (val, t) into the ranges, tag_from keys
//     from a range's front and tag_to keys behind them: 16 B per key, the side
//     is the position.  Both part kernels give a workgroup a tile of T
//     neighbouring replicas x a chunk of n, T the largest power of two with
//     T x 2 x buckets <= 8192 LDS counters: a wave reads T x 32 contiguous
//     bytes per n of the [n][R][2] layout, and global atomics are one per
//     non-empty (replica, bucket, side) of the workgroup, not one per key;
//   tw_measure_join_large  a fixed grid, each workgroup a contiguous run of
//     buckets: per bucket an open-addressed LDS table of 2048 slots (val, acc,
//     state), insert by 64-bit compare-and-swap against the empty mark (the id
//     equal to the mark has a slot of its own), sticky once / more bits per
//     side, acc += side ? t : -t; a sweep classifies the slots into the
//     replica's accumulators (flushed with global atomics when the replica
//     changes: a replica's buckets may span workgroups) and the workgroup's
//     histogram.  More than 2048 distinct ids in one bucket raise a flag; the
//     call then returns TW_ERR_INVALID with nothing written.
// No lane waits for another, every probe loop ends after 2048 steps, every
// barrier is under a workgroup-uniform condition.
//
// tw_measure_quantiles (measure_select.hip) runs the same pass with the two
// join kernels' EMIT instantiations: a pair's latency is stored into a buffer
// segmented by replica (tw_measure_offsets: an exclusive scan of m_r / 2 over
// the replicas, behind the count and the plan) where tw_measure bins it.  The
// ME_BIN instantiations are what the kernels were before the template; ME_TIMES
// (tw_measure_series' LATENCY mode, measure_series.hip) stores t_from as well.
//
// LDS per workgroup: 2048 keys x (8 B val + 8 B t + 1 B flags) = 34 KiB, the
// histogram 4096 x 4 B = 16 KiB, a few accumulators: ~50.1 KiB static, under
// the 64 KiB a workgroup may hold; 3 workgroups per CU of the 160 KiB.
//
// A node-partitioned context (tw_lp_load; tw_set_trace refuses it) comes here
// through tw_lp_measure (abi.hip): its shards' records gathered into one
// buffer, one replica (R == 1) of E records, counted by tw_measure_count_one.
// Out of scope: a job-wide reduction over ranks, chunking the partition path's scratch over
// several passes.  (A traced LPB run keeps its due records on the lanes'
// chains, or, with tw_set_trace_batch, has tw_lp_batch<true> record them into
// the same buffer under the same counter: this pass reads either alike.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/timewarp.h"
#include "measure_combine.hpp"
#include "measure_part.hpp"
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

// R == 1 (tw_lp_measure: a node-partitioned context's one replica, of
// millions of records): the same count with a grid-stride walk over n, 32 B
// apart per lane, reduced per wave and per workgroup, one atomic per workgroup
// on cnt[0] (zeroed by the host).  The workgroup whose add carries the count
// over MS_KEYS sets the error word: exactly one does.
__global__ __launch_bounds__(MS_WG) void tw_measure_count_one(const uint4* __restrict__ trace,
                                                              const uint64_t* __restrict__ emitted, uint32_t cap,
                                                              uint32_t tag_from, uint32_t tag_to,
                                                              uint32_t* __restrict__ cnt, uint32_t* err,
                                                              tw_measure_out* total) {
    __shared__ uint32_t s_k[MS_WG / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        total->min_us = INT64_MAX;
        total->max_us = INT64_MIN;
    }
    const uint64_t em = emitted[0];  // (uniform: every return below is the whole grid's)
    if (em > cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) cnt[0] = MS_TRUNC;
        return;
    }
    const uint32_t kept = (uint32_t)em;
    uint32_t k = 0;
    for (uint64_t n = (uint64_t)blockIdx.x * MS_WG + threadIdx.x; n < kept; n += (uint64_t)gridDim.x * MS_WG) {
        const uint32_t tag = trace[(size_t)n * 2].w;
        k += (tag == tag_from || tag == tag_to) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) k += __shfl_down(k, o, 64);
    if ((threadIdx.x & 63u) == 0) s_k[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t w = 0;
        for (uint32_t i = 0; i < MS_WG / 64; ++i) w += s_k[i];
        if (w) {
            const uint32_t old = atomicAdd(&cnt[0], w);  // (<= kept < 2^32: no wrap)
            if (old <= MS_KEYS && old + w > MS_KEYS) atomicOr(err, 1u);
        }
    }
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

// EMIT (tw_measure_quantiles): instead of binning a pair's latency, store it at
// the replica's segment of qlat -- qoff[r] + its claim on the pairs counter,
// which the classes already take -- and leave the replica's pairs in qfill[r].
// A segment holds m / 2 latencies, and a pair is two of the m keys.
// EMIT is one of three states (tw_measure_series' LATENCY mode takes the third):
// ME_TIMES stores as ME_LAT does and also the pair's t_from, at the same place
// of the segment in a second buffer, qtf.
constexpr int ME_BIN = 0, ME_LAT = 1, ME_TIMES = 2;
template <int EMIT>
__global__ __launch_bounds__(MS_WG) void tw_measure_join(const uint4* __restrict__ trace,
                                                         const uint64_t* __restrict__ emitted, uint32_t R,
                                                         uint32_t tag_from, uint32_t tag_to, uint32_t n_bins,
                                                         int64_t lo_us, int64_t bin_us,
                                                         const uint32_t* __restrict__ cnt, tw_measure_out* total,
                                                         unsigned long long* hist, tw_measure_out* per,
                                                         const unsigned long long* __restrict__ qoff,
                                                         uint32_t* __restrict__ qfill, long long* __restrict__ qlat,
                                                         long long* __restrict__ qtf) {
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
                const uint32_t at = atomicAdd(&s_cls[cls], 1u);
                if (cls == 0) {
                    const int64_t d = (int64_t)((uint64_t)K.t[i + 1] - (uint64_t)K.t[i]);
                    __hip_atomic_fetch_min(&s_min, (long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_max(&s_max, (long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    atomicAdd(&s_sum, (unsigned long long)d);
                    if (EMIT) {
                        if (at < (m >> 1)) {
                            qlat[qoff[r] + at] = (long long)d;
                            if constexpr (EMIT == ME_TIMES) qtf[qoff[r] + at] = (long long)K.t[i];
                        }
                    } else if (d < lo_us) {
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
            if (EMIT) qfill[r] = s_cls[0];  // (a large replica: 0, tw_measure_join_large adds to it)
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

// ---------------------------------------------------------- partition path
using tw::MP_EMPTY;
using tw::MP_SLOTS;

constexpr uint32_t ML_NONE = 0xFFFFFFFFu;   // MsRep::log2b of a replica the partition path skips
constexpr uint32_t ML_CTRS = 8192;          // LDS counters of a part workgroup: [replica of the tile][bucket][side]
constexpr uint32_t ML_TILE_MAX = 64;        // replicas per tile at most: a wave's lanes
constexpr uint32_t ML_WG_RECORDS = 65536;   // records (tile x chunk) one part workgroup scans
constexpr uint32_t ML_GRID = 512;           // tw_measure_join_large: 256 CUs x 2 workgroups
constexpr uint32_t ML_OVER = 1, ML_TABLE = 2;  // MsPlan::flags
static_assert(ML_CTRS == 2u << tw::MP_MAX_LOG2B, "one replica's buckets x 2 sides fit the counters at T = 1");
static_assert(MP_SLOTS * 20 + 20 + MS_BINS * 4 + 256 <= 64 * 1024, "static LDS of tw_measure_join_large");

struct MsRep {       // what the partition path knows of replica r
    uint32_t kept;   // records to scan
    uint32_t log2b;  // log2 of its bucket count, ML_NONE: not large (or truncated)
    uint32_t bbase;  // its first bucket among all
    uint32_t m;      // its matching records
    unsigned long long kbase;  // its first key among all
};
struct MsPlan {  // read by the host after tw_measure_plan (ML_TABLE: after the join)
    uint32_t flags, n_large, max_log2b, max_kept;
    unsigned long long n_buckets, n_keys;
};

__global__ __launch_bounds__(MS_WG) void tw_measure_plan(const uint64_t* __restrict__ emitted, uint32_t R,
                                                         uint32_t lds_keys, uint32_t max_keys, uint32_t bucket_keys,
                                                         uint32_t* __restrict__ cnt, MsRep* __restrict__ rep,
                                                         uint32_t* __restrict__ large, MsPlan* plan) {
    const uint32_t r = blockIdx.x * MS_WG + threadIdx.x;
    if (r >= R) return;
    const uint32_t m = cnt[r];
    MsRep o{0, ML_NONE, 0, 0, 0};
    if (m != MS_TRUNC && m > lds_keys) {
        if (m > max_keys) {
            atomicOr(&plan->flags, ML_OVER);
        } else {
            o.kept = (uint32_t)emitted[r];  // (not truncated: emitted <= cap)
            o.log2b = tw::mp_log2_buckets(m, bucket_keys);
            o.bbase = (uint32_t)atomicAdd(&plan->n_buckets, 1ull << o.log2b);
            o.m = m;
            o.kbase = atomicAdd(&plan->n_keys, (unsigned long long)m);
            atomicMax(&plan->max_log2b, o.log2b);
            atomicMax(&plan->max_kept, o.kept);
            large[atomicAdd(&plan->n_large, 1u)] = r;
            cnt[r] = MS_KEYS + 1;  // tw_measure_join: skip, per[r] = the identity
        }
    }
    rep[r] = o;
}

// A workgroup scans replicas r0 .. r0 + T - 1 (T = 1 << tlog2) over n0 ..
// n0 + chunk - 1: lane (n, r) -> tid = n * T + (r - r0).  blog2 is the batch's
// largest log2b: counter [(r - r0) << blog2 | bucket][side].
template <bool SCATTER>
__global__ __launch_bounds__(MS_WG) void tw_measure_part(const uint4* __restrict__ trace, uint32_t R, uint32_t tag_from,
                                                         uint32_t tag_to, const MsRep* __restrict__ rep,
                                                         uint32_t tlog2, uint32_t blog2, uint32_t chunk,
                                                         uint32_t tiles, unsigned long long n_buckets,
                                                         unsigned long long n_keys, uint32_t* __restrict__ bcnt,
                                                         uint32_t* __restrict__ fill, uint4* __restrict__ keys) {
    __shared__ uint32_t s_c[ML_CTRS];  // counts; in the scatter then each counter's claimed offset, the local cursor
    const uint32_t tid = threadIdx.x;
    const uint32_t T = 1u << tlog2, used = 2u << (tlog2 + blog2);  // <= ML_CTRS (the host chose tlog2 so)
    const uint32_t r0 = (blockIdx.x % tiles) << tlog2, n0 = (blockIdx.x / tiles) * chunk;
    const uint32_t dr = tid & (T - 1), r = r0 + dr;
    MsRep me{0, ML_NONE, 0, 0, 0};
    if (r < R) me = rep[r];
    const bool mine = me.log2b != ML_NONE;
    const uint32_t n_end = mine ? (me.kept < n0 + chunk ? me.kept : n0 + chunk) : 0u;
    const uint32_t n_step = MS_WG >> tlog2;

    for (uint32_t i = tid; i < used; i += MS_WG) s_c[i] = 0;
    __syncthreads();
    for (uint32_t n = n0 + (tid >> tlog2); n < n_end; n += n_step) {
        const uint4* q = trace + ((size_t)n * R + r) * 2;
        const uint4 a = q[0];
        if (a.w == tag_from || a.w == tag_to) {
            const uint4 b = q[1];
            const uint32_t bk = tw::mp_bucket_of((int64_t)(((uint64_t)b.y << 32) | b.x), me.log2b);
            atomicAdd(&s_c[(((dr << blog2) | bk) << 1) | (a.w == tag_to ? 1u : 0u)], 1u);
        }
    }
    __syncthreads();
    // one global atomic per non-empty counter (a non-empty counter belongs to
    // a large replica and to one of its buckets)
    for (uint32_t i = tid; i < used; i += MS_WG) {
        const uint32_t c = s_c[i];
        if (!c) continue;
        const MsRep o = rep[r0 + (i >> (blog2 + 1))];
        const unsigned long long gb = (unsigned long long)o.bbase + ((i >> 1) & ((1u << blog2) - 1));
        if (gb >= n_buckets) continue;
        if (!SCATTER) {
            atomicAdd(&bcnt[2 * gb + (i & 1)], c);
        } else {
            s_c[i] = atomicAdd(&fill[2 * gb + (i & 1)], c);
        }
    }
    if (!SCATTER) return;
    __syncthreads();
    for (uint32_t n = n0 + (tid >> tlog2); n < n_end; n += n_step) {
        const uint4* q = trace + ((size_t)n * R + r) * 2;
        const uint4 a = q[0];
        if (a.w == tag_from || a.w == tag_to) {
            const uint4 b = q[1];
            const uint32_t bk = tw::mp_bucket_of((int64_t)(((uint64_t)b.y << 32) | b.x), me.log2b);
            const uint32_t i = (((dr << blog2) | bk) << 1) | (a.w == tag_to ? 1u : 0u);
            const uint32_t off = atomicAdd(&s_c[i], 1u);  // within the replica's keys
            const unsigned long long at = me.kbase + off;
            if (off < me.m && at < n_keys) keys[at] = make_uint4(b.x, b.y, a.x, a.y);  // (val, t)
        }
    }
}

// one workgroup per large replica: each of its buckets claims its key range
// within the replica's (offsets from MsRep::kbase)
__global__ __launch_bounds__(MS_WG) void tw_measure_ranges(const uint32_t* __restrict__ large,
                                                           const MsRep* __restrict__ rep,
                                                           const uint32_t* __restrict__ bcnt,
                                                           unsigned long long n_buckets,
                                                           uint32_t* __restrict__ bstart, uint32_t* __restrict__ brep,
                                                           uint32_t* __restrict__ fill) {
    __shared__ uint32_t s_cur;
    const uint32_t r = large[blockIdx.x];
    const MsRep o = rep[r];
    if (threadIdx.x == 0) s_cur = 0;
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < (1u << o.log2b); b += MS_WG) {
        const unsigned long long gb = (unsigned long long)o.bbase + b;
        if (gb >= n_buckets) continue;
        const uint32_t cf = bcnt[2 * gb], ct = bcnt[2 * gb + 1];
        const uint32_t at = atomicAdd(&s_cur, cf + ct);  // (the counts of a replica sum to its m)
        bstart[gb] = at;
        brep[gb] = r;
        fill[2 * gb] = at;
        fill[2 * gb + 1] = at + cf;
    }
}

// slot state: a side's "seen" bit, and its "seen again" bit
constexpr uint32_t SF_FROM = 1, SF_FROM2 = 2, SF_TO = 4, SF_TO2 = 8;

// EMIT: as tw_measure_join's.  A replica's buckets span workgroups, so its
// fill count in qfill[r] is the cursor: a wave counts its lanes' pairs of the
// bucket, its last lane claims that many places with one atomic, and the lanes
// store behind the claim in a second walk over their slots.  ME_TIMES: a slot
// also keeps the t of its tag_from key (one key writes it when the id is a
// pair), in the LDS the histogram leaves free: that state bins nothing.
template <int EMIT>
__global__ __launch_bounds__(MS_WG) void tw_measure_join_large(const uint4* __restrict__ keys,
                                                               const uint32_t* __restrict__ bcnt,
                                                               const uint32_t* __restrict__ bstart,
                                                               const uint32_t* __restrict__ brep,
                                                               const MsRep* __restrict__ rep,
                                                               uint32_t n_buckets, uint32_t per_wg,
                                                               unsigned long long n_keys, uint32_t n_bins,
                                                               int64_t lo_us, int64_t bin_us, MsPlan* plan,
                                                               tw_measure_out* total, unsigned long long* hist,
                                                               tw_measure_out* per,
                                                               const unsigned long long* __restrict__ qoff,
                                                               uint32_t* __restrict__ qfill,
                                                               long long* __restrict__ qlat,
                                                               long long* __restrict__ qtf) {
    // slot MP_SLOTS is the id MP_EMPTY's own
    __shared__ unsigned long long s_val[MP_SLOTS + 1];
    __shared__ unsigned long long s_acc[MP_SLOTS + 1];
    __shared__ uint32_t s_st[MP_SLOTS + 1];
    __shared__ uint32_t s_hist[EMIT == ME_TIMES ? 2 : MS_BINS];  // (ME_TIMES: the host passes n_bins = 1)
    __shared__ unsigned long long s_tf[EMIT == ME_TIMES ? MP_SLOTS + 1 : 1];
    __shared__ uint32_t s_cls[4];  // the current replica's pairs, open_from, open_to, repeated (of this workgroup's buckets)
    __shared__ long long s_min, s_max;
    __shared__ unsigned long long s_sum;
    __shared__ unsigned long long s_uf, s_of;
    __shared__ uint32_t s_full;
    const uint32_t tid = threadIdx.x;

    for (uint32_t b = tid; b < n_bins; b += MS_WG) s_hist[b] = 0;
    if (tid == 0) {
        s_uf = s_of = 0;
        s_full = 0;
        s_cls[0] = s_cls[1] = s_cls[2] = s_cls[3] = 0;
        s_min = INT64_MAX;
        s_max = INT64_MIN;
        s_sum = 0;
    }
    tw_measure_out wg;  // the workgroup's totals (thread 0)
    wg.pairs = wg.open_from = wg.open_to = wg.repeated = 0;
    wg.min_us = INT64_MAX;
    wg.max_us = INT64_MIN;
    wg.sum_us = 0;
    // thread 0: the replica's accumulators into per[r] (other workgroups may
    // hold more of its buckets: atomics onto the identity tw_measure_join
    // wrote) and into the workgroup's totals; then reset
    auto flush = [&](uint32_t r) {
        const uint64_t np = s_cls[0];
        if (per) {
            tw_measure_out* o = per + r;
            if (np) atomicAdd((unsigned long long*)&o->pairs, (unsigned long long)np);
            if (s_cls[1]) atomicAdd((unsigned long long*)&o->open_from, (unsigned long long)s_cls[1]);
            if (s_cls[2]) atomicAdd((unsigned long long*)&o->open_to, (unsigned long long)s_cls[2]);
            if (s_cls[3]) atomicAdd((unsigned long long*)&o->repeated, (unsigned long long)s_cls[3]);
            if (np) {
                atomicAdd((unsigned long long*)&o->sum_us, s_sum);
                __hip_atomic_fetch_min((long long*)&o->min_us, s_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max((long long*)&o->max_us, s_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        wg.pairs += np; wg.open_from += s_cls[1]; wg.open_to += s_cls[2]; wg.repeated += s_cls[3];
        wg.min_us = s_min < wg.min_us ? s_min : wg.min_us;
        wg.max_us = s_max > wg.max_us ? s_max : wg.max_us;
        wg.sum_us = (int64_t)((uint64_t)wg.sum_us + s_sum);
        s_cls[0] = s_cls[1] = s_cls[2] = s_cls[3] = 0;
        s_min = INT64_MAX;
        s_max = INT64_MIN;
        s_sum = 0;
    };

    // gb, the bucket's counts and its replica depend on the workgroup alone:
    // every branch that holds a barrier below is taken by all of it or none
    const uint32_t g0 = blockIdx.x * per_wg < n_buckets ? blockIdx.x * per_wg : n_buckets;
    const uint32_t g1 = n_buckets - g0 < per_wg ? n_buckets : g0 + per_wg;
    uint32_t cur = ML_NONE;
    for (uint32_t gb = g0; gb < g1; ++gb) {
        const uint32_t cf = bcnt[2 * gb], ct = bcnt[2 * gb + 1], m = cf + ct;
        if (m == 0) continue;
        const uint32_t r = brep[gb];
        const unsigned long long at = rep[r].kbase + bstart[gb];
        if (at + m > n_keys) continue;
        if (r != cur) {
            // (the sweep's closing barrier is behind us: the accumulators are final)
            if (tid == 0 && cur != ML_NONE) flush(cur);
            cur = r;
        }
        for (uint32_t s = tid; s <= MP_SLOTS; s += MS_WG) {
            s_val[s] = (unsigned long long)MP_EMPTY;
            s_acc[s] = 0;
            s_st[s] = 0;
        }
        __syncthreads();
        for (uint32_t i = tid; i < m; i += MS_WG) {
            const uint4 k = keys[at + i];
            const unsigned long long v = ((unsigned long long)k.y << 32) | k.x;
            const unsigned long long t = ((unsigned long long)k.w << 32) | k.z;
            const bool to = i >= cf;
            uint32_t s = MP_SLOTS;
            if (v != (unsigned long long)MP_EMPTY) {
                s = tw::mp_slot_of((int64_t)v);
                uint32_t probes = 0;
                for (; probes < MP_SLOTS; ++probes) {
                    const unsigned long long old = atomicCAS(&s_val[s], (unsigned long long)MP_EMPTY, v);
                    if (old == (unsigned long long)MP_EMPTY || old == v) break;
                    s = (s + 1) & (MP_SLOTS - 1);
                }
                if (probes == MP_SLOTS) {  // more than MP_SLOTS distinct ids in this bucket
                    s_full = 1;
                    continue;
                }
            }
            const uint32_t once = to ? SF_TO : SF_FROM;
            if (atomicOr(&s_st[s], once) & once) atomicOr(&s_st[s], once << 1);
            atomicAdd(&s_acc[s], to ? t : 0ull - t);
            if constexpr (EMIT == ME_TIMES)
                if (!to) s_tf[s] = t;  // (a pair has one tag_from key: no other lane writes this slot)
        }
        __syncthreads();
        uint32_t mine = 0;  // EMIT: this lane's pairs of the bucket
        for (uint32_t s = tid; s <= MP_SLOTS; s += MS_WG) {
            const uint32_t st = s_st[s];
            if (!st) continue;
            uint32_t cls;  // 0 pair, 1 open_from, 2 open_to, 3 repeated
            if (st & (SF_FROM2 | SF_TO2)) cls = 3u;
            else if (st == (SF_FROM | SF_TO)) cls = 0u;
            else cls = st == SF_FROM ? 1u : 2u;
            atomicAdd(&s_cls[cls], 1u);
            if (cls == 0) {
                const int64_t d = (int64_t)s_acc[s];
                __hip_atomic_fetch_min(&s_min, (long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_max(&s_max, (long long)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                atomicAdd(&s_sum, (unsigned long long)d);
                if (EMIT) {
                    ++mine;
                } else if (d < lo_us) {
                    atomicAdd(&s_uf, 1ull);
                } else {
                    const uint64_t bin = ((uint64_t)d - (uint64_t)lo_us) / (uint64_t)bin_us;
                    if (bin >= n_bins) atomicAdd(&s_of, 1ull);
                    else atomicAdd(&s_hist[(uint32_t)bin], 1u);
                }
            }
        }
        if (EMIT) {
            // (every lane of the wave is here: the loop above has ended for all
            // of them; nothing below waits, the shuffles read registers)
            const uint32_t lane = tid & 63u;
            uint32_t upto = mine;  // inclusive scan over the wave
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(upto, o, 64);
                if (lane >= o) upto += v;
            }
            const uint32_t wave_n = __shfl(upto, 63, 64);
            if (wave_n) {  // (uniform over the wave)
                uint32_t base = 0;
                if (lane == 63) base = atomicAdd(&qfill[r], wave_n);
                base = __shfl(base, 63, 64);
                uint32_t at = base + upto - mine;
                const uint32_t room = rep[r].m >> 1;
                const unsigned long long seg = qoff[r];
                for (uint32_t s = tid; s <= MP_SLOTS; s += MS_WG) {
                    if (s_st[s] != (SF_FROM | SF_TO)) continue;
                    if (at < room) {
                        qlat[seg + at] = (long long)s_acc[s];
                        if constexpr (EMIT == ME_TIMES) qtf[seg + at] = (long long)s_tf[s];
                    }
                    ++at;
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (uint32_t b = tid; b < n_bins; b += MS_WG)
        if (s_hist[b]) atomicAdd(&hist[b], (unsigned long long)s_hist[b]);
    if (tid == 0) {
        if (cur != ML_NONE) flush(cur);
        if (s_full) atomicOr(&plan->flags, ML_TABLE);
        auto add = [](uint64_t* p, uint64_t v) {
            if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
        };
        add(&total->pairs, wg.pairs); add(&total->open_from, wg.open_from); add(&total->open_to, wg.open_to);
        add(&total->repeated, wg.repeated);
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

// EMIT: the replicas' segments of the latency buffer.  Replica r gets m_r / 2
// places (m_r its matching records: cnt[r], or MsRep::m once the plan marked it
// large; none when truncated), off[r] the exclusive sum, off[R] the total.  One
// workgroup: lane i sums a contiguous run of replicas, the 256 sums are scanned
// in LDS, and the lane walks its run again.
__global__ __launch_bounds__(MS_WG) void tw_measure_offsets(const uint32_t* __restrict__ cnt,
                                                            const MsRep* __restrict__ rep, uint32_t R,
                                                            unsigned long long* __restrict__ off) {
    __shared__ unsigned long long s_sum[MS_WG];
    const uint32_t tid = threadIdx.x;
    const uint32_t run = (R + MS_WG - 1) / MS_WG;
    const uint32_t r0 = (uint64_t)tid * run < R ? tid * run : R, r1 = R - r0 < run ? R : r0 + run;
    auto places = [&](uint32_t r) -> unsigned long long {
        uint32_t m = cnt[r];
        if (m == MS_TRUNC) return 0;
        if (m > MS_KEYS) m = rep ? rep[r].m : 0u;
        return m >> 1;
    };
    unsigned long long sum = 0;
    for (uint32_t r = r0; r < r1; ++r) sum += places(r);
    s_sum[tid] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < MS_WG; o <<= 1) {
        const unsigned long long v = tid >= o ? s_sum[tid - o] : 0ull;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    unsigned long long at = s_sum[tid] - sum;
    for (uint32_t r = r0; r < r1; ++r) {
        off[r] = at;
        at += places(r);
    }
    if (tid == MS_WG - 1) off[R] = s_sum[tid];
}

// the call's device scratch and events, released on every return path
struct MsRes {
    void* buf = nullptr;
    void* plan = nullptr;  // partition path: header, per-replica entries, the large list
    void* part = nullptr;  // partition path: per-bucket arrays and the keys
    hipEvent_t ev[13] = {};  // 0-3: the LDS path's; 4-10: made when the partition path runs; 11-12: emit's
    ~MsRes() {
        if (buf) (void)hipFree(buf);
        if (plan) (void)hipFree(plan);
        if (part) (void)hipFree(part);
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
                const tw_measure_spec* spec, const MeasureCfg& cfg, tw_measure_out* total, uint64_t* hist,
                tw_measure_out* per, double* kernel_ms, double* phase_ms, MeasureEmit* emit) {
    if (!measure_spec_ok(spec) || !trace || !emitted || cap == 0) return TW_ERR_INVALID;
    if (cfg.lds_keys > MS_KEYS || cfg.max_keys < MS_KEYS || cfg.max_keys > MP_MAX_KEYS || cfg.bucket_keys == 0)
        return TW_ERR_INVALID;
    if (phase_ms) std::fill(phase_ms, phase_ms + MEASURE_PHASES, 0.0);
    if (R == 0) {
        if (total) measure_empty(total);
        if (hist) std::memset(hist, 0, (size_t)spec->n_bins * 8);
        if (kernel_ms) *kernel_ms = 0.0;
        if (emit) *emit = MeasureEmit{};
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
    for (int i = 0; i < 4; ++i) MSCHK(hipEventCreate(&res.ev[i]));
    char* base = (char*)res.buf;
    uint32_t* d_err = (uint32_t*)base;
    tw_measure_out* d_total = (tw_measure_out*)(base + o_total);
    unsigned long long* d_hist = (unsigned long long*)(base + o_hist);
    tw_measure_out* d_per = per ? (tw_measure_out*)(base + o_per) : nullptr;
    uint32_t* d_cnt = (uint32_t*)(base + o_cnt);

    MSCHK(hipMemsetAsync(base, 0, o_per, stream));
    if (R == 1) MSCHK(hipMemsetAsync(d_cnt, 0, 4, stream));
    MSCHK(hipEventRecord(res.ev[0], stream));
    if (R == 1) {
        // one replica: parallel over its records (at most cap of them are read)
        const uint32_t cgrid = (uint32_t)std::min<uint64_t>(((uint64_t)cap + MS_WG - 1) / MS_WG, 4 * MS_GRID);
        tw_measure_count_one<<<cgrid, MS_WG, 0, stream>>>(trace, emitted, cap, spec->tag_from, spec->tag_to, d_cnt,
                                                          d_err, d_total);
    } else {
        tw_measure_count<<<(R + MS_WG - 1) / MS_WG, MS_WG, 0, stream>>>(trace, emitted, R, cap, spec->tag_from,
                                                                       spec->tag_to, d_cnt, d_err, d_total);
    }
    MSCHK(hipGetLastError());
    MSCHK(hipEventRecord(res.ev[1], stream));
    uint32_t h_err = 0;
    MSCHK(hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, stream));
    MSCHK(hipStreamSynchronize(stream));
    // some replica holds more keys than the LDS join sorts: the partition
    // path's business when the limit was raised (under the testing hook the
    // plan decides, whatever the error word says)
    const bool plan_needed = h_err ? cfg.max_keys > MS_KEYS : cfg.lds_keys < MS_KEYS;
    if (h_err && !plan_needed) return TW_ERR_INVALID;
    MsPlan plan{};
    MsRep* d_rep = nullptr;
    uint32_t *d_large = nullptr, *d_bcnt = nullptr, *d_bstart = nullptr, *d_brep = nullptr;
    uint4* d_keys = nullptr;
    if (plan_needed) {
        // plan scratch: header (64 B) | rep[R] | large[R]
        const size_t o_rep = 64, o_large = o_rep + (size_t)R * sizeof(MsRep);
        static_assert(sizeof(MsPlan) <= 64 && sizeof(MsRep) == 24, "the scratch formula of measure_part.hpp");
        if (hipMalloc(&res.plan, o_large + (size_t)R * 4) != hipSuccess) {
            (void)hipGetLastError();  // (not sticky: the context stays usable)
            return TW_ERR_OOM;
        }
        for (int i = 4; i < 11; ++i) MSCHK(hipEventCreate(&res.ev[i]));
        MsPlan* d_plan = (MsPlan*)res.plan;
        d_rep = (MsRep*)((char*)res.plan + o_rep);
        d_large = (uint32_t*)((char*)res.plan + o_large);
        MSCHK(hipMemsetAsync(d_plan, 0, 64, stream));
        MSCHK(hipEventRecord(res.ev[4], stream));
        tw_measure_plan<<<(R + MS_WG - 1) / MS_WG, MS_WG, 0, stream>>>(emitted, R, cfg.lds_keys, cfg.max_keys,
                                                                      cfg.bucket_keys, d_cnt, d_rep, d_large, d_plan);
        MSCHK(hipGetLastError());
        MSCHK(hipEventRecord(res.ev[5], stream));
        MSCHK(hipMemcpyAsync(&plan, d_plan, sizeof plan, hipMemcpyDeviceToHost, stream));
        MSCHK(hipStreamSynchronize(stream));
        // over the limit: decided before the key scratch exists.  Everything
        // below is bounded by these words: n_large <= R, max_log2b <=
        // MP_MAX_LOG2B, n_keys <= R * max_keys, bucket indices in 32 bits
        if (plan.flags & ML_OVER) return TW_ERR_INVALID;
        if (plan.n_large > R || plan.max_log2b > MP_MAX_LOG2B || plan.max_kept > cap ||
            plan.n_buckets > 0x7FFFFFFFull || plan.n_keys > (unsigned long long)R * cfg.max_keys)
            return TW_ERR_STATE;
    }
    if (emit) {
        // the latency segments: off[R + 1] | fill[R], then the buffer itself
        // once the device has summed the places.  The caller owns both from
        // here on, whatever this call returns (measure_emit_free)
        const bool with_t = emit->with_t;
        *emit = MeasureEmit{};
        emit->with_t = with_t;
        constexpr size_t digits = (size_t)2 * TW_MEASURE_MAX_QUANTILES * 256;  // (select_count's histogram)
        if (hipMalloc(&emit->buf, ((size_t)R + 1 + digits) * 8 + (size_t)R * 4) != hipSuccess) {
            (void)hipGetLastError();
            return TW_ERR_OOM;
        }
        emit->off = (unsigned long long*)emit->buf;
        emit->digits = emit->off + R + 1;
        emit->fill = (uint32_t*)(emit->digits + digits);
        for (int i = 11; i < 13; ++i) MSCHK(hipEventCreate(&res.ev[i]));
        MSCHK(hipMemsetAsync(emit->fill, 0, (size_t)R * 4, stream));
        MSCHK(hipEventRecord(res.ev[11], stream));
        tw_measure_offsets<<<1, MS_WG, 0, stream>>>(d_cnt, d_rep, R, emit->off);
        MSCHK(hipGetLastError());
        MSCHK(hipEventRecord(res.ev[12], stream));
        unsigned long long places = 0;
        MSCHK(hipMemcpyAsync(&places, emit->off + R, 8, hipMemcpyDeviceToHost, stream));
        MSCHK(hipStreamSynchronize(stream));
        // (a place per two matching records, and a matching record is a kept one)
        if (places > (unsigned long long)R * cap / 2) return TW_ERR_STATE;
        emit->places = places;
        // (with_t: the t_from buffer behind the latencies, place for place)
        if (hipMalloc((void**)&emit->lat, (size_t)(places ? places : 1) * (with_t ? 16 : 8)) != hipSuccess) {
            (void)hipGetLastError();
            return TW_ERR_OOM;
        }
        if (with_t) emit->tfrom = emit->lat + (places ? places : 1);
    }
    if (plan.n_large) {
        // part scratch: bcnt[2 B] | fill[2 B] | bstart[B] | brep[B] | keys[K] (16 B each, 16-aligned)
        const size_t B = (size_t)plan.n_buckets, K = (size_t)plan.n_keys;
        const size_t o_fill = B * 8, o_bstart = o_fill + B * 8, o_brep = o_bstart + B * 4;
        const size_t o_keys = (o_brep + B * 4 + 15) & ~(size_t)15;
        if (hipMalloc(&res.part, o_keys + K * 16) != hipSuccess) {
            (void)hipGetLastError();
            return TW_ERR_OOM;
        }
        char* pb = (char*)res.part;
        d_bcnt = (uint32_t*)pb;
        uint32_t* d_fill = (uint32_t*)(pb + o_fill);
        d_bstart = (uint32_t*)(pb + o_bstart);
        d_brep = (uint32_t*)(pb + o_brep);
        d_keys = (uint4*)(pb + o_keys);
        // a tile of T replicas x their buckets x 2 sides within the LDS
        // counters; a workgroup scans about ML_WG_RECORDS records
        uint32_t tlog2 = MP_MAX_LOG2B - plan.max_log2b;
        if (tlog2 > 6) tlog2 = 6;  // ML_TILE_MAX
        while (tlog2 > 0 && (1u << (tlog2 - 1)) >= R) --tlog2;
        static_assert(ML_TILE_MAX == 64 && (2u << MP_MAX_LOG2B) == ML_CTRS, "tile size against the counters");
        const uint32_t tiles = (uint32_t)(((uint64_t)R + (1u << tlog2) - 1) >> tlog2);
        uint32_t chunk = ML_WG_RECORDS >> tlog2;
        uint64_t chunks = ((uint64_t)plan.max_kept + chunk - 1) / chunk;
        while ((uint64_t)tiles * chunks > 0x7FFFFFFFull) {  // (the grid's limit; never at sizes memory holds)
            chunk *= 2;
            chunks = ((uint64_t)plan.max_kept + chunk - 1) / chunk;
        }
        const uint32_t pgrid = (uint32_t)((uint64_t)tiles * (chunks ? chunks : 1));
        MSCHK(hipEventRecord(res.ev[6], stream));
        MSCHK(hipMemsetAsync(d_bcnt, 0, B * 8, stream));
        tw_measure_part<false><<<pgrid, MS_WG, 0, stream>>>(trace, R, spec->tag_from, spec->tag_to, d_rep, tlog2,
                                                            plan.max_log2b, chunk, tiles, plan.n_buckets, plan.n_keys,
                                                            d_bcnt, d_fill, d_keys);
        MSCHK(hipGetLastError());
        MSCHK(hipEventRecord(res.ev[7], stream));
        tw_measure_ranges<<<plan.n_large, MS_WG, 0, stream>>>(d_large, d_rep, d_bcnt, plan.n_buckets, d_bstart, d_brep,
                                                              d_fill);
        MSCHK(hipGetLastError());
        MSCHK(hipEventRecord(res.ev[8], stream));
        tw_measure_part<true><<<pgrid, MS_WG, 0, stream>>>(trace, R, spec->tag_from, spec->tag_to, d_rep, tlog2,
                                                           plan.max_log2b, chunk, tiles, plan.n_buckets, plan.n_keys,
                                                           d_bcnt, d_fill, d_keys);
        MSCHK(hipGetLastError());
        MSCHK(hipEventRecord(res.ev[9], stream));
    }

    // a workgroup's histogram counters are 32-bit: at most 2^20 replicas of
    // <= MS_KEYS / 2 pairs each per workgroup
    uint32_t grid = R < MS_GRID ? R : MS_GRID;
    const uint32_t need = (uint32_t)(((uint64_t)R + (1u << 20) - 1) >> 20);
    if (grid < need) grid = need;
    MSCHK(hipEventRecord(res.ev[2], stream));
    if (emit && emit->with_t)
        tw_measure_join<ME_TIMES><<<grid, MS_WG, 0, stream>>>(trace, emitted, R, spec->tag_from, spec->tag_to,
                                                              spec->n_bins, spec->lo_us, spec->bin_us, d_cnt, d_total,
                                                              d_hist, d_per, emit->off, emit->fill, emit->lat,
                                                              emit->tfrom);
    else if (emit)
        tw_measure_join<ME_LAT><<<grid, MS_WG, 0, stream>>>(trace, emitted, R, spec->tag_from, spec->tag_to,
                                                            spec->n_bins, spec->lo_us, spec->bin_us, d_cnt, d_total,
                                                            d_hist, d_per, emit->off, emit->fill, emit->lat, nullptr);
    else
        tw_measure_join<ME_BIN><<<grid, MS_WG, 0, stream>>>(trace, emitted, R, spec->tag_from, spec->tag_to,
                                                            spec->n_bins, spec->lo_us, spec->bin_us, d_cnt, d_total,
                                                            d_hist, d_per, nullptr, nullptr, nullptr, nullptr);
    MSCHK(hipGetLastError());
    MSCHK(hipEventRecord(res.ev[3], stream));
    if (plan.n_large) {
        // behind tw_measure_join, which wrote the large replicas' per[r] as the
        // identity.  32-bit histogram counters: at most 2^20 buckets of <=
        // MP_SLOTS + 1 pairs each per workgroup
        const uint32_t B = (uint32_t)plan.n_buckets;
        uint32_t lgrid = B < ML_GRID ? B : ML_GRID;
        const uint32_t lneed = (uint32_t)(((uint64_t)B + (1u << 20) - 1) >> 20);
        if (lgrid < lneed) lgrid = lneed;
        const uint32_t per_wg = (B + lgrid - 1) / lgrid;
        if (emit && emit->with_t)
            tw_measure_join_large<ME_TIMES><<<lgrid, MS_WG, 0, stream>>>(
                d_keys, d_bcnt, d_bstart, d_brep, d_rep, B, per_wg, plan.n_keys, 1u, spec->lo_us, spec->bin_us,
                (MsPlan*)res.plan, d_total, d_hist, d_per, emit->off, emit->fill, emit->lat, emit->tfrom);
        else if (emit)
            tw_measure_join_large<ME_LAT><<<lgrid, MS_WG, 0, stream>>>(
                d_keys, d_bcnt, d_bstart, d_brep, d_rep, B, per_wg, plan.n_keys, spec->n_bins, spec->lo_us,
                spec->bin_us, (MsPlan*)res.plan, d_total, d_hist, d_per, emit->off, emit->fill, emit->lat, nullptr);
        else
            tw_measure_join_large<ME_BIN><<<lgrid, MS_WG, 0, stream>>>(
                d_keys, d_bcnt, d_bstart, d_brep, d_rep, B, per_wg, plan.n_keys, spec->n_bins, spec->lo_us,
                spec->bin_us, (MsPlan*)res.plan, d_total, d_hist, d_per, nullptr, nullptr, nullptr, nullptr);
        MSCHK(hipGetLastError());
        MSCHK(hipEventRecord(res.ev[10], stream));
        MSCHK(hipMemcpyAsync(&plan.flags, res.plan, 4, hipMemcpyDeviceToHost, stream));
    }
    // host copies of the device results: the caller's buffers are written
    // only once everything has succeeded
    std::vector<char> h_head(o_per - o_total);
    std::vector<tw_measure_out> h_per(per ? R : 0);
    MSCHK(hipMemcpyAsync(h_head.data(), base + o_total, h_head.size(), hipMemcpyDeviceToHost, stream));
    if (per) MSCHK(hipMemcpyAsync(h_per.data(), d_per, (size_t)R * sizeof(tw_measure_out), hipMemcpyDeviceToHost, stream));
    MSCHK(hipStreamSynchronize(stream));
    if (plan.flags & ML_TABLE) return TW_ERR_INVALID;  // a bucket held more distinct ids than its table
    float ms_a = 0.f, ms_b = 0.f;
    MSCHK(hipEventElapsedTime(&ms_a, res.ev[0], res.ev[1]));
    MSCHK(hipEventElapsedTime(&ms_b, res.ev[2], res.ev[3]));
    // count, plan, part<false>, ranges, part<true>, join, join_large
    double ph[MEASURE_PHASES] = {ms_a, 0, 0, 0, 0, ms_b, 0};
    if (plan_needed) {
        static const int span[MEASURE_PHASES][2] = {{0, 1}, {4, 5}, {6, 7}, {7, 8}, {8, 9}, {2, 3}, {3, 10}};
        for (int i = 1; i < MEASURE_PHASES; ++i) {
            if (i == 5 || (i > 1 && !plan.n_large)) continue;
            float ms = 0.f;
            MSCHK(hipEventElapsedTime(&ms, res.ev[span[i][0]], res.ev[span[i][1]]));
            ph[i] = ms;
        }
    }
    if (total) std::memcpy(total, h_head.data(), sizeof(tw_measure_out));
    if (hist) std::memcpy(hist, h_head.data() + sizeof(tw_measure_out), (size_t)spec->n_bins * 8);
    if (per) std::memcpy(per, h_per.data(), (size_t)R * sizeof(tw_measure_out));
    if (kernel_ms) {
        *kernel_ms = 0.0;
        for (double v : ph) *kernel_ms += v;
    }
    if (phase_ms) std::copy(ph, ph + MEASURE_PHASES, phase_ms);
    if (emit) {
        float ms = 0.f;
        MSCHK(hipEventElapsedTime(&ms, res.ev[11], res.ev[12]));
        emit->offsets_ms = ms;
    }
    return TW_OK;
}

void measure_emit_free(MeasureEmit* e) {
    if (e->buf) (void)hipFree(e->buf);
    if (e->lat) (void)hipFree(e->lat);
    *e = MeasureEmit{};
}

}  // namespace tw
