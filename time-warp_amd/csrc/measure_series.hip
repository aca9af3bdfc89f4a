// measure_series.hip — tw_measure_series' device pass (include/timewarp.h):
// TRACE records binned over virtual time for every replica of a batch.  The
// records sit as [n][R][2] quads (measure.hip's header: every geometry, a traced
// batched LP context and, with R == 1, a node-partitioned shard's block alike);
// the bin of a time is series_bin (measure_series.hpp), the one rule the host
// restatement shares.  Global atomics execute at the memory side, so every
// kernel keeps its histogram in workgroup-private LDS and flushes one 64-bit
// global atomic per non-empty bin per workgroup.
//
//   tw_series_init   one lane per replica: a truncated replica (emitted > cap)
//     counts once and gets its per-replica entry; the batch's t_min / t_max and
//     the LATENCY stats get their empty values.
//   tw_series_count<PER>   EVENTS.  A workgroup takes a tile of T neighbouring
//     replicas (a wave reads T x 32 contiguous bytes per n) and walks n with a
//     grid stride over `chunks` workgroups per tile; with R == 1 that is a plain
//     grid-stride walk over the records.  !PER: one LDS histogram of n_bins
//     32-bit counters for the tile; the host picks `chunks` so that a lane sees
//     at most 2^20 records, a workgroup fewer than 2^32.  PER (per-replica
//     outputs asked for): T x n_bins <= 8192 counters, a row per replica of the
//     tile, chunks == 1 -- the workgroup owns its replicas over all n, so their
//     rows and tw_series_out entries leave as plain stores, and the batch's
//     counts are the rows summed in LDS first.
//   FIRST: a table of int64 first times per (replica, node) of a chunk of
//     replicas (series_chunks: at most SERIES_MAX_ENTRIES entries at a time),
//     tw_series_table_init sets it to INT64_MAX, tw_series_first_fill walks the
//     records as the count kernel does and takes a 64-bit atomic min per
//     matching record, tw_series_first_bin<PER> bins one lane per entry (PER: a
//     workgroup owns the entries of its tile's replicas, contiguous in the
//     replica-major table).
//   LATENCY: measure.hip's join in its ME_TIMES state leaves (d, t_from) per
//     pair in the replicas' segments; tw_series_lat<PER> gives a wave a replica
//     at a time, bins t_from and folds (count, sum, min, max) of d per bin in
//     LDS -- 1,024 bins x 32 B -- flushed with 64-bit global atomics.  PER: a
//     wave-private row of pair counts per replica, stored plainly.
// Everything is integer: the order of the atomics changes no result.  Every
// barrier is under a workgroup-uniform condition; no lane waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/timewarp.h"
#include "measure_series.hpp"
#include "shard.hpp"

namespace {

using tw::SERIES_OVER;
using tw::SERIES_UNDER;
using tw::series_bin;

constexpr uint32_t SR_WG = 256;
constexpr uint32_t SR_CTRS = 8192;     // LDS counters of a count / bin workgroup
constexpr uint32_t SR_TILE_LOG2 = 6;   // replicas per tile at most: a wave's lanes
constexpr uint32_t SR_TILE = 1u << SR_TILE_LOG2;
constexpr uint32_t SR_LANE_RECORDS = 1u << 20;  // records one lane of a !PER count workgroup walks at most
constexpr uint32_t SR_ERR_NODE = 1;    // a record's node is outside the scenario
static_assert(SR_CTRS == TW_SERIES_MAX_BINS, "one replica's row fits the counters at T = 1");
static_assert(SR_CTRS * 4 + SR_TILE * 28 + 256 <= 64 * 1024, "static LDS of the count and bin kernels");
static_assert(TW_SERIES_MAX_LAT_BINS * 32 + 4 * TW_SERIES_MAX_LAT_BINS * 4 + 256 <= 64 * 1024,
              "static LDS of tw_series_lat<true>");

struct SrStat {  // LATENCY's per-bin folds on the device, one array each
    unsigned long long* sum;
    long long* min;
    long long* max;
};

// the accumulators of the replicas of a tile, in LDS: what a workgroup knows of
// each replica's items besides their bins
struct SrTile {
    uint32_t n[SR_TILE], uf[SR_TILE], of[SR_TILE];
    long long min[SR_TILE], max[SR_TILE];
};

// a lane's items of one replica, in registers until they are flushed into the tile
struct SrLane {
    uint32_t n = 0, uf = 0, of = 0;
    long long min = INT64_MAX, max = INT64_MIN;
    __device__ __forceinline__ void item(int64_t t, uint32_t bin) {
        ++n;
        uf += bin == SERIES_UNDER ? 1u : 0u;
        of += bin == SERIES_OVER ? 1u : 0u;
        min = t < min ? t : min;
        max = t > max ? t : max;
    }
    __device__ __forceinline__ void flush(SrTile& s, uint32_t dr) {
        if (!n) return;
        atomicAdd(&s.n[dr], n);
        if (uf) atomicAdd(&s.uf[dr], uf);
        if (of) atomicAdd(&s.of[dr], of);
        __hip_atomic_fetch_min(&s.min[dr], min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(&s.max[dr], max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        *this = SrLane{};
    }
};

__device__ __forceinline__ void sr_tile_clear(SrTile& s, uint32_t tid) {
    if (tid < SR_TILE) {
        s.n[tid] = s.uf[tid] = s.of[tid] = 0;
        s.min[tid] = INT64_MAX;
        s.max[tid] = INT64_MIN;
    }
}

// thread 0, behind a barrier: the tile's replicas [0, T) summed into the batch's totals
__device__ __forceinline__ void sr_tile_total(const SrTile& s, uint32_t T, tw_series_out* total) {
    unsigned long long n = 0, uf = 0, of = 0;
    long long mn = INT64_MAX, mx = INT64_MIN;
    for (uint32_t i = 0; i < T; ++i) {
        n += s.n[i]; uf += s.uf[i]; of += s.of[i];
        mn = s.min[i] < mn ? s.min[i] : mn;
        mx = s.max[i] > mx ? s.max[i] : mx;
    }
    if (!n) return;
    atomicAdd((unsigned long long*)&total->counted, n);
    if (uf) atomicAdd((unsigned long long*)&total->underflow, uf);
    if (of) atomicAdd((unsigned long long*)&total->overflow, of);
    __hip_atomic_fetch_min((long long*)&total->t_min, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max((long long*)&total->t_max, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ tw_series_out sr_out_of(const SrTile& s, uint32_t dr) {
    tw_series_out o;
    o.counted = s.n[dr]; o.underflow = s.uf[dr]; o.overflow = s.of[dr]; o.truncated = 0;
    o.t_min = s.min[dr]; o.t_max = s.max[dr];
    return o;
}

__device__ __forceinline__ int64_t sr_time(const uint4& a) { return (int64_t)(((uint64_t)a.y << 32) | a.x); }

// (the rest of *total was zeroed by the host's memset)
__global__ __launch_bounds__(SR_WG) void tw_series_init(const uint64_t* __restrict__ emitted, uint32_t R, uint32_t cap,
                                                        uint32_t n_stat, tw_series_out* total, tw_series_out* per,
                                                        SrStat st) {
    const uint32_t i = blockIdx.x * SR_WG + threadIdx.x;
    if (i == 0) {
        total->t_min = INT64_MAX;
        total->t_max = INT64_MIN;
    }
    if (i < n_stat) {  // (LATENCY; sums zeroed by the memset)
        st.min[i] = INT64_MAX;
        st.max[i] = INT64_MIN;
    }
    if (i >= R || emitted[i] <= cap) return;
    atomicAdd((unsigned long long*)&total->truncated, 1ull);  // (rare: one atomic per truncated replica)
    if (per) {
        tw_series_out o{};
        o.truncated = 1;
        o.t_min = INT64_MAX;
        o.t_max = INT64_MIN;
        per[i] = o;
    }
}

// Replicas r_lo + [0, r_n) of the R in the buffer; a workgroup: tile
// blockIdx.x % tiles of T = 1 << tlog2 of them, lane (n, r) -> tid = n * T + dr,
// n from (blockIdx.x / tiles) * (SR_WG / T) in steps of chunks * (SR_WG / T).
template <bool PER>
__global__ __launch_bounds__(SR_WG) void tw_series_count(const uint4* __restrict__ trace,
                                                         const uint64_t* __restrict__ emitted, uint32_t R, uint32_t cap,
                                                         uint32_t tag, int64_t t0_us, int64_t bin_us, uint32_t n_bins,
                                                         uint32_t tlog2, uint32_t tiles, uint32_t chunks,
                                                         tw_series_out* total, unsigned long long* count,
                                                         tw_series_out* __restrict__ per,
                                                         unsigned long long* __restrict__ per_count) {
    __shared__ uint32_t s_c[SR_CTRS];
    __shared__ SrTile s_t;
    const uint32_t tid = threadIdx.x;
    const uint32_t T = 1u << tlog2, n_step = SR_WG >> tlog2;
    const uint32_t used = PER ? n_bins << tlog2 : n_bins;  // <= SR_CTRS (the host chose tlog2 so)
    const uint32_t r0 = (blockIdx.x % tiles) << tlog2, dr = tid & (T - 1), r = r0 + dr;
    for (uint32_t i = tid; i < used; i += SR_WG) s_c[i] = 0;
    sr_tile_clear(s_t, tid);
    __syncthreads();
    uint32_t kept = 0;
    if (r < R) {
        const uint64_t em = emitted[r];
        kept = em > cap ? 0u : (uint32_t)em;  // (a truncated replica: tw_series_init's)
    }
    const uint32_t row = PER ? dr * n_bins : 0u;
    SrLane me;
    const uint64_t stride = (uint64_t)chunks * n_step;
    for (uint64_t n = (uint64_t)(blockIdx.x / tiles) * n_step + (tid >> tlog2); n < kept; n += stride) {
        const uint4 a = trace[((size_t)n * R + r) * 2];
        if (a.w != tag) continue;
        const int64_t t = sr_time(a);
        const uint32_t b = series_bin(t, t0_us, bin_us, n_bins);
        me.item(t, b);
        if (b < n_bins) atomicAdd(&s_c[row + b], 1u);
    }
    me.flush(s_t, dr);
    __syncthreads();
    if (PER) {
        // the rows and entries of the tile's replicas: this workgroup alone holds them
        if (per_count)
            for (uint32_t i = tid; i < used; i += SR_WG) {
                const uint32_t rr = r0 + i / n_bins;
                if (rr < R) per_count[(size_t)rr * n_bins + i % n_bins] = s_c[i];
            }
        if (per && tid < T && r0 + tid < R && emitted[r0 + tid] <= cap) per[r0 + tid] = sr_out_of(s_t, tid);
        for (uint32_t b = tid; b < n_bins; b += SR_WG) {
            unsigned long long c = 0;
            for (uint32_t i = 0; i < T; ++i) c += s_c[i * n_bins + b];
            if (c) atomicAdd(&count[b], c);
        }
    } else {
        for (uint32_t b = tid; b < n_bins; b += SR_WG)
            if (s_c[b]) atomicAdd(&count[b], (unsigned long long)s_c[b]);
    }
    if (tid == 0) sr_tile_total(s_t, T, total);
}

__global__ __launch_bounds__(SR_WG) void tw_series_table_init(long long* __restrict__ table, unsigned long long n) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * SR_WG + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * SR_WG)
        table[i] = INT64_MAX;
}

// the walk of tw_series_count over replicas r_lo + [0, r_n): table[(r - r_lo) * N + node] = min(., t)
__global__ __launch_bounds__(SR_WG) void tw_series_first_fill(const uint4* __restrict__ trace,
                                                              const uint64_t* __restrict__ emitted, uint32_t R,
                                                              uint32_t cap, uint32_t tag, uint32_t r_lo, uint32_t r_n,
                                                              uint32_t N, uint32_t tlog2, uint32_t tiles,
                                                              uint32_t chunks, long long* table, uint32_t* err) {
    const uint32_t tid = threadIdx.x;
    const uint32_t T = 1u << tlog2, n_step = SR_WG >> tlog2;
    const uint32_t q = ((blockIdx.x % tiles) << tlog2) + (tid & (T - 1));  // the replica within the chunk
    if (q >= r_n) return;
    const uint32_t r = r_lo + q;  // < R
    const uint64_t em = emitted[r];
    const uint32_t kept = em > cap ? 0u : (uint32_t)em;
    const uint64_t stride = (uint64_t)chunks * n_step;
    for (uint64_t n = (uint64_t)(blockIdx.x / tiles) * n_step + (tid >> tlog2); n < kept; n += stride) {
        const uint4 a = trace[((size_t)n * R + r) * 2];
        if (a.w != tag) continue;
        if (a.z >= N) {
            atomicOr(err, SR_ERR_NODE);
            continue;
        }
        __hip_atomic_fetch_min(&table[(size_t)q * N + a.z], (long long)sr_time(a), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One lane per table entry.  !PER: the grid strides over the chunk's r_n x N
// entries, one histogram per workgroup.  PER: workgroup g owns replicas
// (g << tlog2) + [0, T) of the chunk, whose entries are contiguous.
template <bool PER>
__global__ __launch_bounds__(SR_WG) void tw_series_first_bin(const long long* __restrict__ table,
                                                             const uint64_t* __restrict__ emitted, uint32_t cap,
                                                             uint32_t r_lo, uint32_t r_n, uint32_t N, int64_t t0_us,
                                                             int64_t bin_us, uint32_t n_bins, uint32_t tlog2,
                                                             tw_series_out* total, unsigned long long* count,
                                                             tw_series_out* __restrict__ per,
                                                             unsigned long long* __restrict__ per_count) {
    __shared__ uint32_t s_c[SR_CTRS];
    __shared__ SrTile s_t;
    const uint32_t tid = threadIdx.x;
    const uint32_t T = PER ? 1u << tlog2 : 1u;
    const uint32_t used = PER ? n_bins << tlog2 : n_bins;
    const uint32_t q0 = PER ? blockIdx.x << tlog2 : 0u;  // < r_n (the grid is the tiles)
    const uint32_t q1 = PER ? (r_n - q0 < T ? r_n : q0 + T) : r_n;
    const unsigned long long e0 = PER ? (unsigned long long)q0 * N + tid : (unsigned long long)blockIdx.x * SR_WG + tid;
    const unsigned long long e1 = (unsigned long long)q1 * N;
    const unsigned long long step = PER ? SR_WG : (unsigned long long)gridDim.x * SR_WG;
    for (uint32_t i = tid; i < used; i += SR_WG) s_c[i] = 0;
    sr_tile_clear(s_t, tid);
    __syncthreads();
    SrLane me;
    uint32_t cur = 0;  // the replica of the tile `me` holds items of
    for (unsigned long long e = e0; e < e1; e += step) {
        const long long t = table[e];
        if (t == INT64_MAX) continue;  // no record of the tag at this node
        const uint32_t dr = PER ? (uint32_t)(e / N) - q0 : 0u;
        if (dr != cur) {
            me.flush(s_t, cur);
            cur = dr;
        }
        const uint32_t b = series_bin(t, t0_us, bin_us, n_bins);
        me.item(t, b);
        if (b < n_bins) atomicAdd(&s_c[(PER ? dr * n_bins : 0u) + b], 1u);
    }
    me.flush(s_t, cur);
    __syncthreads();
    if (PER) {
        if (per_count)
            for (uint32_t i = tid; i < used; i += SR_WG) {
                const uint32_t q = q0 + i / n_bins;
                if (q < r_n) per_count[(size_t)(r_lo + q) * n_bins + i % n_bins] = s_c[i];
            }
        if (per && tid < T && q0 + tid < r_n && emitted[r_lo + q0 + tid] <= cap) per[r_lo + q0 + tid] = sr_out_of(s_t, tid);
        for (uint32_t b = tid; b < n_bins; b += SR_WG) {
            unsigned long long c = 0;
            for (uint32_t i = 0; i < T; ++i) c += s_c[i * n_bins + b];
            if (c) atomicAdd(&count[b], c);
        }
    } else {
        for (uint32_t b = tid; b < n_bins; b += SR_WG)
            if (s_c[b]) atomicAdd(&count[b], (unsigned long long)s_c[b]);
    }
    if (tid == 0) sr_tile_total(s_t, T, total);
}

__device__ __forceinline__ unsigned long long sr_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // (lane 0's)
}
__device__ __forceinline__ long long sr_wave_min(long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const long long w = __shfl_down(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ long long sr_wave_max(long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const long long w = __shfl_down(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// The pairs of replica r: (lat, tfrom)[off[r] .. off[r] + fill[r]).  A wave
// takes a replica at a time; the four waves of a workgroup share the per-bin
// folds in LDS.  PER: s_row[wave] is the replica's row of pair counts, touched
// by that wave alone (its LDS operations execute in program order).
template <bool PER>
__global__ __launch_bounds__(SR_WG) void tw_series_lat(const unsigned long long* __restrict__ off,
                                                       const uint32_t* __restrict__ fill,
                                                       const long long* __restrict__ lat,
                                                       const long long* __restrict__ tfrom,
                                                       const uint64_t* __restrict__ emitted, uint32_t R, uint32_t cap,
                                                       int64_t t0_us, int64_t bin_us, uint32_t n_bins,
                                                       tw_series_out* total, unsigned long long* count, SrStat st,
                                                       tw_series_out* __restrict__ per,
                                                       unsigned long long* __restrict__ per_count) {
    __shared__ unsigned long long s_n[TW_SERIES_MAX_LAT_BINS], s_sum[TW_SERIES_MAX_LAT_BINS];
    __shared__ long long s_min[TW_SERIES_MAX_LAT_BINS], s_max[TW_SERIES_MAX_LAT_BINS];
    __shared__ uint32_t s_row[PER ? SR_WG / 64 : 1][PER ? TW_SERIES_MAX_LAT_BINS : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t b = tid; b < n_bins; b += SR_WG) {
        s_n[b] = 0;
        s_sum[b] = 0;
        s_min[b] = INT64_MAX;
        s_max[b] = INT64_MIN;
    }
    __syncthreads();
    // the wave's items: this lane's share, over all its replicas
    unsigned long long w_n = 0, w_uf = 0, w_of = 0;
    long long w_min = INT64_MAX, w_max = INT64_MIN;
    const uint32_t waves = gridDim.x * (SR_WG / 64);
    for (uint32_t r = blockIdx.x * (SR_WG / 64) + wave; r < R; r += waves) {  // (r: uniform over the wave)
        if (emitted[r] > cap) continue;  // truncated: tw_series_init's
        const unsigned long long seg = off[r], room = off[r + 1] - seg;
        const unsigned long long f = fill[r] < room ? fill[r] : room;
        if (PER) {
            for (uint32_t b = lane; b < n_bins; b += 64) s_row[wave][b] = 0;
            __builtin_amdgcn_wave_barrier();
        }
        SrLane me;
        for (unsigned long long i = lane; i < f; i += 64) {
            const long long d = lat[seg + i], t = tfrom[seg + i];
            const uint32_t b = series_bin(t, t0_us, bin_us, n_bins);
            me.item(t, b);
            if (b < n_bins) {
                atomicAdd(&s_n[b], 1ull);
                atomicAdd(&s_sum[b], (unsigned long long)d);
                __hip_atomic_fetch_min(&s_min[b], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_max(&s_max[b], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (PER) atomicAdd(&s_row[wave][b], 1u);
            }
        }
        if (PER) {
            // (every lane of the wave is here: r and the loop bounds are the wave's)
            tw_series_out o;
            o.counted = sr_wave_sum(me.n); o.underflow = sr_wave_sum(me.uf); o.overflow = sr_wave_sum(me.of);
            o.truncated = 0;
            o.t_min = sr_wave_min(me.min); o.t_max = sr_wave_max(me.max);
            if (lane == 0 && per) per[r] = o;
            __builtin_amdgcn_wave_barrier();
            if (per_count)
                for (uint32_t b = lane; b < n_bins; b += 64) per_count[(size_t)r * n_bins + b] = s_row[wave][b];
            __builtin_amdgcn_wave_barrier();
        }
        w_n += me.n; w_uf += me.uf; w_of += me.of;
        w_min = me.min < w_min ? me.min : w_min;
        w_max = me.max > w_max ? me.max : w_max;
    }
    w_n = sr_wave_sum(w_n); w_uf = sr_wave_sum(w_uf); w_of = sr_wave_sum(w_of);
    w_min = sr_wave_min(w_min); w_max = sr_wave_max(w_max);
    if (lane == 0 && w_n) {
        atomicAdd((unsigned long long*)&total->counted, w_n);
        if (w_uf) atomicAdd((unsigned long long*)&total->underflow, w_uf);
        if (w_of) atomicAdd((unsigned long long*)&total->overflow, w_of);
        __hip_atomic_fetch_min((long long*)&total->t_min, w_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max((long long*)&total->t_max, w_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (uint32_t b = tid; b < n_bins; b += SR_WG) {
        if (!s_n[b]) continue;
        atomicAdd(&count[b], s_n[b]);
        atomicAdd(&st.sum[b], s_sum[b]);
        __hip_atomic_fetch_min(&st.min[b], s_min[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&st.max[b], s_max[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the call's device scratch and events, released on every return path
struct SrRes {
    void* buf = nullptr;
    void* table = nullptr;
    std::vector<hipEvent_t> ev;
    tw::MeasureEmit emit;
    ~SrRes() {
        if (buf) (void)hipFree(buf);
        if (table) (void)hipFree(table);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        tw::measure_emit_free(&emit);
    }
};

#define SRCHK(x)                                                                     \
    do {                                                                             \
        hipError_t _e = (x);                                                         \
        if (_e != hipSuccess) {                                                      \
            fprintf(stderr, "timewarp: %s failed: %s\n", #x, hipGetErrorString(_e)); \
            return _e == hipErrorOutOfMemory ? TW_ERR_OOM : TW_ERR_HIP;              \
        }                                                                            \
    } while (0)

// the record walk's geometry over Rn replicas of up to cap records: the tile
// (at most 1 << max_tlog2 replicas, no wider than the replicas need) and the
// workgroups per tile
struct SrWalk {
    uint32_t tlog2, tiles, chunks;
    uint64_t grid() const { return (uint64_t)tiles * chunks; }
};

SrWalk sr_walk(uint32_t Rn, uint32_t cap, uint32_t max_tlog2, bool own_all_n) {
    SrWalk w;
    w.tlog2 = max_tlog2 < SR_TILE_LOG2 ? max_tlog2 : SR_TILE_LOG2;
    while (w.tlog2 > 0 && (1u << (w.tlog2 - 1)) >= Rn) --w.tlog2;
    w.tiles = (uint32_t)(((uint64_t)Rn + (1u << w.tlog2) - 1) >> w.tlog2);
    w.chunks = 1;
    if (!own_all_n) {
        // about 16 records a lane, within some 8192 workgroups; and never more
        // than SR_LANE_RECORDS a lane: a workgroup's 32-bit counters see fewer
        // than SR_WG x 2^20 records
        const uint64_t n_step = SR_WG >> w.tlog2;
        uint64_t c = ((uint64_t)cap + n_step * 16 - 1) / (n_step * 16);
        const uint64_t most = std::max<uint64_t>(1, 8192 / w.tiles);
        c = std::min(std::max<uint64_t>(c, 1), most);
        while (((uint64_t)cap + c * n_step - 1) / (c * n_step) > SR_LANE_RECORDS) c *= 2;
        w.chunks = (uint32_t)c;
    }
    return w;
}

uint32_t sr_row_tlog2(uint32_t n_bins) {  // the largest T with T x n_bins <= SR_CTRS
    uint32_t l = 0;
    while (l < SR_TILE_LOG2 && ((uint64_t)n_bins << (l + 1)) <= SR_CTRS) ++l;
    return l;
}

}  // namespace

namespace tw {

int series_run(int device, hipStream_t stream, const uint4* trace, const uint64_t* emitted, uint32_t R, uint32_t cap,
               uint32_t n_nodes, uint64_t max_entries, const tw_series_spec* spec, const MeasureCfg& cfg,
               tw_series_out* total, uint64_t* count, tw_series_stat* stat, tw_series_out* per, uint64_t* per_count,
               double* phase_ms) {
    if (!series_spec_ok(spec) || !trace || !emitted || cap == 0) return TW_ERR_INVALID;
    const uint32_t nb = spec->n_bins;
    const bool is_lat = spec->mode == TW_SERIES_LATENCY, is_first = spec->mode == TW_SERIES_FIRST;
    if (stat && !is_lat) return TW_ERR_INVALID;
    double ph[SERIES_PHASES] = {};
    SeriesChunks plan;
    if (is_first && R) {
        if (max_entries == 0 || max_entries > SERIES_MAX_ENTRIES) max_entries = SERIES_MAX_ENTRIES;
        plan = series_chunks(R, n_nodes, max_entries);
        if (!plan.per_chunk) return TW_ERR_INVALID;
    }
    if (R == 0) {
        if (total) series_empty(total);
        if (count) std::memset(count, 0, (size_t)nb * 8);
        if (stat)
            for (uint32_t b = 0; b < nb; ++b) series_stat_empty(&stat[b]);
        if (phase_ms) std::copy(ph, ph + SERIES_PHASES, phase_ms);
        return TW_OK;
    }
    const bool rows = per || per_count;
    // scratch: err word | total | count[nb] | sum[nb] min[nb] max[nb] (LATENCY) | per[R] | per_count[R][nb]
    const size_t o_total = 8, o_count = o_total + sizeof(tw_series_out), o_stat = o_count + (size_t)nb * 8;
    const size_t o_per = o_stat + (is_lat ? (size_t)nb * 24 : 0);
    const size_t o_rows = o_per + (per ? (size_t)R * sizeof(tw_series_out) : 0);
    const size_t bytes = o_rows + (per_count ? (size_t)R * nb * 8 : 0);
    SrRes res;
    SRCHK(hipSetDevice(device));
    if (hipMalloc(&res.buf, bytes) != hipSuccess) {
        (void)hipGetLastError();  // (not sticky: the context stays usable)
        return TW_ERR_OOM;
    }
    char* base = (char*)res.buf;
    uint32_t* d_err = (uint32_t*)base;
    tw_series_out* d_total = (tw_series_out*)(base + o_total);
    unsigned long long* d_count = (unsigned long long*)(base + o_count);
    SrStat d_st{nullptr, nullptr, nullptr};
    if (is_lat) {
        d_st.sum = (unsigned long long*)(base + o_stat);
        d_st.min = (long long*)(base + o_stat + (size_t)nb * 8);
        d_st.max = (long long*)(base + o_stat + (size_t)nb * 16);
    }
    tw_series_out* d_per = per ? (tw_series_out*)(base + o_per) : nullptr;
    unsigned long long* d_rows = per_count ? (unsigned long long*)(base + o_rows) : nullptr;
    auto event = [&](hipEvent_t* e) {
        res.ev.push_back(nullptr);
        hipError_t rc = hipEventCreate(&res.ev.back());
        *e = res.ev.back();
        return rc;
    };
    auto elapsed = [&](hipEvent_t a, hipEvent_t b, double* into) {
        float ms = 0.f;
        hipError_t rc = hipEventElapsedTime(&ms, a, b);
        *into += ms;
        return rc;
    };

    SRCHK(hipMemsetAsync(base, 0, bytes, stream));
    const uint32_t n_init = std::max(R, is_lat ? nb : 0u);
    tw_series_init<<<(n_init + SR_WG - 1) / SR_WG, SR_WG, 0, stream>>>(emitted, R, cap, is_lat ? nb : 0u, d_total, d_per,
                                                                      d_st);
    SRCHK(hipGetLastError());
    const uint32_t row_tlog2 = sr_row_tlog2(nb);
    std::vector<hipEvent_t> spans;  // FIRST: (start, filled, binned) per chunk; otherwise (start, end)
    if (spec->mode == TW_SERIES_EVENTS) {
        const SrWalk w = sr_walk(R, cap, rows ? row_tlog2 : SR_TILE_LOG2, rows);
        if (w.grid() > 0x7FFFFFFFull) return TW_ERR_INVALID;
        spans.resize(2);
        SRCHK(event(&spans[0]));
        SRCHK(event(&spans[1]));
        SRCHK(hipEventRecord(spans[0], stream));
        if (rows)
            tw_series_count<true><<<(uint32_t)w.grid(), SR_WG, 0, stream>>>(trace, emitted, R, cap, spec->tag,
                                                                           spec->t0_us, spec->bin_us, nb, w.tlog2,
                                                                           w.tiles, w.chunks, d_total, d_count, d_per,
                                                                           d_rows);
        else
            tw_series_count<false><<<(uint32_t)w.grid(), SR_WG, 0, stream>>>(trace, emitted, R, cap, spec->tag,
                                                                            spec->t0_us, spec->bin_us, nb, w.tlog2,
                                                                            w.tiles, w.chunks, d_total, d_count,
                                                                            nullptr, nullptr);
        SRCHK(hipGetLastError());
        SRCHK(hipEventRecord(spans[1], stream));
    } else if (is_first) {
        const size_t entries = (size_t)plan.per_chunk * n_nodes;  // <= SERIES_MAX_ENTRIES
        if (hipMalloc(&res.table, entries * 8) != hipSuccess) {
            (void)hipGetLastError();
            return TW_ERR_OOM;
        }
        long long* d_table = (long long*)res.table;
        spans.resize((size_t)plan.n_chunks * 3);
        for (hipEvent_t& e : spans) SRCHK(event(&e));
        for (uint32_t k = 0; k < plan.n_chunks; ++k) {
            uint32_t r_lo = 0, r_n = 0;
            series_chunk_at(plan, R, k, &r_lo, &r_n);
            if (!r_n) continue;
            const unsigned long long ne = (unsigned long long)r_n * n_nodes;
            const SrWalk w = sr_walk(r_n, cap, SR_TILE_LOG2, false);
            if (w.grid() > 0x7FFFFFFFull) return TW_ERR_INVALID;
            SRCHK(hipEventRecord(spans[3 * k], stream));
            const uint32_t igrid = (uint32_t)std::min<unsigned long long>((ne + SR_WG - 1) / SR_WG, 4096);
            tw_series_table_init<<<igrid, SR_WG, 0, stream>>>(d_table, ne);
            SRCHK(hipGetLastError());
            tw_series_first_fill<<<(uint32_t)w.grid(), SR_WG, 0, stream>>>(trace, emitted, R, cap, spec->tag, r_lo, r_n,
                                                                          n_nodes, w.tlog2, w.tiles, w.chunks, d_table,
                                                                          d_err);
            SRCHK(hipGetLastError());
            SRCHK(hipEventRecord(spans[3 * k + 1], stream));
            if (rows) {
                const uint32_t tiles = (uint32_t)(((uint64_t)r_n + (1u << row_tlog2) - 1) >> row_tlog2);
                tw_series_first_bin<true><<<tiles, SR_WG, 0, stream>>>(d_table, emitted, cap, r_lo, r_n, n_nodes,
                                                                      spec->t0_us, spec->bin_us, nb, row_tlog2, d_total,
                                                                      d_count, d_per, d_rows);
            } else {
                tw_series_first_bin<false><<<igrid, SR_WG, 0, stream>>>(d_table, emitted, cap, r_lo, r_n, n_nodes,
                                                                       spec->t0_us, spec->bin_us, nb, 0u, d_total,
                                                                       d_count, nullptr, nullptr);
            }
            SRCHK(hipGetLastError());
            SRCHK(hipEventRecord(spans[3 * k + 2], stream));
        }
    } else {
        // the join of tw_measure(tag, tag_to) with its pairs left on the device
        // (one bin that is never counted: the emit states bin nothing)
        tw_measure_spec ms{};
        ms.tag_from = spec->tag;
        ms.tag_to = spec->tag_to;
        ms.n_bins = 1;
        ms.bin_us = 1;
        tw_measure_out mt;
        double jms = 0.0;
        res.emit.with_t = true;
        int rc = measure_run(device, stream, trace, emitted, R, cap, &ms, cfg, &mt, nullptr, nullptr, &jms, nullptr,
                             &res.emit);
        if (rc) return rc;
        ph[0] = jms + res.emit.offsets_ms;
        spans.resize(2);
        SRCHK(event(&spans[0]));
        SRCHK(event(&spans[1]));
        SRCHK(hipEventRecord(spans[0], stream));
        const uint32_t grid = std::min<uint32_t>((R + SR_WG / 64 - 1) / (SR_WG / 64), 1024);
        if (rows)
            tw_series_lat<true><<<grid, SR_WG, 0, stream>>>(res.emit.off, res.emit.fill, res.emit.lat, res.emit.tfrom,
                                                           emitted, R, cap, spec->t0_us, spec->bin_us, nb, d_total,
                                                           d_count, d_st, d_per, d_rows);
        else
            tw_series_lat<false><<<grid, SR_WG, 0, stream>>>(res.emit.off, res.emit.fill, res.emit.lat, res.emit.tfrom,
                                                            emitted, R, cap, spec->t0_us, spec->bin_us, nb, d_total,
                                                            d_count, d_st, nullptr, nullptr);
        SRCHK(hipGetLastError());
        SRCHK(hipEventRecord(spans[1], stream));
    }
    // host copies of the device results: the caller's buffers are written only
    // once everything has succeeded
    std::vector<char> h_head(o_per);
    std::vector<tw_series_out> h_per(per ? R : 0);
    std::vector<uint64_t> h_rows(per_count ? (size_t)R * nb : 0);
    SRCHK(hipMemcpyAsync(h_head.data(), base, o_per, hipMemcpyDeviceToHost, stream));
    if (per) SRCHK(hipMemcpyAsync(h_per.data(), d_per, (size_t)R * sizeof(tw_series_out), hipMemcpyDeviceToHost, stream));
    if (per_count) SRCHK(hipMemcpyAsync(h_rows.data(), d_rows, (size_t)R * nb * 8, hipMemcpyDeviceToHost, stream));
    SRCHK(hipStreamSynchronize(stream));
    uint32_t h_err = 0;
    std::memcpy(&h_err, h_head.data(), 4);
    if (h_err) return TW_ERR_STATE;  // a record names a node the scenario does not have
    if (is_first) {
        for (uint32_t k = 0; k < plan.n_chunks; ++k) {
            SRCHK(elapsed(spans[3 * k], spans[3 * k + 1], &ph[1]));
            SRCHK(elapsed(spans[3 * k + 1], spans[3 * k + 2], &ph[2]));
        }
    } else {
        SRCHK(elapsed(spans[0], spans[1], &ph[is_lat ? 3 : 2]));
    }
    if (total) std::memcpy(total, h_head.data() + o_total, sizeof(tw_series_out));
    if (count) std::memcpy(count, h_head.data() + o_count, (size_t)nb * 8);
    if (stat) {
        const char* s = h_head.data() + o_stat;
        for (uint32_t b = 0; b < nb; ++b) {
            std::memcpy(&stat[b].sum_us, s + (size_t)b * 8, 8);
            std::memcpy(&stat[b].min_us, s + ((size_t)nb + b) * 8, 8);
            std::memcpy(&stat[b].max_us, s + ((size_t)2 * nb + b) * 8, 8);
        }
    }
    if (per) std::memcpy(per, h_per.data(), (size_t)R * sizeof(tw_series_out));
    if (per_count) std::memcpy(per_count, h_rows.data(), (size_t)R * nb * 8);
    if (phase_ms) std::copy(ph, ph + SERIES_PHASES, phase_ms);
    return TW_OK;
}

}  // namespace tw
