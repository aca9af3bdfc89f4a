// prefix.hip — the send-free prefix of a run, computed once and copied
// (DESIGN §3m).
//
// Until a replica executes its first TW_OP_SEND it reads nothing of its own:
// the link table's column is a send's input, and the batch has no per-replica
// main registers.  So all replicas pass through the same states up to T0 - 1
// (prefix_classify.hpp).  sh_run lets one workgroup run that far (the pilot),
// gathers replica 0's parked state into a snapshot here, and stores it to
// every replica; later runs of the loaded scenario store the cached snapshot
// instead of re-running the chain of pops.
//
//   take    one thread per directory row: replica 0's element -> the snapshot
//   apply   one workgroup per (row, span of the row): the row's value to the
//           span's replicas; store-only, 16 B per lane where the row allows.
//           A row the last sweep proved unwritten in every replica since the
//           apply before, or that holds what tw_reset has
//           just left there, is left as it is: its workgroups return.  The
//           pilot's apply, and a cached one's early-exit form
//   list, apply_list
//           a cached apply's compact form (§3v): one thread per row writes the
//           (row, span) pairs of the rows that are stored, then one workgroup
//           per listed pair stores it: no workgroup for a row left as it is
//   audit   the testing hook's check of those rows (read-only), and its count
//           of them by class
//
// Every per-replica array is replica-minor, so a row is R contiguous elements.
// Plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tw_dev.hpp"
#include "prefix_dev.hpp"
#include "sweep_dev.hpp"

namespace {

using namespace tw;

__global__ void __launch_bounds__(256) tw_prefix_take(PrefixTab t) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.n_rows) return;
    const PrefixRow e = gp(t.rows)[i];
    const uint8_t GAS* src = (const uint8_t GAS*)(uintptr_t)e.dst;
    uint8_t GAS* dst = gp(t.snap) + e.off;
    if (e.es == 1) {
        *dst = *src;
    } else if (e.es == 4) {
        *(uint32_t GAS*)dst = *(const uint32_t GAS*)src;
    } else if (e.es == 8) {
        *(uint2 GAS*)dst = *(const uint2 GAS*)src;
    } else {
        for (uint32_t k = 0; k < e.es; k += 16) *(uint4 GAS*)(dst + k) = *(const uint4 GAS*)(src + k);
    }
}

__device__ __forceinline__ uint32_t word_of(uint4 v, uint32_t i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// The class under which the apply leaves `row` unstored, RC_NONE: it stores it
// (§3o, §3v; prefix_dev.hpp has the rule).  The device's own flag words and
// dirty bytes decide for RC_BODY, RC_HDR and RC_RUN.
__device__ __forceinline__ uint32_t row_skipped(const PrefixTab& t, uint32_t row) {
    if (!t.cls) return RC_NONE;
    const uint32_t k = t.cls[row];
    if (k == RC_NONE) return RC_NONE;
    if (k == RC_RESET) return t.reset ? k : (uint32_t)RC_NONE;
    if (!t.dirty || t.cflags[k == RC_HDR ? CF_HDR_OK : CF_VALID] != 1u) return RC_NONE;
    return t.dirty[t.tag[row]] == 0 ? k : (uint32_t)RC_NONE;
}

// One workgroup's share: bytes [span * SPAN, + SPAN) of the 16-byte-aligned
// body of `row`.  A row of 4-byte (1-byte) elements starts on any dword (byte)
// when R is no multiple of 4 (16): the bytes in front of the first 16-byte
// boundary and behind the last go out as dwords (bytes) from the row's first
// workgroup.  The value is read once per wave, through the scalar cache (the
// row is uniform over the workgroup); only rows wider than 16 B (the
// handler-stack overflow, FXQ > 1) load their quad per lane.
__device__ __forceinline__ void store_span(const PrefixTab& t, uint32_t R, uint32_t row, uint32_t span) {
    const PrefixRow e = t.rows[row];
    const uint32_t es = e.es;
    const uint64_t len = (uint64_t)R * es;
    const uint64_t mis = (16u - (uint32_t)(e.dst & 15u)) & 15u;
    const uint64_t head = mis < len ? mis : len;
    const uint64_t body = (len - head) & ~15ull;
    const uint64_t b0 = (uint64_t)span * TW_PREFIX_SPAN;
    if (span != 0 && b0 >= body) return;
    const uint8_t* src = t.snap + e.off;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (es == 1) {
        const uint32_t u = (uint32_t)*src * 0x01010101u;
        v = make_uint4(u, u, u, u);
    } else if (es == 4) {
        const uint32_t u = *(const uint32_t*)src;
        v = make_uint4(u, u, u, u);
    } else if (es == 8) {
        const uint2 u = *(const uint2*)src;
        v = make_uint4(u.x, u.y, u.x, u.y);
    } else if (es == 16) {
        v = *(const uint4*)src;
    }
    uint8_t GAS* dst = (uint8_t GAS*)(uintptr_t)e.dst;
    const uint64_t b1 = b0 + TW_PREFIX_SPAN < body ? b0 + TW_PREFIX_SPAN : body;
    if (es <= 16) {
        for (uint64_t o = b0 + (uint64_t)threadIdx.x * 16u; o < b1; o += 256u * 16u) *(uint4 GAS*)(dst + head + o) = v;
    } else {
        for (uint64_t o = b0 + (uint64_t)threadIdx.x * 16u; o < b1; o += 256u * 16u)
            *(uint4 GAS*)(dst + head + o) = *(const uint4 GAS*)(gp(t.snap) + e.off + (uint32_t)((head + o) % es));
    }
    if (span != 0) return;
    const uint64_t tail0 = head + body, tail = len - tail0;  // (both edges: < 16 bytes each)
    if (es == 1) {
        if (threadIdx.x < head) dst[threadIdx.x] = (uint8_t)v.x;
        if (threadIdx.x < tail) dst[tail0 + threadIdx.x] = (uint8_t)v.x;
    } else if (es <= 8) {
        // (the pattern's period divides 16: word (b / 4) % 4 of v is the row's word at byte b)
        if (threadIdx.x < head / 4u) *(uint32_t GAS*)(dst + threadIdx.x * 4u) = word_of(v, threadIdx.x & 3u);
        if (threadIdx.x < tail / 4u) {
            const uint64_t b = tail0 + threadIdx.x * 4u;
            *(uint32_t GAS*)(dst + b) = word_of(v, (uint32_t)(b >> 2) & 3u);
        }
    }
}

// The early-exit form: one workgroup per (row, span of the widest row); those
// of a skipped row, and those past a narrower row's end, return.
__global__ void __launch_bounds__(256) tw_prefix_apply(PrefixTab t, uint32_t R) {
    if (row_skipped(t, blockIdx.x) != RC_NONE) return;
    store_span(t, R, blockIdx.x, blockIdx.y);
}

// The compact form (§3v): tw_prefix_list writes the (row, span) pairs of the
// rows the apply stores, on the device's own flags; tw_prefix_apply_list is
// launched over about that many workgroups (the host's count, from its copy of
// the flags) and walks the list by its grid, so every pair is stored whatever
// the grid.  A row's pairs are contiguous; rows come in any order.
__global__ void __launch_bounds__(256) tw_prefix_list(PrefixTab t, uint32_t R) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    if (row >= t.n_rows || row_skipped(t, row) != RC_NONE) return;
    const PrefixRow e = t.rows[row];
    const uint32_t ns = prefix_row_spans(e.dst, e.es, R);
    const uint32_t at = __hip_atomic_fetch_add(gp(t.list_n), ns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t s = 0; s < ns && at + s < t.list_cap; ++s) gp(t.list)[at + s] = make_uint2(row, s);
}

__global__ void __launch_bounds__(256) tw_prefix_apply_list(PrefixTab t, uint32_t R) {
    const uint32_t n = *t.list_n < t.list_cap ? *t.list_n : t.list_cap;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint2 p = t.list[i];
        store_span(t, R, p.x, p.y);
    }
}

// The rows tw_prefix_apply skipped (its own test, on the flags it read): every
// element of the row against the snapshot's.  Elements of 16, 8, 4 bytes and
// single bytes, each loaded whole from its own naturally aligned address, so a
// row that starts off a 16-byte boundary (R no multiple of 16) needs no head
// or tail: workgroup blockIdx.y takes elements [i0, i1) of the R.
// count[0] += the elements that differ; count[class] += 1 per skipped row (the
// device's own count of what its flags let the apply skip).
__global__ void __launch_bounds__(256) tw_prefix_audit(PrefixTab t, uint32_t R, unsigned long long* count) {
    const uint32_t k = row_skipped(t, blockIdx.x);
    if (k == RC_NONE) return;
    if (blockIdx.y == 0 && threadIdx.x == 0)
        __hip_atomic_fetch_add(gp(count) + k, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const PrefixRow e = t.rows[blockIdx.x];
    const uint32_t es = e.es;
    if (es > 16) return;  // (no class has such a row)
    const uint64_t per = TW_PREFIX_SPAN / es;
    const uint64_t i0 = (uint64_t)blockIdx.y * per;
    const uint64_t i1 = i0 + per < R ? i0 + per : R;
    const uint8_t* src = t.snap + e.off;
    const uint8_t GAS* dst = (const uint8_t GAS*)(uintptr_t)e.dst;
    uint32_t bad = 0;
    if (es == 16) {
        const uint4 v = *(const uint4*)src;
        for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256u) {
            const uint4 x = ((const uint4 GAS*)dst)[i];
            bad += (x.x != v.x || x.y != v.y || x.z != v.z || x.w != v.w) ? 1u : 0u;
        }
    } else if (es == 8) {
        const uint2 v = *(const uint2*)src;
        for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256u) {
            const uint2 x = ((const uint2 GAS*)dst)[i];
            bad += (x.x != v.x || x.y != v.y) ? 1u : 0u;
        }
    } else if (es == 4) {
        const uint32_t v = *(const uint32_t*)src;
        for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256u) bad += ((const uint32_t GAS*)dst)[i] != v ? 1u : 0u;
    } else if (es == 1) {
        const uint8_t v = *src;
        for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256u) bad += dst[i] != v ? 1u : 0u;
    }
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if ((threadIdx.x & 63u) == 0 && bad)
        __hip_atomic_fetch_add(gp(count), (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static_assert(PCL_FL_SHIFT == FL_SHIFT && PCL_EXC_SHIFT == EXC_SHIFT && PCL_F_MAIN == F_MAIN,
              "prefix_clean.hpp reads the record header of tw_dev.hpp");

}  // namespace

namespace tw {

CleanLayout clean_layout(const Dev& d) {
    return CleanLayout{(uint64_t)(uintptr_t)d.slots, (uint64_t)(uintptr_t)d.runs, d.R, d.RQ, d.S, d.Cr, d.N, d.n_insns,
                       (uint32_t)TW_RUNS};
}

bool prefix_directory(const Dev& d, const uint64_t* sc, uint32_t near_cap, std::vector<PrefixRow>& rows, size_t& bytes) {
    rows.clear();
    bytes = 0;
    const size_t R = d.R;
    const uint64_t bump = sc[SC_BUMP], free_n = sc[SC_FREE_N], far_n = sc[SC_FAR_N], near_n = sc[SC_NEAR_N];
    if (bump > d.S || free_n > d.S || far_n > d.Q || near_n > near_cap) return false;
    auto row = [&](const void* base, size_t elem, uint32_t es) {
        rows.push_back(PrefixRow{(uint64_t)(uintptr_t)base + (uint64_t)elem * es, 0u, es});
    };
    for (uint32_t f = 0; f < SC_COUNT; ++f) row(d.scal, (size_t)f * R, 8);
    for (uint32_t s = 0; s < bump; ++s)
        for (uint32_t q = 0; q < 4; ++q) row(d.slots, rec_row(d, s, q), 16);
    for (uint32_t i = 0; i < free_n; ++i) row(d.free_stk, (size_t)i * R, 4);
    for (uint32_t i = 0; i < far_n; ++i) row(d.far, (size_t)i * R, 16);
    if (d.Cr) {
        for (uint32_t j = 0; j < TW_RUNS; ++j) {
            const uint64_t rh = sc[SC_RH0 + j], rn = sc[SC_RC0 + j];
            if (rn > d.Cr || (rn && rh >= d.Cr)) return false;
            for (uint32_t k = 0; k < rn; ++k) {
                uint32_t pos = (uint32_t)rh + k;
                pos = pos >= d.Cr ? pos - d.Cr : pos;  // (a ring: the live window may wrap)
                row(d.runs, run_row(d, j, pos), 16);
            }
        }
    }
    for (uint32_t j = 0; j < near_n; ++j) row(d.near_spill, (size_t)j * R, 16);
    for (uint32_t i = 0; i < d.N * 4; ++i) row(d.nvars, (size_t)i * R, 8);
    for (uint32_t n = 0; n < d.N; ++n) {
        row(d.hash, (size_t)n * R, 8);
        row(d.bind, (size_t)n * R, 4);
        row(d.bind_own, (size_t)n * R, 4);
        row(d.bind_rel, (size_t)n * R, 4);
    }
    for (uint32_t e = 0; e < d.T; ++e) row(d.tmo_done, (size_t)e * R, 1);
    if (d.FXQ)
        for (uint32_t s = 0; s < bump; ++s) row(d.fx, (size_t)s * R * d.FXQ, 16u * d.FXQ);
    // widest elements first: every snapshot offset is then a multiple of its element size
    std::stable_sort(rows.begin(), rows.end(), [](const PrefixRow& a, const PrefixRow& b) { return a.es > b.es; });
    uint64_t off = 0;
    for (PrefixRow& r : rows) {
        r.off = (uint32_t)off;
        off += r.es;
    }
    if (off > 0xFFFFFFFFull) return false;
    bytes = (size_t)off;
    return true;
}

hipError_t prefix_take(const PrefixTab& t, hipStream_t st) {
    if (t.n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(tw_prefix_take, dim3((t.n_rows + 255u) / 256u), dim3(256), 0, st, t);
    return hipGetLastError();
}

hipError_t prefix_apply(const PrefixTab& t, uint32_t R, uint32_t max_es, uint32_t pairs, hipStream_t st) {
    if (t.n_rows == 0 || R == 0) return hipSuccess;
    if (t.list && t.cls) {
        hipError_t e = hipMemsetAsync(t.list_n, 0, 4, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tw_prefix_list, dim3((t.n_rows + 255u) / 256u), dim3(256), 0, st, t, R);
        const uint32_t grid = pairs < 1u ? 1u : pairs > t.list_cap ? t.list_cap : pairs;
        hipLaunchKernelGGL(tw_prefix_apply_list, dim3(grid), dim3(256), 0, st, t, R);
        return hipGetLastError();
    }
    // rows x spans: the whole chip stores at once (C3: ~70k rows of 256 KB - 1 MB)
    const uint64_t spans = ((uint64_t)R * max_es + TW_PREFIX_SPAN - 1) / TW_PREFIX_SPAN;
    hipLaunchKernelGGL(tw_prefix_apply, dim3(t.n_rows, (uint32_t)(spans ? spans : 1)), dim3(256), 0, st, t, R);
    return hipGetLastError();
}

hipError_t prefix_audit(const PrefixTab& t, uint32_t R, uint32_t max_es, unsigned long long* count, hipStream_t st) {
    if (t.n_rows == 0 || R == 0 || !t.cls) return hipSuccess;
    const uint64_t spans = ((uint64_t)R * max_es + TW_PREFIX_SPAN - 1) / TW_PREFIX_SPAN;
    hipLaunchKernelGGL(tw_prefix_audit, dim3(t.n_rows, (uint32_t)(spans ? spans : 1)), dim3(256), 0, st, t, R, count);
    return hipGetLastError();
}

}  // namespace tw
