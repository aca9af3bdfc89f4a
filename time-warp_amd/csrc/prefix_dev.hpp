// prefix_dev.hpp — what engine.hip and prefix.hip share of the send-free
// prefix: the row directory of a parked replica's live state and
// the two kernels over it, with tables passed as a kernel argument of their
// own (Dev, the event kernels' argument, is unchanged).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "tw_dev.hpp"
#include "prefix_clean.hpp"

namespace tw {

struct PrefixTab {
    const PrefixRow* rows;  // device copy of the directory (PrefixRow: prefix_clean.hpp)
    uint8_t* snap;          // the snapshot: every row's value of the pilot replica
    uint32_t n_rows;
    // Rows an apply may leave unstored (§3o, §3v); cls null: every row is stored.
    // cls[row]: the row's class (prefix_clean.hpp RC_*), tag[row]: the claimed
    // slot whose dirty byte speaks for a row of RC_BODY, RC_HDR or RC_RUN.  Such
    // a row is skipped when its flag word is set -- CF_HDR_OK for RC_HDR, else
    // CF_VALID -- and dirty[slot] is 0 (dirty null: none of them is skipped).
    // An RC_RESET row is skipped when `reset` is set: the apply is the first
    // device work behind a tw_reset.
    const uint8_t* cls;
    const uint32_t* tag;
    const uint8_t* dirty;   // [S]
    const uint32_t* cflags; // [CF_COUNT]
    uint32_t reset;
    // The compact form's list (§3v; list null: the early-exit form): the
    // (row, span) pairs an apply stores, at most list_cap, and their count.
    uint2* list;
    uint32_t* list_n;
    uint32_t list_cap;
};

#define TW_PREFIX_SPAN 65536u  // bytes of a row one workgroup of tw_prefix_apply stores

// the workgroups that store a row of R elements of `es` bytes from address dst:
// one per span of its 16-byte-aligned body, at least one (the edges are the first's)
__host__ __device__ __forceinline__ uint32_t prefix_row_spans(uint64_t dst, uint32_t es, uint32_t R) {
    const uint64_t len = (uint64_t)R * es;
    const uint64_t mis = (16u - (uint32_t)(dst & 15u)) & 15u;
    const uint64_t head = mis < len ? mis : len;
    const uint64_t n = (((len - head) & ~15ull) + TW_PREFIX_SPAN - 1) / TW_PREFIX_SPAN;
    return n ? (uint32_t)n : 1u;
}

// The directory of replica 0's parked state from its scalar block (sc:
// SC_COUNT words): every array element a later launch can read before writing
// it.  near_cap: entries of the near spill per replica.  False when a scalar
// is out of its array's range (nothing is taken then).  bytes: the snapshot's
// size = bytes written per replica.
bool prefix_directory(const Dev& d, const uint64_t* sc, uint32_t near_cap, std::vector<PrefixRow>& rows, size_t& bytes);
// snapshot[off .. off + es) = replica 0's element, for every row
hipError_t prefix_take(const PrefixTab& t, hipStream_t st);
// every row's value to all R replicas (store-only), but the rows t.cls lets it
// skip.  With t.list and t.cls: the compact form, over `pairs` workgroups (the
// host's count of the pairs the list will hold; any value stores every pair).
hipError_t prefix_apply(const PrefixTab& t, uint32_t R, uint32_t max_es, uint32_t pairs, hipStream_t st);
// the testing hook's check of an apply that could skip rows (read-only): every
// element of every skipped row against the snapshot's value; count[0] += the
// elements that differ, count[RC_*] += the skipped rows of that class
// (count: RC_COUNT words)
hipError_t prefix_audit(const PrefixTab& t, uint32_t R, uint32_t max_es, unsigned long long* count, hipStream_t st);
// the layout clean_build and clean_tags take (prefix_clean.hpp), from Dev
CleanLayout clean_layout(const Dev& d);

}  // namespace tw
