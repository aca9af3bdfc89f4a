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
    // Rows an apply may leave unstored (§3o); all null: every row is stored.
    // tag[row]: the claimed slot whose quad 1 - 3 the row is, else PCL_NO_SLOT.
    // Such a row is skipped when cflags[CF_VALID] is set and dirty[slot] is 0.
    const uint32_t* tag;
    const uint8_t* dirty;   // [S]
    const uint32_t* cflags; // [CF_COUNT]
};

#define TW_PREFIX_SPAN 65536u  // bytes of a row one workgroup of tw_prefix_apply stores

// The directory of replica 0's parked state from its scalar block (sc:
// SC_COUNT words): every array element a later launch can read before writing
// it.  near_cap: entries of the near spill per replica.  False when a scalar
// is out of its array's range (nothing is taken then).  bytes: the snapshot's
// size = bytes written per replica.
bool prefix_directory(const Dev& d, const uint64_t* sc, uint32_t near_cap, std::vector<PrefixRow>& rows, size_t& bytes);
// snapshot[off .. off + es) = replica 0's element, for every row
hipError_t prefix_take(const PrefixTab& t, hipStream_t st);
// every row's value to all R replicas (store-only), but the rows t.tag lets it skip
hipError_t prefix_apply(const PrefixTab& t, uint32_t R, uint32_t max_es, hipStream_t st);
// the testing hook's check of an apply that could skip rows (read-only): every
// element of every skipped row against the snapshot's value; *count += the
// elements that differ
hipError_t prefix_audit(const PrefixTab& t, uint32_t R, uint32_t max_es, unsigned long long* count, hipStream_t st);
// the layout clean_build and clean_tags take (prefix_clean.hpp), from Dev
CleanLayout clean_layout(const Dev& d);

}  // namespace tw
