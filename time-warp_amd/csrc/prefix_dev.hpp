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

namespace tw {

// One row of a replica-minor array: R elements of `es` bytes from device
// address `dst` (replica 0's element), whose snapshot value lies `off` bytes
// into the snapshot buffer.  es is 1, 4, 8 or a multiple of 16; off is a
// multiple of es (of 16 for the wider rows).
struct PrefixRow {
    uint64_t dst;
    uint32_t off;
    uint32_t es;
};

struct PrefixTab {
    const PrefixRow* rows;  // device copy of the directory
    uint8_t* snap;          // the snapshot: every row's value of the pilot replica
    uint32_t n_rows;
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
// every row's value to all R replicas (store-only)
hipError_t prefix_apply(const PrefixTab& t, uint32_t R, uint32_t max_es, hipStream_t st);

}  // namespace tw
