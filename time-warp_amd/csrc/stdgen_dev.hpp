// stdgen_dev.hpp — random-1.1's StdGen on the device, shared by the link-table
// draw (tables.hip) and the live delays of the event kernels (engine_dev.hpp,
// wave.hip; tw_set_live_delays).
//
// random-1.1 is an un-vendored dependency of the reference (lts-7.9); this is
// its published algorithm (restated on the host in
// timewarp/stdgen.py):
//   mkStdGen s : s' = s .&. 0x7fffffff (s taken as Int32); (q, s1) = s' divMod
//                2147483562; s2 = q mod 2147483398; StdGen (s1+1) (s2+1)
//   next       : L'Ecuyer's combined MLCG (Schrage steps), z in [1, 2147483562]
//   randomR    : for ranges k <= 2147483, one `next`: lo + (z - 1) mod k
// Every intermediate fits in 32 bits: 40014 * (s1 mod 53668) <= 2,147,431,938
// and 40692 * (s2 mod 52774) <= 2,147,438,916, both below 2^31.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tw {

struct Gen {
    int32_t s1, s2;
};

__device__ __forceinline__ Gen mk_stdgen(int64_t seed) {
    const int32_t s = (int32_t)(uint32_t)(uint64_t)seed & 0x7FFFFFFF;
    return Gen{s % 2147483562 + 1, (s / 2147483562) % 2147483398 + 1};
}

__device__ __forceinline__ uint32_t next(Gen& g) {
    const int32_t k = g.s1 / 53668;
    int32_t s1 = 40014 * (g.s1 - k * 53668) - k * 12211;
    s1 += s1 < 0 ? 2147483563 : 0;
    const int32_t k2 = g.s2 / 52774;
    int32_t s2 = 40692 * (g.s2 - k2 * 52774) - k2 * 3791;
    s2 += s2 < 0 ? 2147483399 : 0;
    g.s1 = s1;
    g.s2 = s2;
    const int32_t z = s1 - s2;
    return (uint32_t)(z < 1 ? z + 2147483562 : z);
}

}  // namespace tw
