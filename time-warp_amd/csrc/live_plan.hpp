// live_plan.hpp — the host logic of tw_set_live_delays that needs no device:
// the argument checks and the per-link descriptor the event kernels read at a
// SEND.  Kept free of HIP so it compiles into a plain host program
// (tests/live_plan_main.cpp, run under ASan / UBSan), like load_plan.hpp.
//
// The semantics are the oracle's link_entry (oracle/timedt_oracle.cpp): a link
// of kind 1 delays by lo, a link of kind 2 by lo + (next - 1) mod k with
// k = hi - lo + 1 after a reversed range was swapped (randomR), one `next` of
// the replica's generator; kind 0 stays with the link table.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/timewarp.h"

namespace tw {

// What a SEND loads for its link: 16 bytes, one quad.
//   kind  0 table, 1 constant, 2 drawn
//   lo    the delay of kind 1, the range's lower end of kind 2 (<= 0x7FFFFFFF)
//   k     kind 2: the range size, 1 .. LIVE_K_MAX (else 1)
//   m     kind 2: floor(2^32 / k), capped at 2^32 - 1 (k = 1): live_mod's reciprocal
struct LiveLink {
    uint32_t kind, lo, k, m;
};

// randomR draws one StdGen digit while k * 1000 <= 2147483562 (the bound
// tw_draw_link_table enforces): k <= 2147483.
constexpr int64_t LIVE_DIGIT = 2147483562;
constexpr int64_t LIVE_K_MAX = LIVE_DIGIT / 1000;
// the largest argument of the modulo: next - 1 with next in [1, 2147483562]
constexpr uint32_t LIVE_X_MAX = 2147483561u;

inline uint32_t live_recip(uint32_t k) {
    const uint64_t m = (1ull << 32) / k;
    return m > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)m;
}

// x mod k without a division, for k >= 1 and any 32-bit x, m = live_recip(k).
// With m = floor(2^32 / k) (k = 1: 2^32 - 1) the estimate q = floor(x * m /
// 2^32) is never above floor(x / k), and x / k - x * m / 2^32 =
// x * (2^32 / k - m) / 2^32 < x / 2^32 < 1 (k = 1: = x / 2^32 < 1), so it is
// at most one below: x - q * k lies in [0, 2k) and one conditional
// subtraction finishes.  (2k - 1 < 2^32: no wrap.)  The device computes the
// same with __umulhi (engine_dev.hpp, wave.hip); tests/live_plan_main.cpp
// checks it for every k the plan admits.
#if defined(__HIPCC__)
__host__ __device__ __forceinline__
#else
inline
#endif
uint32_t live_mod(uint32_t x, uint32_t k, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t q = __umulhi(x, m);
#else
    const uint32_t q = (uint32_t)(((uint64_t)x * m) >> 32);
#endif
    const uint32_t r = x - q * k;
    return r >= k ? r - k : r;
}

// TW_OK and desc[n_links], or TW_ERR_INVALID: a null spec or array, a kind
// above 2, a constant delay or a range end outside [0, 0x7FFFFFFF], a range
// that needs more than one draw.  A link of kind 0 is not looked at further.
inline int live_plan(const tw_live_delays* spec, uint32_t n_links, std::vector<LiveLink>& desc) {
    desc.clear();
    if (!spec || !spec->kind || !spec->lo || !spec->hi) return TW_ERR_INVALID;
    std::vector<LiveLink> out(n_links, LiveLink{0u, 0u, 1u, 0xFFFFFFFFu});
    for (uint32_t l = 0; l < n_links; ++l) {
        const uint32_t kind = spec->kind[l];
        if (kind > 2) return TW_ERR_INVALID;
        if (kind == 0) continue;
        int64_t lo = spec->lo[l], hi = spec->hi[l];
        if (kind == 1) {
            if (lo < 0 || lo > 0x7FFFFFFF) return TW_ERR_INVALID;
            out[l] = LiveLink{1u, (uint32_t)lo, 1u, 0xFFFFFFFFu};
            continue;
        }
        if (lo > hi) std::swap(lo, hi);  // randomR swaps a reversed range
        if (lo < 0 || hi > 0x7FFFFFFF) return TW_ERR_INVALID;
        const int64_t k = hi - lo + 1;
        if (k * 1000 > LIVE_DIGIT) return TW_ERR_INVALID;
        out[l] = LiveLink{2u, (uint32_t)lo, (uint32_t)k, live_recip((uint32_t)k)};
    }
    desc.swap(out);
    return TW_OK;
}

// kind-2 links of a plan (a context with none never steps a generator)
inline uint32_t live_drawn_links(const std::vector<LiveLink>& desc) {
    uint32_t n = 0;
    for (const LiveLink& d : desc) n += d.kind == 2 ? 1u : 0u;
    return n;
}

}  // namespace tw
