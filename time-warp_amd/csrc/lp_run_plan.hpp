// lp_run_plan.hpp — the host arithmetic of tw_lp_run (abi.hip)
// that needs no HIP and no RCCL:
//   * the severity table on which every job-wide agreement rests (status codes
//     ranked for a MAX reduction) and the worst of a set of local codes;
//   * the node boundaries of every rank: the even split (also tw_load's and
//     tw_lp_load's sharding) and the boundaries from all-gathered
//     (begin, count) pairs, which must be contiguous;
//   * the exchange's block sizes: the first block, the next one from the
//     largest per-tick demand, and a block's bytes;
//   * the two environment hooks of the loop as functions of a string.
// Kept free of HIP so it compiles into a plain host program
// (tests/lp_run_plan_main.cpp, run under ASan / UBSan).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/timewarp.h"

namespace tw {

// Status codes ranked by severity for the job-wide reduction (MAX): a hard
// runtime, communicator or state failure on one shard outranks a replica
// error or an incomplete run on another, whatever their numeric values
inline int64_t sev_of(int rc) {
    switch (rc) {
    case TW_OK: return 0;
    case TW_ERR_REPLICA: return 1;
    case TW_ERR_INCOMPLETE: return 2;
    case TW_ERR_INVALID: return 3;
    case TW_ERR_STATE: return 4;
    case TW_ERR_COMM: return 5;
    case TW_ERR_OOM: return 6;
    case TW_ERR_HIP: return 7;
    default: return 8;  // TW_ERR_NO_DEVICE and anything unknown
    }
}
inline int rc_of_sev(int64_t s) {
    static const int rcs[] = {TW_OK, TW_ERR_REPLICA, TW_ERR_INCOMPLETE, TW_ERR_INVALID, TW_ERR_STATE,
                              TW_ERR_COMM, TW_ERR_OOM, TW_ERR_HIP, TW_ERR_NO_DEVICE};
    return s >= 0 && s <= 8 ? rcs[s] : TW_ERR_HIP;
}
// the worst of these local codes (of equally bad ones the first)
inline int worst_of(const std::vector<int>& local) {
    int w = TW_OK;
    for (int r : local)
        if (sev_of(r) > sev_of(w)) w = r;
    return w;
}

// part i of `total` items cut into `parts` contiguous blocks whose sizes
// differ by at most one (the larger ones first): [b0, b0 + nb)
inline void split(uint32_t total, uint32_t parts, uint32_t i, uint32_t& b0, uint32_t& nb) {
    const uint32_t base = total / parts, rem = total % parts;
    b0 = i * base + std::min(i, rem);
    nb = base + (i < rem ? 1u : 0u);
}

// world + 1 node boundaries of nodes [lp_begin, lp_begin + lp_count) split
// evenly over the ranks (a world larger than lp_count leaves empty blocks)
inline void lp_starts_even(uint32_t lp_begin, uint32_t lp_count, uint32_t world, std::vector<uint32_t>& starts) {
    starts.assign((size_t)world + 1, 0);
    for (uint32_t g = 0; g < world; ++g) {
        uint32_t b0, nb;
        split(lp_count, world, g, b0, nb);
        starts[g] = lp_begin + b0;
    }
    starts[world] = lp_begin + lp_count;
}

// ... from the ranks' own (begin, count) pairs, pairs[2g] and pairs[2g + 1]
// (world >= 1).  false when a rank does not begin where the one before it
// ends: a gap or an overlap.  An empty rank in between is contiguous.
inline bool lp_starts_gathered(const uint32_t* pairs, uint32_t world, std::vector<uint32_t>& starts) {
    starts.assign((size_t)world + 1, 0);
    for (uint32_t g = 0; g < world; ++g) {
        starts[g] = pairs[2 * g];
        if (g > 0 && pairs[2 * g] != pairs[2 * (g - 1)] + pairs[2 * (g - 1) + 1]) return false;
    }
    starts[world] = pairs[2 * (world - 1)] + pairs[2 * (world - 1) + 1];
    return true;
}

// The exchange keeps `stride` records per rank pair, of which the first
// cap_eff travel each tick.  The first block of a run:
inline uint32_t lp_first_block(uint32_t stride) { return std::min<uint32_t>(stride, 4096u); }

// The next 16 ticks' block from the largest demand any rank had in one tick:
// the power of two from 64 up that holds demand + 25 %, at most the stride;
// taken only when it is larger than the present block or at most a quarter of
// it, so the size does not flap.  (A negative demand reads as a huge one: the
// stride.)
inline uint32_t lp_next_block(int64_t demand, uint32_t stride, uint32_t cap_eff) {
    uint32_t want = 64;
    while (want < (uint64_t)demand + (uint64_t)demand / 4 && want < stride) want <<= 1;
    want = std::min(want, stride);
    if (want > cap_eff || want * 4 <= cap_eff) cap_eff = want;
    return cap_eff;
}

// bytes of a block of `records` records behind its header, 32 B each: the
// distance between two ranks' blocks (records = stride) and what travels
// (records = cap_eff)
inline size_t lp_block_bytes(uint32_t records) { return 32ull * ((size_t)records + 1); }

// TW_LP_XCAP: the exchange's stride, 1 .. 2^22 records; anything else (no
// string, an empty one, garbage, out of range) is ignored and leaves `keep`
constexpr uint32_t LP_XCAP_DEFAULT = 1u << 14;
inline uint32_t lp_parse_xcap(const char* s, uint32_t keep) {
    if (!s) return keep;
    const long v = strtol(s, nullptr, 10);
    return v >= 1 && v <= (1 << 22) ? (uint32_t)v : keep;
}

// TW_TEST_FAIL_TICK=shard:tick; without the colon no tick ever matches
struct LpFailAt {
    long shard = -1, tick = -1;
    bool hit(size_t i, uint64_t t) const { return (long)i == shard && (long)t == tick; }
};
inline LpFailAt lp_parse_fail_tick(const char* s) {
    LpFailAt f;
    if (!s) return f;
    char* e = nullptr;
    f.shard = strtol(s, &e, 10);
    f.tick = (e && *e == ':') ? strtol(e + 1, nullptr, 10) : -1;
    return f;
}

}  // namespace tw
