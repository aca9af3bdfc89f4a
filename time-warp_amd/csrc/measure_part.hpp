// measure_part.hpp — what tw_measure's partition path (measure.hip: replicas
// with more matching records than one workgroup's LDS sorts) computes the same
// way on the host and on the device, free of HIP: the id mixer, the number of
// buckets of a replica, the bucket and the table slot of an id, the limits.
// Kept apart so that it is tested as a stand-alone host program
// (tests/measure_part_main.cpp, run under ASan / UBSan).
//
// A large replica's keys are split by the top bits of mix(id) into
// buckets(m) HBM buckets of MP_BUCKET_KEYS keys in the mean; one workgroup
// then aggregates a bucket in an open-addressed LDS table of MP_SLOTS slots,
// addressed by the low bits of the same mix.  The mixer is a bijection, so
// distinct ids never collide as wholes: a bucket overflows its table only when
// more than MP_SLOTS distinct ids share their top bits, which well-spread
// mixes do not do (the test pins the id families the scenarios produce).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MP_HD __host__ __device__
#else
#define MP_HD
#endif

namespace tw {

constexpr uint32_t MP_LDS_KEYS = 2048;         // TW_MEASURE_MAX_KEYS: at most this many keys go through the LDS sort
constexpr uint32_t MP_MAX_KEYS = 4194304;      // TW_MEASURE_MAX_KEYS_LARGE
constexpr uint32_t MP_BUCKET_KEYS = 1024;      // mean keys per bucket
constexpr uint32_t MP_SLOTS = 2048;            // distinct ids one bucket's table holds (plus the empty mark's own slot)
constexpr uint32_t MP_MAX_LOG2B = 12;          // at most 4096 buckets per replica
constexpr int64_t MP_EMPTY = INT64_MIN;        // the table's empty mark; the id of that value has a slot of its own
static_assert((uint64_t)MP_MAX_KEYS == ((uint64_t)MP_BUCKET_KEYS << MP_MAX_LOG2B), "4096 buckets of 1024 keys");
static_assert((MP_SLOTS & (MP_SLOTS - 1)) == 0, "slots are addressed by masking");

// the splitmix64 finalizer: xor-shifts and odd multiplications, each a bijection
MP_HD inline uint64_t mp_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// its inverse (the multipliers' inverses modulo 2^64)
MP_HD inline uint64_t mp_unmix(uint64_t x) {
    x ^= (x >> 31) ^ (x >> 62);
    x *= 0x319642B2D24D8EC3ull;
    x ^= (x >> 27) ^ (x >> 54);
    x *= 0x96DE1B173F119089ull;
    x ^= (x >> 30) ^ (x >> 60);
    return x;
}

// log2 of buckets(m): the next power of two >= ceil(m / bucket_keys), at most
// 2^MP_MAX_LOG2B (bucket_keys >= 1; it is MP_BUCKET_KEYS but under the testing hook)
MP_HD inline uint32_t mp_log2_buckets(uint32_t m, uint32_t bucket_keys) {
    const uint64_t need = ((uint64_t)m + bucket_keys - 1) / bucket_keys;
    uint32_t l = 0;
    while (l < MP_MAX_LOG2B && ((uint64_t)1 << l) < need) ++l;
    return l;
}
MP_HD inline uint32_t mp_buckets(uint32_t m, uint32_t bucket_keys = MP_BUCKET_KEYS) {
    return 1u << mp_log2_buckets(m, bucket_keys);
}

// bucket of an id among 2^log2b: the top bits of its mix
MP_HD inline uint32_t mp_bucket_of(int64_t id, uint32_t log2b) {
    return log2b ? (uint32_t)(mp_mix((uint64_t)id) >> (64 - log2b)) : 0u;
}
// where an id's probe sequence starts in a bucket's table: the low bits
MP_HD inline uint32_t mp_slot_of(int64_t id) { return (uint32_t)mp_mix((uint64_t)id) & (MP_SLOTS - 1); }

// device scratch of one tw_measure call on one shard beyond the LDS path's
// (include/timewarp.h states it): 16 B per key of the large replicas, 24 B per
// bucket, 28 B per replica of the shard, a 64-byte header
inline uint64_t mp_scratch_bytes(uint64_t keys, uint64_t buckets, uint64_t replicas) {
    return 64 + 28 * replicas + 24 * buckets + 16 * keys;
}

}  // namespace tw
