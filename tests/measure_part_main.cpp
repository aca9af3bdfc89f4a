// Stand-alone host program over csrc/measure_part.hpp (no HIP): the id mixer,
// the bucket count and the bucket of an id as tw_measure's partition path
// computes them.  Built and run by tests/test_measure_part_host.py with
// -fsanitize=address,undefined.  Prints the fullest bucket of every id family.
#include <cstdio>
#include <vector>

#include "../include/timewarp.h"
#include "../time-warp_amd/csrc/measure_part.hpp"

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            return 1;                                         \
        }                                                     \
    } while (0)

// the most distinct ids any of buckets(m) buckets receives from ids
// first + i * step, i < n (distinct by construction: the mixer is a bijection,
// so distinct ids stay distinct keys)
static uint32_t fullest(const char* name, int64_t first, int64_t step, uint32_t n, uint32_t m) {
    const uint32_t l = tw::mp_log2_buckets(m, tw::MP_BUCKET_KEYS);
    std::vector<uint32_t> c((size_t)1 << l, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const int64_t id = (int64_t)((uint64_t)first + (uint64_t)step * i);
        const uint32_t b = tw::mp_bucket_of(id, l);
        if (b >= c.size()) return UINT32_MAX;
        ++c[b];
    }
    uint32_t mx = 0;
    for (uint32_t v : c) mx = v > mx ? v : mx;
    printf("%s: %u ids over %zu buckets, fullest %u of %u slots\n", name, n, c.size(), mx, tw::MP_SLOTS);
    return mx;
}

int main() {
    using namespace tw;
    static_assert(MP_LDS_KEYS == TW_MEASURE_MAX_KEYS && MP_MAX_KEYS == TW_MEASURE_MAX_KEYS_LARGE, "the header's limits");
    // buckets(m): the next power of two >= ceil(m / 1024)
    CHECK(mp_buckets(1) == 1 && mp_buckets(1024) == 1 && mp_buckets(1025) == 2);
    CHECK(mp_buckets(2048) == 2 && mp_buckets(2049) == 4);
    for (uint32_t l = 1; l <= MP_MAX_LOG2B; ++l) {
        const uint32_t m = MP_BUCKET_KEYS << l;  // 2^l buckets exactly full
        CHECK(mp_buckets(m - 1) == 1u << l);
        CHECK(mp_buckets(m) == 1u << l);
        CHECK(mp_buckets(m + 1) == (l < MP_MAX_LOG2B ? 2u << l : 1u << l));  // capped at 4096
        CHECK(mp_log2_buckets(m, MP_BUCKET_KEYS) == l);
    }
    CHECK(mp_buckets(TW_MEASURE_MAX_KEYS_LARGE) == 4096);
    CHECK(mp_buckets(512000) == 512);
    // the testing hook's bucket sizes
    CHECK(mp_buckets(6010, 1u << 20) == 1 && mp_buckets(2049, 1) == 4096 && mp_buckets(30, 8) == 4);
    CHECK(mp_bucket_of(12345, 0) == 0);

    // the mixer is a bijection: forward then inverse, inverse then forward
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 200000; ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        CHECK(mp_unmix(mp_mix(x)) == x);
        CHECK(mp_mix(mp_unmix(x)) == x);
    }
    const uint64_t edge[] = {0, 1, ~0ull, (uint64_t)INT64_MIN, (uint64_t)INT64_MAX, 1ull << 40, (uint64_t)-5000ll};
    for (uint64_t e : edge) CHECK(mp_unmix(mp_mix(e)) == e && mp_mix(mp_unmix(e)) == e);
    for (int64_t id = -3000; id < 3000; ++id) {
        CHECK(mp_slot_of(id) < MP_SLOTS);
        CHECK(mp_bucket_of(id, MP_MAX_LOG2B) < 4096 && mp_bucket_of(id, 2) < 4);
    }

    // no bucket receives more distinct ids than its table has slots
    CHECK(fullest("consecutive 0..4194303", 0, 1, 4194304, 4194304) <= MP_SLOTS);
    CHECK(fullest("1..256000 at m = 512000", 1, 1, 256000, 512000) <= MP_SLOTS);
    CHECK(fullest("stride 256 from 1 << 40", (int64_t)1 << 40, 256, 2097152, 4194304) <= MP_SLOTS);
    CHECK(fullest("negative multiples of 7919", -7919, -7919, 2097152, 4194304) <= MP_SLOTS);
    CHECK(fullest("multiples of 2^20", 0, (int64_t)1 << 20, 2097152, 4194304) <= MP_SLOTS);

    CHECK(mp_scratch_bytes(0, 0, 0) == 64);
    CHECK(mp_scratch_bytes(512000, 512, 256) == 64 + 28 * 256 + 24 * 512 + 16 * 512000);
    printf("part ok\n");
    return 0;
}
