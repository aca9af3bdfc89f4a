// Stand-alone host program over csrc/lp_run_plan.hpp (no HIP): built with
// ASan + UBSan by tests/test_lp_run_host.py.  Every check prints its name on
// failure and the program exits non-zero; "ok <n>" on success.
#include <climits>
#include <cstdio>
#include <vector>

#include "../time-warp_amd/csrc/lp_run_plan.hpp"

using namespace tw;

static int failures = 0;
static long checks = 0;
#define CHECK(x)                                            \
    do {                                                    \
        ++checks;                                           \
        if (!(x)) {                                         \
            ++failures;                                     \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
        }                                                   \
    } while (0)

// The block-size rule as tw_lp_run had it inline before lp_next_block
// existed: the reference of the grid below.  Kept statement for statement
// (`dem`, `stride` and `cap_eff` were the loop's locals); do not tidy it.
static uint32_t ref_next_block(int64_t dem, uint32_t stride, uint32_t cap_eff) {
    uint32_t want = 64;
    while (want < (uint64_t)dem + (uint64_t)dem / 4 && want < stride) want <<= 1;
    want = std::min(want, stride);
    if (want > cap_eff || want * 4 <= cap_eff) cap_eff = want;
    return cap_eff;
}

static std::vector<uint32_t> even(uint32_t begin, uint32_t count, uint32_t world) {
    std::vector<uint32_t> s;
    lp_starts_even(begin, count, world, s);
    return s;
}

int main() {
    // ---- block sizes: the whole grid against the reference
    {
        std::vector<int64_t> demands;
        for (int64_t d = 0; d <= 70000; ++d) demands.push_back(d);
        demands.push_back(-1);
        demands.push_back(INT64_MAX);
        demands.push_back(INT64_MIN);
        long mismatches = 0, cases = 0;
        for (uint32_t stride : {1u, 8u, 63u, 64u, 65u, 4096u, 16384u, 1u << 22}) {
            std::vector<uint32_t> caps;  // every power of two <= stride, and stride itself
            for (uint32_t p = 1; p <= stride; p <<= 1) caps.push_back(p);
            if (caps.back() != stride) caps.push_back(stride);
            for (uint32_t cap : caps)
                for (int64_t d : demands) {
                    ++cases;
                    if (lp_next_block(d, stride, cap) != ref_next_block(d, stride, cap)) {
                        if (mismatches++ < 10)
                            printf("FAIL next_block(%lld, %u, %u)\n", (long long)d, (unsigned)stride, (unsigned)cap);
                    }
                }
        }
        CHECK(mismatches == 0);
        CHECK(cases == 70004l * (1 + 4 + 7 + 7 + 8 + 13 + 15 + 23));
    }
    // ---- ... and the cases that follow from the rule
    CHECK(lp_first_block(8) == 8 && lp_first_block(16384) == 4096 && lp_first_block(4096) == 4096 &&
          lp_first_block(4097) == 4096 && lp_first_block(1) == 1 && lp_first_block(1u << 22) == 4096);
    for (int64_t d : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)8, (int64_t)9, (int64_t)100, (int64_t)70000,
                      (int64_t)-1, INT64_MAX, INT64_MIN})
        CHECK(lp_next_block(d, 8, lp_first_block(8)) == 8);  // want starts at 64 and is clamped to the stride
    CHECK(lp_next_block(100, 16384, lp_first_block(16384)) == 128);  // 64 < 125 <= 128; 128 * 4 <= 4096
    CHECK(lp_next_block(1000, 16384, 4096) == 4096);  // want 2048: neither larger nor at most a quarter
    CHECK(lp_next_block(3000, 16384, 4096) == 4096);  // want 4096
    CHECK(lp_next_block(5000, 16384, 4096) == 8192);
    for (uint32_t cap : {1u, 64u, 128u, 4096u, 8192u, 16384u}) CHECK(lp_next_block(20000, 16384, cap) == 16384);
    CHECK(lp_next_block(0, 16384, 4096) == 64 && lp_next_block(0, 16384, 128) == 128 &&
          lp_next_block(0, 16384, 256) == 64);
    CHECK(lp_next_block(-1, 16384, 64) == 16384 && lp_next_block(INT64_MIN, 1u << 22, 64) == 1u << 22 &&
          lp_next_block(INT64_MAX, 4096, 64) == 4096);
    // ---- a block's bytes: a 32-byte header and 32 bytes per record
    CHECK(lp_block_bytes(0) == 32 && lp_block_bytes(8) == 288 && lp_block_bytes(4096) == 32ull * 4097 &&
          lp_block_bytes(16384) == 32ull * 16385 && lp_block_bytes(1u << 22) == 32ull * ((1ull << 22) + 1));
    CHECK(lp_block_bytes(UINT32_MAX) == 32ull * (1ull << 32));  // (no 32-bit wrap)

    // ---- boundaries: the even split
    CHECK((even(3, 10, 1) == std::vector<uint32_t>{3, 13}));
    CHECK((even(3, 10, 3) == std::vector<uint32_t>{3, 7, 10, 13}));  // 4 + 3 + 3
    CHECK((even(3, 10, 4) == std::vector<uint32_t>{3, 6, 9, 11, 13}));  // 3 + 3 + 2 + 2
    CHECK((even(3, 10, 12) == std::vector<uint32_t>{3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 13, 13}));  // two empty blocks
    CHECK((even(0, 0, 2) == std::vector<uint32_t>{0, 0, 0}));
    for (uint32_t world : {1u, 3u, 4u, 12u}) {  // the boundaries are split()'s blocks, end to end
        const std::vector<uint32_t> s = even(3, 10, world);
        CHECK(s.size() == world + 1);
        for (uint32_t g = 0; g < world; ++g) {
            uint32_t b0, nb;
            split(10, world, g, b0, nb);
            CHECK(s[g] == 3 + b0 && s[g + 1] == 3 + b0 + nb);
        }
    }
    // ---- ... and from gathered (begin, count) pairs
    {
        std::vector<uint32_t> s;
        const uint32_t ok[6] = {3, 4, 7, 3, 10, 3};
        CHECK(lp_starts_gathered(ok, 3, s) && (s == std::vector<uint32_t>{3, 7, 10, 13}));
        CHECK(lp_starts_gathered(ok, 1, s) && (s == std::vector<uint32_t>{3, 7}));
        const uint32_t gap[6] = {3, 4, 8, 2, 10, 3};
        CHECK(!lp_starts_gathered(gap, 3, s));
        const uint32_t overlap[6] = {3, 4, 6, 4, 10, 3};
        CHECK(!lp_starts_gathered(overlap, 3, s));
        const uint32_t late_gap[6] = {3, 4, 7, 3, 11, 2};
        CHECK(!lp_starts_gathered(late_gap, 3, s));
        const uint32_t empty_mid[6] = {3, 4, 7, 0, 7, 6};
        CHECK(lp_starts_gathered(empty_mid, 3, s) && (s == std::vector<uint32_t>{3, 7, 7, 13}));
        const uint32_t unordered[4] = {7, 3, 3, 4};  // contiguous as a set, not in rank order
        CHECK(!lp_starts_gathered(unordered, 2, s));
    }

    // ---- the severity table
    {
        const int all[] = {TW_OK, TW_ERR_INVALID, TW_ERR_NO_DEVICE, TW_ERR_HIP, TW_ERR_OOM, TW_ERR_STATE,
                           TW_ERR_REPLICA, TW_ERR_INCOMPLETE, TW_ERR_COMM};
        for (int rc : all) CHECK(rc_of_sev(sev_of(rc)) == rc);
        // the order of the table's comment: a replica error or an incomplete
        // run below every hard failure, whatever the numeric values
        const int order[] = {TW_OK, TW_ERR_REPLICA, TW_ERR_INCOMPLETE, TW_ERR_INVALID, TW_ERR_STATE, TW_ERR_COMM,
                             TW_ERR_OOM, TW_ERR_HIP, TW_ERR_NO_DEVICE};
        for (int i = 0; i < 9; ++i) CHECK(sev_of(order[i]) == i);
        for (int rc : all) CHECK(sev_of(-99) >= sev_of(rc) && sev_of(1) >= sev_of(rc));  // unknown: the worst
        CHECK(rc_of_sev(sev_of(-99)) == TW_ERR_NO_DEVICE);
        CHECK(rc_of_sev(-1) == TW_ERR_HIP && rc_of_sev(9) == TW_ERR_HIP && rc_of_sev(INT64_MAX) == TW_ERR_HIP);
        CHECK(worst_of({}) == TW_OK);
        CHECK(worst_of({TW_OK}) == TW_OK && worst_of({TW_OK, TW_OK, TW_OK}) == TW_OK);
        CHECK(worst_of({TW_OK, TW_ERR_STATE, TW_OK}) == TW_ERR_STATE);
        CHECK(worst_of({TW_ERR_REPLICA, TW_ERR_HIP}) == TW_ERR_HIP && worst_of({TW_ERR_HIP, TW_ERR_REPLICA}) == TW_ERR_HIP);
        CHECK(worst_of({TW_ERR_INVALID, TW_ERR_INCOMPLETE}) == TW_ERR_INVALID &&
              worst_of({TW_ERR_INCOMPLETE, TW_ERR_INVALID}) == TW_ERR_INVALID);  // -1 outranks -7
        CHECK(worst_of({-99, -98}) == -99);  // equally bad: the first
    }

    // ---- TW_LP_XCAP: 1 .. 2^22, else what the context had
    {
        const uint32_t d = LP_XCAP_DEFAULT;
        CHECK(d == 1u << 14);
        CHECK(lp_parse_xcap(nullptr, d) == d && lp_parse_xcap("", d) == d && lp_parse_xcap("abc", d) == d);
        CHECK(lp_parse_xcap("8", d) == 8 && lp_parse_xcap("1", d) == 1 && lp_parse_xcap("4194304", d) == 1u << 22);
        CHECK(lp_parse_xcap("0", d) == d && lp_parse_xcap("-3", d) == d && lp_parse_xcap("4194305", d) == d);
        CHECK(lp_parse_xcap("99999999999999999999999", d) == d && lp_parse_xcap("-99999999999999999999999", d) == d);
        CHECK(lp_parse_xcap(" 16", d) == 16 && lp_parse_xcap("8x", d) == 8);  // strtol's reading, as before
        CHECK(lp_parse_xcap("junk", 8) == 8 && lp_parse_xcap("32", 8) == 32);  // an earlier set-up's value stays
    }
    // ---- TW_TEST_FAIL_TICK=shard:tick
    {
        LpFailAt f = lp_parse_fail_tick(nullptr);
        CHECK(f.shard == -1 && f.tick == -1 && !f.hit(0, 0));
        f = lp_parse_fail_tick("1:5");
        CHECK(f.shard == 1 && f.tick == 5 && f.hit(1, 5) && !f.hit(0, 5) && !f.hit(1, 4) && !f.hit(1, 6));
        f = lp_parse_fail_tick("0:0");
        CHECK(f.hit(0, 0) && !f.hit(0, 1));
        f = lp_parse_fail_tick("3");  // no colon: no tick
        CHECK(f.shard == 3 && f.tick == -1);
        f = lp_parse_fail_tick("");
        CHECK(f.shard == 0 && f.tick == -1);
        f = lp_parse_fail_tick("garbage");
        CHECK(f.shard == 0 && f.tick == -1);
        f = lp_parse_fail_tick("2;7");
        CHECK(f.shard == 2 && f.tick == -1);
        f = lp_parse_fail_tick("2:x");  // strtol's reading, as before
        CHECK(f.shard == 2 && f.tick == 0);
        f = lp_parse_fail_tick("-1:5");
        CHECK(f.shard == -1 && f.tick == 5);
        for (const char* s : {"3", "", "garbage", "2;7", "-1:5", "0:-1"}) {  // none of these ever fires
            f = lp_parse_fail_tick(s);
            for (size_t i = 0; i < 4; ++i)
                for (uint64_t t : {(uint64_t)0, (uint64_t)1, (uint64_t)5, (uint64_t)1 << 40}) CHECK(!f.hit(i, t));
        }
    }

    if (failures) {
        printf("%d of %ld checks failed\n", failures, checks);
        return 1;
    }
    printf("ok %ld\n", checks);
    return 0;
}
