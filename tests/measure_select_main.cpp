// The HIP-free half of tw_measure_quantiles (csrc/measure_select.hpp) over
// plain arrays: the argument checks, the index arithmetic, the digit select
// loop against std::nth_element / std::sort.  Built with ASan + UBSan by
// tests/test_measure_select_host.py; prints "select ok" and exits 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../time-warp_amd/csrc/measure_select.hpp"

using namespace tw;

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                              \
        }                                                         \
    } while (0)

static const uint32_t QS[] = {0, 1, 499999, 500000, 500001, 999999, 1000000};
static const uint32_t NQ = sizeof QS / sizeof QS[0];

// the values split over `shards` arrays, counted as the device pass counts them
struct Shards {
    std::vector<std::vector<int64_t>> part;
    uint32_t passes = 0;
    bool operator()(const uint64_t* prefix, uint32_t nk, uint32_t shift, uint64_t* hist) {
        ++passes;
        for (const auto& p : part) {
            std::vector<uint64_t> h((size_t)nk * QS_DIGITS, 0);  // a shard's own histogram, then summed
            for (int64_t d : p) {
                const uint64_t key = qs_key(d);
                for (uint32_t j = 0; j < nk; ++j)
                    if (qs_match(key, prefix[j], shift)) ++h[(size_t)j * QS_DIGITS + qs_digit(key, shift)];
            }
            for (size_t i = 0; i < h.size(); ++i) hist[i] += h[i];
        }
        return true;
    }
};

// every quantile of QS over `v`, selected over 1, 2 and 3 shards, against a sort
// and against nth_element; returns the passes the one-shard select took
static uint32_t check_values(const std::vector<int64_t>& v) {
    std::vector<int64_t> sorted = v;
    std::sort(sorted.begin(), sorted.end());
    uint32_t passes1 = 0;
    for (uint32_t shards = 1; shards <= 3; ++shards) {
        Shards s;
        s.part.resize(shards);
        for (size_t i = 0; i < v.size(); ++i) s.part[(i * 7 + i / 3) % shards].push_back(v[i]);
        QsRanks ranks;
        qs_ranks(QS, NQ, v.size(), &ranks);
        CHECK(ranks.n >= 1 && ranks.n <= QS_MAX_RANKS);
        int64_t val[QS_MAX_RANKS];
        uint32_t passes = 99;
        CHECK(qs_select(ranks, sorted.front(), sorted.back(), s, val, &passes));
        CHECK(passes == s.passes && passes <= 8);
        if (shards == 1) passes1 = passes;
        for (uint32_t i = 0; i < NQ; ++i) {
            uint64_t lo, hi;
            qs_index(QS[i], v.size(), &lo, &hi);
            CHECK(lo <= hi && hi < v.size() && hi - lo <= 1);
            CHECK(val[ranks.lo_at[i]] == sorted[lo]);
            CHECK(val[ranks.hi_at[i]] == sorted[hi]);
            std::vector<int64_t> w = v;
            std::nth_element(w.begin(), w.begin() + (ptrdiff_t)lo, w.end());
            CHECK(val[ranks.lo_at[i]] == w[lo]);
            std::nth_element(w.begin(), w.begin() + (ptrdiff_t)hi, w.end());
            CHECK(val[ranks.hi_at[i]] == w[hi]);
        }
        // q = 0 and 10^6 are the ends
        CHECK(val[ranks.lo_at[0]] == sorted.front() && val[ranks.hi_at[0]] == sorted.front());
        CHECK(val[ranks.lo_at[NQ - 1]] == sorted.back() && val[ranks.hi_at[NQ - 1]] == sorted.back());
    }
    return passes1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    // ---- key order and digits
    const int64_t edge[] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
    for (size_t i = 0; i + 1 < sizeof edge / sizeof edge[0]; ++i) {
        CHECK(qs_key(edge[i]) < qs_key(edge[i + 1]));
        CHECK(qs_unkey(qs_key(edge[i])) == edge[i]);
    }
    CHECK(qs_key(INT64_MIN) == 0 && qs_key(INT64_MAX) == UINT64_MAX && qs_key(0) == 1ull << 63);
    CHECK(qs_digit(0x0123456789ABCDEFull, 56) == 0x01 && qs_digit(0x0123456789ABCDEFull, 0) == 0xEF);
    CHECK(qs_match(0x0123456789ABCDEFull, 0, 56) && qs_match(0x0123456789ABCDEFull, 0x0123450000000000ull, 32));
    CHECK(!qs_match(0x0123456789ABCDEFull, 0x0123460000000000ull, 32) && qs_match(0x0123456789ABCDEFull, 0x0123456789ABCD00ull, 0));

    // ---- the common-prefix start
    uint64_t p = 1;
    CHECK(qs_start(5, 5, &p) == 0 && p == qs_key(5));                      // all equal: nothing to fix
    CHECK(qs_start(INT64_MIN, INT64_MAX, &p) == 8 && p == 0);              // nothing shared
    CHECK(qs_start(-1, 0, &p) == 8 && p == 0);                             // the sign digit differs
    CHECK(qs_start(2000, 9000, &p) == 2 && p == (1ull << 63));             // real latencies: two passes
    CHECK(qs_start(0x10000, 0x1FFFF, &p) == 2 && p == ((1ull << 63) | 0x10000));
    CHECK(qs_start(70000, 70001, &p) == 1 && p == ((1ull << 63) | (70000 & ~0xFFull)));

    // ---- the index arithmetic against 128 bits, up to the largest n
    const uint64_t ns[] = {1, 2, 3, 4, 5, 999999, 1000000, 1000001, 1000002, 1ull << 21, (1ull << 32) + 7,
                           1ull << 53, UINT64_MAX - 1, UINT64_MAX};
    for (uint64_t n : ns)
        for (uint32_t q : QS) {
            const unsigned __int128 pos = (unsigned __int128)q * (n - 1);
            uint64_t lo, hi;
            qs_index(q, n, &lo, &hi);
            CHECK(lo == (uint64_t)(pos / 1000000u));
            CHECK(hi == lo + (pos % 1000000u != 0 ? 1 : 0));
            CHECK(hi <= n - 1);
        }
    uint64_t lo, hi;
    qs_index(500000, 4, &lo, &hi);
    CHECK(lo == 1 && hi == 2);  // even n: the two middle values
    qs_index(500000, 5, &lo, &hi);
    CHECK(lo == 2 && hi == 2);  // odd n: the middle one
    qs_index(1000000, UINT64_MAX, &lo, &hi);
    CHECK(lo == UINT64_MAX - 1 && hi == UINT64_MAX - 1);

    // ---- the digit step
    uint32_t h[QS_DIGITS] = {};
    h[3] = 2;
    h[200] = 5;
    uint64_t k = 0;
    CHECK(qs_step(h, &k) == 3 && k == 0);
    k = 1;
    CHECK(qs_step(h, &k) == 3 && k == 1);
    k = 2;
    CHECK(qs_step(h, &k) == 200 && k == 0);
    k = 6;
    CHECK(qs_step(h, &k) == 200 && k == 4);
    k = 7;
    CHECK(qs_step(h, &k) == QS_NO_DIGIT);  // beyond the counted
    k = UINT64_MAX;
    CHECK(qs_step(h, &k) == QS_NO_DIGIT);

    // ---- the select loop
    check_values({42});                                                     // n = 1
    check_values({7, -7});                                                  // two values
    check_values({INT64_MIN, INT64_MAX});
    check_values({INT64_MIN, -1, 0, INT64_MAX});                            // the full range, even n
    check_values({INT64_MIN, -1, 0, 1, INT64_MAX});                         // odd n
    CHECK(check_values(std::vector<int64_t>(37, -123456789)) == 0);         // all equal: no pass at all
    CHECK(check_values(std::vector<int64_t>(64, INT64_MIN)) == 0);
    {
        std::vector<int64_t> v;                                             // real latencies: two passes
        for (int i = 0; i < 1000; ++i) v.push_back(2000 + (int64_t)(rng() % 7000));
        CHECK(check_values(v) == 2);
    }
    for (uint32_t n : {2u, 3u, 10u, 11u, 255u, 256u, 257u, 1000u, 4097u}) {  // even and odd, random over all 64 bits
        std::vector<int64_t> v(n);
        for (auto& x : v) x = (int64_t)rng();
        check_values(v);
        for (auto& x : v) x = (int64_t)(rng() % 5) - 2;                     // many ties around zero
        check_values(v);
        for (auto& x : v) x = (int64_t)(rng() >> 24) - (1ll << 39);         // above 2^32 either side of zero
        check_values(v);
    }
    {
        // a rank beyond the values (the buffers disagree with the count): refused
        Shards s;
        s.part = {{1, 2, 300}};
        QsRanks ranks;
        qs_ranks(QS, NQ, 5, &ranks);  // claims five values
        int64_t val[QS_MAX_RANKS];
        CHECK(!qs_select(ranks, 1, 300, s, val, nullptr));
        // a failing pass: refused
        QsRanks r1;
        qs_ranks(QS, 1, 3, &r1);
        CHECK(!qs_select(r1, 1, 300, [](const uint64_t*, uint32_t, uint32_t, uint64_t*) { return false; }, val, nullptr));
    }

    // ---- the ranks of a call: deduplicated, every quantile placed
    {
        QsRanks r;
        qs_ranks(QS, NQ, 1, &r);
        CHECK(r.n == 1 && r.rank[0] == 0);
        const uint32_t same[TW_MEASURE_MAX_QUANTILES] = {500000, 500000, 500000, 500000, 500000, 500000, 500000, 500000,
                                                         500000, 500000, 500000, 500000, 500000, 500000, 500000, 500000};
        qs_ranks(same, TW_MEASURE_MAX_QUANTILES, 10, &r);
        CHECK(r.n == 2 && r.rank[0] == 4 && r.rank[1] == 5 && r.lo_at[15] == 0 && r.hi_at[15] == 1);
        uint32_t all[TW_MEASURE_MAX_QUANTILES];
        for (uint32_t i = 0; i < TW_MEASURE_MAX_QUANTILES; ++i) all[i] = 31250 + i * 62500;  // 32 distinct ranks
        qs_ranks(all, TW_MEASURE_MAX_QUANTILES, 1000002, &r);           // pos = q * 10^6 + q: lo = q, hi = q + 1
        CHECK(r.n == QS_MAX_RANKS);
    }

    // ---- the refusals
    const uint32_t ok[2] = {0, 1000000}, bad[2] = {500000, 1000001};
    uint32_t many[TW_MEASURE_MAX_QUANTILES + 1] = {};
    CHECK(quantile_args_ok(1, 2, ok, 2));
    CHECK(quantile_args_ok(1, 2, many, TW_MEASURE_MAX_QUANTILES));
    CHECK(!quantile_args_ok(2, 2, ok, 2));                                  // equal tags
    CHECK(!quantile_args_ok(1, 2, ok, 0));                                  // n_q == 0
    CHECK(!quantile_args_ok(1, 2, many, TW_MEASURE_MAX_QUANTILES + 1));     // above the maximum
    CHECK(!quantile_args_ok(1, 2, bad, 2));                                 // a q_ppm above 10^6
    CHECK(!quantile_args_ok(1, 2, nullptr, 1));
    tw_quantile e{0, 0};
    quantile_empty(&e);
    CHECK(e.lo_us == INT64_MAX && e.hi_us == INT64_MIN);

    if (fails) return 1;
    std::printf("select ok\n");
    return 0;
}
