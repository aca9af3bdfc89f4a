// Stand-alone check of csrc/measure_series.hpp (no HIP): series_bin at the bin
// boundaries and the ends of int64, the shard fold against a direct
// computation, FIRST's chunk plan, and the spec check case by case.  Built with
// ASan + UBSan by tests/test_series_host.py; prints "series ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../time-warp_amd/csrc/measure_series.hpp"

using namespace tw;

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int test_bin() {
    const int64_t t0 = 2000, w = 1500;
    const uint32_t n = 10;
    CHECK(series_bin(t0 - 1, t0, w, n) == SERIES_UNDER);
    CHECK(series_bin(t0, t0, w, n) == 0);
    CHECK(series_bin(t0 + w - 1, t0, w, n) == 0);
    CHECK(series_bin(t0 + w, t0, w, n) == 1);
    CHECK(series_bin(t0 + n * w - 1, t0, w, n) == n - 1);
    CHECK(series_bin(t0 + n * w, t0, w, n) == SERIES_OVER);
    CHECK(series_bin(INT64_MIN, t0, w, n) == SERIES_UNDER);
    CHECK(series_bin(-1, 0, 1, 1) == SERIES_UNDER);
    // t = INT64_MAX: the difference to t0 >= 0 does not wrap
    CHECK(series_bin(INT64_MAX, 0, 1, TW_SERIES_MAX_BINS) == SERIES_OVER);
    CHECK(series_bin(INT64_MAX, INT64_MAX, 1, 1) == 0);
    CHECK(series_bin(INT64_MAX, INT64_MAX - 5, 1, 6) == 5);
    CHECK(series_bin(INT64_MAX, INT64_MAX - 6, 1, 6) == SERIES_OVER);
    CHECK(series_bin(INT64_MAX, 0, INT64_MAX, 1) == SERIES_OVER);  // bin 1 of 1
    CHECK(series_bin(INT64_MAX - 1, 0, INT64_MAX, 1) == 0);
    CHECK(series_bin(INT64_MAX, 0, INT64_MAX, 2) == 1);
    // bin_us = 1: the bin is the offset
    for (int64_t t = 0; t < 20; ++t) CHECK(series_bin(7 + t, 7, 1, 16) == (t < 16 ? (uint32_t)t : SERIES_OVER));
    // bin_us = 2^40
    const int64_t big = (int64_t)1 << 40;
    CHECK(series_bin(big - 1, 0, big, 4) == 0);
    CHECK(series_bin(big, 0, big, 4) == 1);
    CHECK(series_bin(4 * big - 1, 0, big, 4) == 3);
    CHECK(series_bin(4 * big, 0, big, 4) == SERIES_OVER);
    CHECK(series_bin(INT64_MAX, 0, big, TW_SERIES_MAX_BINS) == SERIES_OVER);  // 2^23 - 1
    CHECK(series_bin(5 + 3 * big, 5, big, 4) == 3 && series_bin(4 + 3 * big, 5, big, 4) == 2);
    return 0;
}

// replicas of random items, binned directly and through 1, 2 and 3 shards' folds
static int test_fold() {
    std::mt19937_64 rng(12345);
    const uint32_t nb = 7;
    const int64_t t0 = 100, w = 13;
    for (size_t n_shards = 1; n_shards <= 3; ++n_shards) {
        const size_t per_shard[3] = {5, 0, 3};  // (a shard without replicas among them)
        size_t n = 0;
        for (size_t s = 0; s < n_shards; ++s) n += per_shard[s];
        tw_series_out want;
        series_empty(&want);
        std::vector<uint64_t> want_count(nb, 0), want_rows(n * nb, 0);
        std::vector<tw_series_stat> want_stat(nb);
        for (auto& s : want_stat) series_stat_empty(&s);
        std::vector<tw_series_out> want_per(n);
        tw_series_out tot;
        series_empty(&tot);
        std::vector<uint64_t> count(nb, 0), rows(n * nb, 0xA5A5A5A5u);
        std::vector<tw_series_stat> stat(nb);
        for (auto& s : stat) series_stat_empty(&s);
        std::vector<tw_series_out> per(n);
        size_t r = 0;
        for (size_t s = 0; s < n_shards; ++s) {
            const size_t k = per_shard[s];
            tw_series_out st;
            series_empty(&st);
            std::vector<uint64_t> s_count(nb, 0), s_rows(k * nb, 0);
            std::vector<tw_series_stat> s_stat(nb);
            for (auto& x : s_stat) series_stat_empty(&x);
            std::vector<tw_series_out> s_per(k);
            for (size_t q = 0; q < k; ++q) {
                tw_series_out o;
                series_empty(&o);
                if (rng() % 4 == 0) {
                    o.truncated = 1;
                } else {
                    const size_t items = rng() % 40;
                    for (size_t i = 0; i < items; ++i) {
                        const int64_t t = (int64_t)(rng() % 300), d = (int64_t)(rng() % 1000) - 500;
                        const uint32_t b = series_bin(t, t0, w, nb);
                        ++o.counted;
                        o.underflow += b == SERIES_UNDER;
                        o.overflow += b == SERIES_OVER;
                        o.t_min = t < o.t_min ? t : o.t_min;
                        o.t_max = t > o.t_max ? t : o.t_max;
                        if (b < nb) {
                            ++s_count[b]; ++s_rows[q * nb + b];
                            ++want_count[b]; ++want_rows[(r + q) * nb + b];
                            tw_series_stat one{d, d, d};
                            series_stat_add(&s_stat[b], &one);
                            series_stat_add(&want_stat[b], &one);
                        }
                    }
                }
                s_per[q] = o;
                want_per[r + q] = o;
                series_add(&st, &o);
                series_add(&want, &o);
            }
            CHECK(series_combine(&tot, count.data(), stat.data(), nb, per.data(), rows.data(), n, &st, s_count.data(),
                                 s_stat.data(), s_per.data(), s_rows.data(), r, k));
            r += k;
        }
        CHECK(std::memcmp(&tot, &want, sizeof tot) == 0);
        CHECK(count == want_count && rows == want_rows);
        CHECK(std::memcmp(stat.data(), want_stat.data(), nb * sizeof(tw_series_stat)) == 0);
        CHECK(std::memcmp(per.data(), want_per.data(), n * sizeof(tw_series_out)) == 0);
        uint64_t in_bins = 0;
        for (uint64_t c : count) in_bins += c;
        CHECK(in_bins + tot.underflow + tot.overflow == tot.counted);
        // a block that does not fit changes nothing
        tw_series_out before = tot, extra;
        series_empty(&extra);
        extra.counted = 9;
        std::vector<tw_series_out> one(1);
        CHECK(!series_combine(&tot, count.data(), nullptr, nb, per.data(), nullptr, n, &extra, nullptr, nullptr,
                              one.data(), nullptr, n, 1));
        CHECK(std::memcmp(&tot, &before, sizeof tot) == 0);
    }
    // the two's-complement sum wraps without undefined behaviour
    tw_series_stat a{INT64_MAX, 1, 2}, b{1, 0, 3};
    series_stat_add(&a, &b);
    CHECK(a.sum_us == INT64_MIN && a.min_us == 0 && a.max_us == 3);
    // empties are the identity
    tw_series_out e, acc;
    series_empty(&e);
    series_empty(&acc);
    series_add(&acc, &e);
    CHECK(acc.counted == 0 && acc.t_min == INT64_MAX && acc.t_max == INT64_MIN);
    return 0;
}

static int test_chunks() {
    const uint64_t limits[] = {1, 7, 16, 100, 448, 1ull << 25};
    const uint32_t reps[] = {1, 2, 69, 70, 1000, 65536};
    const uint32_t nodes[] = {1, 7, 16, 130, 1u << 20, 1u << 25};
    for (uint64_t limit : limits)
        for (uint32_t R : reps)
            for (uint32_t N : nodes) {
                const SeriesChunks p = series_chunks(R, N, limit);
                if (N > limit) {
                    CHECK(p.per_chunk == 0);
                    continue;
                }
                CHECK(p.per_chunk >= 1 && (uint64_t)p.per_chunk * N <= limit && p.per_chunk <= R);
                // every replica once, in order
                uint32_t next = 0;
                for (uint32_t k = 0; k < p.n_chunks; ++k) {
                    uint32_t first = 0, count = 0;
                    series_chunk_at(p, R, k, &first, &count);
                    CHECK(first == next && count >= 1 && count <= p.per_chunk);
                    CHECK((uint64_t)count * N <= limit);
                    next += count;
                }
                CHECK(next == R);
                uint32_t first = 0, count = 1;
                series_chunk_at(p, R, p.n_chunks, &first, &count);  // behind the last: empty
                CHECK(first == R && count == 0);
            }
    CHECK(series_chunks(70, 7, 16).per_chunk == 2 && series_chunks(70, 7, 16).n_chunks == 35);
    CHECK(series_chunks(70, 7, SERIES_MAX_ENTRIES).n_chunks == 1);
    CHECK(series_chunks(4, (1u << 25) + 1, SERIES_MAX_ENTRIES).per_chunk == 0);  // too many nodes
    CHECK(series_chunks(4, 0, SERIES_MAX_ENTRIES).per_chunk == 0);
    CHECK(series_chunks(0, 5, SERIES_MAX_ENTRIES).n_chunks == 0);
    CHECK(series_chunks(UINT32_MAX, 1u << 25, SERIES_MAX_ENTRIES).n_chunks == UINT32_MAX);
    return 0;
}

static int test_spec() {
    tw_series_spec ok{};
    ok.tag = 5;
    ok.mode = TW_SERIES_EVENTS;
    ok.n_bins = 10;
    ok.t0_us = 0;
    ok.bin_us = 1;
    CHECK(series_spec_ok(&ok));
    CHECK(!series_spec_ok(nullptr));
    tw_series_spec s = ok;
    s.n_bins = 0;
    CHECK(!series_spec_ok(&s));
    s = ok; s.n_bins = TW_SERIES_MAX_BINS;
    CHECK(series_spec_ok(&s));
    s.mode = TW_SERIES_FIRST;
    CHECK(series_spec_ok(&s));
    s.n_bins = TW_SERIES_MAX_BINS + 1;
    CHECK(!series_spec_ok(&s));
    s.mode = TW_SERIES_EVENTS;
    CHECK(!series_spec_ok(&s));
    s = ok; s.t0_us = -1;
    CHECK(!series_spec_ok(&s));
    s = ok; s.t0_us = INT64_MAX;
    CHECK(series_spec_ok(&s));
    s = ok; s.bin_us = 0;
    CHECK(!series_spec_ok(&s));
    s = ok; s.bin_us = -7;
    CHECK(!series_spec_ok(&s));
    s = ok; s.bin_us = INT64_MAX;
    CHECK(series_spec_ok(&s));
    s = ok; s.reserved = 1;
    CHECK(!series_spec_ok(&s));
    s = ok; s.mode = 3;
    CHECK(!series_spec_ok(&s));
    s = ok; s.tag_to = 6;  // only LATENCY takes a second tag
    CHECK(!series_spec_ok(&s));
    s.mode = TW_SERIES_FIRST;
    CHECK(!series_spec_ok(&s));
    s.mode = TW_SERIES_LATENCY;
    CHECK(series_spec_ok(&s));
    s.tag_to = s.tag;
    CHECK(!series_spec_ok(&s));
    s.tag = 0; s.tag_to = 0;
    CHECK(!series_spec_ok(&s));
    s.tag = 0; s.tag_to = 1;  // (tag 0 is a tag like any other)
    CHECK(series_spec_ok(&s));
    s.n_bins = TW_SERIES_MAX_LAT_BINS;
    CHECK(series_spec_ok(&s));
    s.n_bins = TW_SERIES_MAX_LAT_BINS + 1;
    CHECK(!series_spec_ok(&s));
    return 0;
}

int main() {
    if (test_bin() || test_fold() || test_chunks() || test_spec()) return 1;
    std::printf("series ok\n");
    return 0;
}
