// Stand-alone host program over csrc/measure_combine.hpp (no HIP): the fold
// of per-shard tw_measure outputs into a context's.  Built and run by
// tests/test_measure_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "../time-warp_amd/csrc/measure_combine.hpp"

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            return 1;                                         \
        }                                                     \
    } while (0)

static tw_measure_out entry(uint64_t pairs, int64_t lo, int64_t hi, int64_t sum) {
    tw_measure_out o;
    tw::measure_empty(&o);
    o.pairs = pairs;
    if (pairs) {
        o.min_us = lo;
        o.max_us = hi;
    }
    o.sum_us = sum;
    return o;
}

int main() {
    // spec check
    tw_measure_spec s{1, 2, 4, 0, -5, 3};
    CHECK(tw::measure_spec_ok(&s));
    tw_measure_spec bad = s;
    bad.tag_to = 1;
    CHECK(!tw::measure_spec_ok(&bad));
    bad = s; bad.n_bins = 0;
    CHECK(!tw::measure_spec_ok(&bad));
    bad = s; bad.n_bins = TW_MEASURE_MAX_BINS + 1;
    CHECK(!tw::measure_spec_ok(&bad));
    bad = s; bad.bin_us = 0;
    CHECK(!tw::measure_spec_ok(&bad));
    bad = s; bad.reserved = 1;
    CHECK(!tw::measure_spec_ok(&bad));
    CHECK(!tw::measure_spec_ok(nullptr));

    // three shards of 3, 0 and 2 replicas -> a context of 5
    const uint32_t n_bins = 4;
    const size_t n = 5;
    tw_measure_out total;
    tw::measure_empty(&total);
    CHECK(total.min_us == INT64_MAX && total.max_us == INT64_MIN && total.pairs == 0);
    std::vector<uint64_t> hist(n_bins, 0);
    std::vector<tw_measure_out> per(n);
    for (auto& p : per) tw::measure_empty(&p);

    std::vector<tw_measure_out> p0 = {entry(2, -4, 9, 5), entry(0, 0, 0, 0), entry(1, 40, 40, 40)};
    tw_measure_out t0 = entry(3, -4, 40, 45);
    t0.open_from = 2; t0.underflow = 1; t0.truncated = 1;
    std::vector<uint64_t> h0 = {1, 0, 1, 0};
    CHECK(tw::measure_combine(&total, hist.data(), n_bins, per.data(), n, &t0, h0.data(), p0.data(), 0, 3));

    tw_measure_out t1;  // an empty shard keeps min / max
    tw::measure_empty(&t1);
    std::vector<uint64_t> h1(n_bins, 0);
    CHECK(tw::measure_combine(&total, hist.data(), n_bins, per.data(), n, &t1, h1.data(), nullptr, 3, 0));
    CHECK(total.min_us == -4 && total.max_us == 40);

    std::vector<tw_measure_out> p2 = {entry(1, -30, -30, -30), entry(1, INT64_MAX, INT64_MAX, INT64_MAX)};
    tw_measure_out t2 = entry(2, -30, INT64_MAX, (int64_t)((uint64_t)INT64_MAX - 30u));
    t2.open_to = 4; t2.repeated = 1; t2.overflow = 1;
    std::vector<uint64_t> h2 = {0, 0, 0, 1};
    CHECK(tw::measure_combine(&total, hist.data(), n_bins, per.data(), n, &t2, h2.data(), p2.data(), 3, 2));

    CHECK(total.pairs == 5 && total.open_from == 2 && total.open_to == 4 && total.repeated == 1);
    CHECK(total.truncated == 1 && total.underflow == 1 && total.overflow == 1);
    CHECK(total.min_us == -30 && total.max_us == INT64_MAX);
    // the sum wraps in two's complement instead of overflowing
    CHECK(total.sum_us == (int64_t)((uint64_t)INT64_MAX - 30u + 45u) && total.sum_us < 0);
    CHECK(hist[0] == 1 && hist[1] == 0 && hist[2] == 1 && hist[3] == 1);
    CHECK(per[0].pairs == 2 && per[2].sum_us == 40 && per[3].min_us == -30 && per[4].max_us == INT64_MAX);
    CHECK(per[1].pairs == 0 && per[1].min_us == INT64_MAX);

    // a block that does not fit is refused and writes nothing
    tw_measure_out before = total;
    CHECK(!tw::measure_combine(&total, hist.data(), n_bins, per.data(), n, &t2, h2.data(), p2.data(), 4, 2));
    CHECK(!tw::measure_combine(&total, hist.data(), n_bins, per.data(), n, &t2, h2.data(), p2.data(), 6, 0));
    CHECK(std::memcmp(&before, &total, sizeof(total)) == 0 && hist[3] == 1);
    // no per-replica output asked for: totals and histogram alone
    CHECK(tw::measure_combine(&total, nullptr, n_bins, nullptr, 0, &t0, h0.data(), p0.data(), 0, 3));
    CHECK(total.pairs == 8 && hist[0] == 1);
    printf("combine ok\n");
    return 0;
}
