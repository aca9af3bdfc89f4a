// Stand-alone host program over csrc/live_plan.hpp (no HIP): the argument
// checks of tw_set_live_delays, the per-link descriptor, and the exactness of
// the reciprocal that replaces `mod k` in the event kernels.
// Built and run by tests/test_live_host.py with -fsanitize=address,undefined.
//   (no argument)  the checks and descriptors, and draws against the oracle's
//                  randomR (oracle/stdgen.hpp);
//   `recip`        live_mod == mod for EVERY k the plan admits (1 .. 2147483)
//                  at the arguments 0, k - 1, k, 2147483561 and 2,048 random
//                  ones each, on a few threads.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../oracle/stdgen.hpp"
#include "../time-warp_amd/csrc/live_plan.hpp"

#define CHECK(x)                                              \
    do {                                                      \
        if (!(x)) {                                           \
            printf("FAILED %s (line %d)\n", #x, __LINE__);    \
            return 1;                                         \
        }                                                     \
    } while (0)

using tw::live_mod;
using tw::live_plan;
using tw::live_recip;
using tw::LiveLink;

static int plan1(uint32_t kind, int64_t lo, int64_t hi, LiveLink* out = nullptr) {
    const tw_live_delays s{&kind, &lo, &hi, 0};
    std::vector<LiveLink> d;
    const int rc = live_plan(&s, 1, d);
    if (rc == TW_OK && out) *out = d[0];
    if (rc != TW_OK && !d.empty()) return 1000;  // a refusal hands nothing out
    return rc;
}

static int test_refusals() {
    std::vector<LiveLink> d;
    const uint32_t kind[2] = {1, 2};
    const int64_t lo[2] = {0, 1000}, hi[2] = {0, 5000};
    CHECK(live_plan(nullptr, 2, d) == TW_ERR_INVALID);
    tw_live_delays s{kind, lo, hi, 0};
    CHECK(live_plan(&s, 2, d) == TW_OK && d.size() == 2);
    s.kind = nullptr;
    CHECK(live_plan(&s, 2, d) == TW_ERR_INVALID && d.empty());
    s.kind = kind; s.lo = nullptr;
    CHECK(live_plan(&s, 2, d) == TW_ERR_INVALID);
    s.lo = lo; s.hi = nullptr;
    CHECK(live_plan(&s, 2, d) == TW_ERR_INVALID);
    // a kind above 2
    CHECK(plan1(3, 0, 0) == TW_ERR_INVALID);
    CHECK(plan1(0xFFFFFFFFu, 0, 0) == TW_ERR_INVALID);
    // lo < 0, hi > 0x7FFFFFFF (either way round)
    CHECK(plan1(2, -1, 5) == TW_ERR_INVALID);
    CHECK(plan1(2, 5, -1) == TW_ERR_INVALID);
    CHECK(plan1(2, 0x7FFFFFFFll, 0x80000000ll) == TW_ERR_INVALID);
    CHECK(plan1(2, 0x80000000ll, 0x7FFFFFFFll) == TW_ERR_INVALID);
    CHECK(plan1(2, INT64_MIN, INT64_MAX) == TW_ERR_INVALID);
    CHECK(plan1(1, -1, 0) == TW_ERR_INVALID);
    CHECK(plan1(1, 0x80000000ll, 0) == TW_ERR_INVALID);
    // a range that needs two draws: k * 1000 > 2147483562
    CHECK(plan1(2, 0, tw::LIVE_K_MAX) == TW_ERR_INVALID);          // k = LIVE_K_MAX + 1
    CHECK(plan1(2, 7, 7 + tw::LIVE_K_MAX) == TW_ERR_INVALID);
    CHECK(plan1(2, 0, 0x7FFFFFFFll) == TW_ERR_INVALID);
    // kind 0 is not looked at further; one bad link refuses the whole spec
    CHECK(plan1(0, -5, INT64_MAX) == TW_OK);
    const uint32_t k3[3] = {0, 2, 2};
    const int64_t l3[3] = {0, 0, -1}, h3[3] = {0, 2, 3};
    const tw_live_delays s3{k3, l3, h3, 0};
    CHECK(live_plan(&s3, 3, d) == TW_ERR_INVALID && d.empty());
    CHECK(live_plan(&s3, 2, d) == TW_OK && d.size() == 2);  // (the bad link lies past n_links)
    CHECK(live_plan(&s3, 0, d) == TW_OK && d.empty());
    return 0;
}

static int test_descriptors() {
    LiveLink d{};
    CHECK(tw::LIVE_K_MAX == 2147483 && tw::LIVE_X_MAX == 2147483561u);
    CHECK(sizeof(LiveLink) == 16);
    CHECK(plan1(0, 3, 9, &d) == TW_OK && d.kind == 0);
    CHECK(plan1(1, 0, 99, &d) == TW_OK && d.kind == 1 && d.lo == 0);               // hi is not read
    CHECK(plan1(1, 0x7FFFFFFFll, 0, &d) == TW_OK && d.kind == 1 && d.lo == 0x7FFFFFFFu);
    CHECK(plan1(2, 1000, 5000, &d) == TW_OK && d.kind == 2 && d.lo == 1000 && d.k == 4001 && d.m == live_recip(4001));
    // a reversed range is swapped, as randomR does
    CHECK(plan1(2, 5000, 1000, &d) == TW_OK && d.kind == 2 && d.lo == 1000 && d.k == 4001);
    // k = 1: one draw all the same, delay lo
    CHECK(plan1(2, 0, 0, &d) == TW_OK && d.kind == 2 && d.lo == 0 && d.k == 1 && d.m == 0xFFFFFFFFu);
    CHECK(plan1(2, 77, 77, &d) == TW_OK && d.k == 1 && d.lo == 77);
    // k at the bound, low and high in the delay range
    CHECK(plan1(2, 0, tw::LIVE_K_MAX - 1, &d) == TW_OK && d.k == 2147483u && d.m == 2000u);
    CHECK(plan1(2, 0x7FFFFFFFll - (tw::LIVE_K_MAX - 1), 0x7FFFFFFFll, &d) == TW_OK && d.k == 2147483u);
    CHECK((uint64_t)d.lo + d.k - 1 == 0x7FFFFFFFull);  // the largest delay a live link can give: bit 31 clear
    return 0;
}

// the plan's draw against the oracle's randomR, generator state for state
static int test_draws() {
    const int64_t ranges[][2] = {{0, 0}, {0, 2}, {0, 5}, {1000, 5000}, {5000, 1000}, {0, tw::LIVE_K_MAX - 1},
                                 {0x7FFFFFFFll - 9, 0x7FFFFFFFll}, {3, 2}};
    for (const auto& rg : ranges) {
        LiveLink d{};
        CHECK(plan1(2, rg[0], rg[1], &d) == TW_OK);
        for (int64_t seed : {0ll, 7ll, 306ll, -1ll, 0x7FFFFFFFll, 0x123456789ll}) {
            StdGen a = mk_stdgen(seed), b = a;
            for (int i = 0; i < 2000; ++i) {
                const int64_t want = stdgen_range(a, rg[0], rg[1]);
                const uint32_t z = (uint32_t)stdgen_next(b);
                CHECK(z >= 1 && z - 1u <= tw::LIVE_X_MAX);
                const int64_t got = (int64_t)d.lo + live_mod(z - 1u, d.k, d.m);
                CHECK(got == want);
                CHECK(a.s1 == b.s1 && a.s2 == b.s2);  // exactly one step each
            }
        }
    }
    return 0;
}

// live_mod(x, k, live_recip(k)) == x mod k: r = live_mod is the remainder iff
// r < k and x - r is a multiple of k; checked as r < k && (x - r) == q * k for
// the 64-bit quotient estimate's two candidates without a division per
// argument, and against `%` itself at the fixed arguments.
static bool recip_range(uint32_t k0, uint32_t k1, uint64_t* checked) {
    uint64_t n = 0;
    uint32_t s = 0x9E3779B9u ^ k0;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t m = live_recip(k);
        const uint32_t fixed[] = {0u, k - 1u, k, tw::LIVE_X_MAX, k + 1u, 2u * k - 1u, 2u * k, tw::LIVE_X_MAX - 1u,
                                  (tw::LIVE_X_MAX / k) * k, (tw::LIVE_X_MAX / k) * k - 1u};
        for (uint32_t x : fixed)
            if (live_mod(x, k, m) != x % k) return false;
        n += sizeof(fixed) / sizeof(fixed[0]);
        for (int i = 0; i < 2048; ++i) {
            s = s * 1664525u + 1013904223u;
            const uint32_t x = (uint32_t)(((uint64_t)s * (tw::LIVE_X_MAX + 1ull)) >> 32);  // in [0, LIVE_X_MAX]
            const uint32_t r = live_mod(x, k, m);
            const uint32_t q = (uint32_t)(((uint64_t)x * m) >> 32);  // floor(x / k) or one below (live_plan.hpp)
            const uint32_t d = x - r;
            if (r >= k || (d != q * k && d != (q + 1u) * k)) return false;
        }
        n += 2048;
    }
    *checked = n;
    return true;
}

static int test_recip() {
    // the sampled identity agrees with `%` where both are computed
    for (uint32_t k : {1u, 2u, 3u, 4001u, 65536u, 2147483u})
        for (uint32_t x = 0; x < 100000u; x += 7u)
            CHECK(live_mod(x, k, live_recip(k)) == x % k);
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    const uint32_t K1 = (uint32_t)tw::LIVE_K_MAX + 1u;
    std::vector<std::thread> th;
    std::vector<int> ok(nt, 0);
    std::vector<uint64_t> cnt(nt, 0);
    for (unsigned t = 0; t < nt; ++t) {
        const uint32_t a = 1u + (uint32_t)((uint64_t)(K1 - 1u) * t / nt), b = 1u + (uint32_t)((uint64_t)(K1 - 1u) * (t + 1) / nt);
        th.emplace_back([&, t, a, b] { ok[t] = recip_range(a, b, &cnt[t]) ? 1 : 0; });
    }
    for (auto& x : th) x.join();
    uint64_t total = 0;
    for (unsigned t = 0; t < nt; ++t) {
        CHECK(ok[t] == 1);
        total += cnt[t];
    }
    CHECK(total == (uint64_t)tw::LIVE_K_MAX * (2048 + 10));
    printf("recip ok: %" PRIu64 " arguments over k = 1 .. %" PRId64 "\n", total, tw::LIVE_K_MAX);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "recip")) return test_recip();
    if (test_refusals() || test_descriptors() || test_draws()) return 1;
    printf("live plan ok\n");
    return 0;
}
