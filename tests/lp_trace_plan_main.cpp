// Stand-alone host program over csrc/lp_trace_plan.hpp (no HIP): built with
// ASan + UBSan by tests/test_lp_trace_host.py.  Every check prints its name on
// failure and the program exits non-zero; "ok <n>" on success.
#include <cstdio>
#include <vector>

#include "../time-warp_amd/csrc/lp_trace_plan.hpp"

using namespace tw;

static int failures = 0, checks = 0;
#define CHECK(x)                                            \
    do {                                                    \
        ++checks;                                           \
        if (!(x)) {                                         \
            ++failures;                                     \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
        }                                                   \
    } while (0)

static tw_trace_rec rec(int64_t t, uint32_t node, uint32_t tag, int64_t val) {
    tw_trace_rec r;
    r.t = t; r.val = val; r.node = node; r.tag = tag;
    return r;
}
static bool same(const tw_trace_rec& a, const tw_trace_rec& b) {
    return a.t == b.t && a.val == b.val && a.node == b.node && a.tag == b.tag;
}

// merge `lists` and compare with a plain sort of their concatenation
static void merge_case(const std::vector<std::vector<tw_trace_rec>>& lists, size_t out_cap) {
    std::vector<const tw_trace_rec*> ptr;
    std::vector<uint64_t> len;
    std::vector<tw_trace_rec> all;
    for (const auto& l : lists) {
        ptr.push_back(l.data());
        len.push_back(l.size());
        all.insert(all.end(), l.begin(), l.end());
    }
    lp_trace_sort(all.data(), all.size());
    // (exactly out_cap slots: a write past the clip is the sanitizer's to see)
    std::vector<tw_trace_rec> out(out_cap);
    const size_t w = lp_trace_merge(ptr.data(), len.data(), lists.size(), out.data(), out_cap);
    const size_t want = all.size() < out_cap ? all.size() : out_cap;
    CHECK(w == want);
    for (size_t i = 0; i < w && i < want; ++i) CHECK(same(out[i], all[i]));
    for (size_t i = 1; i < w; ++i) CHECK(!lp_trace_less(out[i], out[i - 1]));
}

int main() {
    // ---- the canonical order: t, then node, then tag, then val (signed)
    CHECK(lp_trace_less(rec(1, 9, 9, 9), rec(2, 0, 0, 0)));
    CHECK(lp_trace_less(rec(1, 1, 9, 9), rec(1, 2, 0, 0)));
    CHECK(lp_trace_less(rec(1, 1, 3, 9), rec(1, 1, 4, 0)));
    CHECK(lp_trace_less(rec(1, 1, 3, -5), rec(1, 1, 3, 4)));
    CHECK(lp_trace_less(rec(-7, 0, 0, 0), rec(0, 0, 0, 0)));
    CHECK(!lp_trace_less(rec(1, 1, 3, 4), rec(1, 1, 3, 4)));

    // ---- merges of 1 .. 4 lists, empty ones and equal keys among them
    const std::vector<tw_trace_rec> a = {rec(1, 0, 9, 7), rec(5, 2, 9, 7), rec(5, 2, 10, 1), rec(9, 1, 9, 7)};
    const std::vector<tw_trace_rec> b = {rec(0, 4, 9, 7), rec(5, 2, 9, 7), rec(5, 3, 9, -1), rec(12, 4, 11, 3)};
    const std::vector<tw_trace_rec> c = {rec(5, 2, 9, 7)};
    const std::vector<tw_trace_rec> d = {rec(2, 8, 9, 7), rec(2, 8, 9, 7), rec(30, 8, 9, 7)};
    const std::vector<tw_trace_rec> none;
    for (size_t cap : {(size_t)0, (size_t)1, (size_t)3, (size_t)12, (size_t)64}) {
        merge_case({a}, cap);
        merge_case({none}, cap);
        merge_case({a, b}, cap);
        merge_case({none, b}, cap);
        merge_case({a, none}, cap);
        merge_case({a, b, c}, cap);
        merge_case({a, none, c}, cap);
        merge_case({none, none, none}, cap);
        merge_case({a, b, c, d}, cap);
        merge_case({d, none, none, a}, cap);
        merge_case({c, c, c, c}, cap);
    }
    merge_case({}, 4);

    // ---- counts -> E, truncated, kept, offsets
    {
        const uint64_t n[3] = {5, 0, 7};
        LpTracePlan p = lp_trace_plan(n, 3, 12);  // E == cap
        CHECK(p.emitted == 12 && !p.truncated && p.gathered == 12);
        CHECK(p.kept[0] == 5 && p.kept[1] == 0 && p.kept[2] == 7);
        CHECK(p.off[0] == 0 && p.off[1] == 5 && p.off[2] == 5);
        p = lp_trace_plan(n, 3, 11);  // E == cap + 1: truncated although every shard kept all
        CHECK(p.emitted == 12 && p.truncated);
        CHECK(p.kept[0] == 5 && p.kept[2] == 7 && p.gathered == 12);
        p = lp_trace_plan(n, 3, 8);  // a cap between the largest shard count and E
        CHECK(p.emitted == 12 && p.truncated && p.kept[2] == 7);
        p = lp_trace_plan(n, 3, 6);  // a shard over the cap: it kept cap
        CHECK(p.emitted == 12 && p.truncated && p.kept[0] == 5 && p.kept[2] == 6 && p.off[2] == 5 && p.gathered == 11);
        p = lp_trace_plan(n, 3, 1u << 20);
        CHECK(p.emitted == 12 && !p.truncated);
        p = lp_trace_plan(n, 1, 5);  // one shard
        CHECK(p.emitted == 5 && !p.truncated && p.off[0] == 0);
        p = lp_trace_plan(n, 1, 4);
        CHECK(p.emitted == 5 && p.truncated && p.kept[0] == 4);
        p = lp_trace_plan(n, 0, 4);  // no shard
        CHECK(p.emitted == 0 && !p.truncated && p.gathered == 0 && p.kept.empty());
        const uint64_t z[4] = {0, 0, 0, 0};
        p = lp_trace_plan(z, 4, 9);
        CHECK(p.emitted == 0 && !p.truncated && p.off[3] == 0);
        const uint64_t big[2] = {UINT64_MAX, 2};  // a sum past 64 bits saturates: truncated
        p = lp_trace_plan(big, 2, 100);
        CHECK(p.emitted == UINT64_MAX && p.truncated && p.kept[0] == 100 && p.kept[1] == 2);
    }

    // ---- the clip: min(caller's cap, E, trace cap)
    CHECK(lp_trace_clip(12, 12, 100) == 12);
    CHECK(lp_trace_clip(12, 12, 5) == 5);
    CHECK(lp_trace_clip(12, 8, 100) == 8);
    CHECK(lp_trace_clip(3, 8, 100) == 3);
    CHECK(lp_trace_clip(0, 8, 100) == 0);
    CHECK(lp_trace_clip(12, 8, 0) == 0);
    CHECK(lp_trace_clip(UINT64_MAX, 0xFFFFFFFFu, 7) == 7);

    // ---- the whole read: sort each shard's claim-ordered block, merge, clip
    {
        std::vector<tw_trace_rec> s0 = {rec(9, 1, 9, 7), rec(1, 0, 9, 7), rec(5, 2, 10, 1)};
        std::vector<tw_trace_rec> s1 = {rec(12, 4, 11, 3), rec(0, 4, 9, 7)};
        const uint64_t n[2] = {s0.size(), s1.size()};
        const LpTracePlan p = lp_trace_plan(n, 2, 5);
        lp_trace_sort(s0.data(), s0.size());
        lp_trace_sort(s1.data(), s1.size());
        const tw_trace_rec* lists[2] = {s0.data(), s1.data()};
        const size_t k = lp_trace_clip(p.emitted, 5, 4);  // a caller's buffer smaller than E
        std::vector<tw_trace_rec> out(k);
        CHECK(k == 4 && lp_trace_merge(lists, p.kept.data(), 2, out.data(), k) == 4);
        CHECK(same(out[0], rec(0, 4, 9, 7)) && same(out[1], rec(1, 0, 9, 7)) && same(out[2], rec(5, 2, 10, 1)) &&
              same(out[3], rec(9, 1, 9, 7)));
    }

    if (failures) {
        printf("%d of %d checks failed\n", failures, checks);
        return 1;
    }
    printf("ok %d\n", checks);
    return 0;
}
