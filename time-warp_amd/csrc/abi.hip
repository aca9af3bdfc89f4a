// abi.hip — the public C ABI of libtimewarp.so (include/timewarp.h) over one
// or more device shards (engine.hip via shard.hpp).
//
// Replaces the runner of time-warp's pure-emulation path,
//   runTimedT :: (MonadIO m, MonadCatch m) => TimedT m a -> m a
//   (src/Control/TimeWarp/Timed/TimedT.hs:293-304),
// for a batch of replicas (or one node-partitioned scenario) spread over the
// GPUs of a node, with the library owning the collectives:
//   * tw_create(devices, ndev): one process drives ndev GPUs; replicas are
//     split into contiguous blocks [g*R/G, (g+1)*R/G), the
//     statistics are all-reduced over RCCL communicators the library creates
//     (ncclCommInitAll); a node-partitioned scenario's window loop moves its
//     record blocks by RCCL send/recv and reduces its window words by RCCL
//     all-reduce(min), all enqueued on the shards' streams.  A device listed
//     twice (tests on one GPU) or TW_TRANSPORT=copy uses device-to-device
//     copies ordered by HIP events instead of RCCL;
//   * tw_comm_id + tw_create_rank: one process per GPU (torchrun) with a
//     library-owned RCCL communicator over all ranks (ncclCommInitRank): the
//     same collectives, across processes.
// No CPU fallback: without a gfx950 device tw_create fails.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../../include/timewarp.h"
#include "live_plan.hpp"
#include "lp_run_plan.hpp"
#include "lp_trace_plan.hpp"
#include "measure_combine.hpp"
#include "measure_select.hpp"
#include "measure_series.hpp"
#include "shard.hpp"
#include "tw_dev.hpp"

using namespace tw;

namespace {

enum Transport { TP_NONE, TP_RCCL, TP_COPY };

#define RD_N 4  // reduction words (tw_dev.hpp RD_COUNT)
static_assert(RD_N == RD_COUNT, "reduction words");

// COPY transport: red[i] = min over the ranks' words (staged in `all`)
__global__ void tw_red_min(int64_t* red, const int64_t* all, uint32_t world) {
    const uint32_t i = threadIdx.x;
    if (i >= RD_N) return;
    int64_t m = all[i];
    for (uint32_t g = 1; g < world; ++g) m = all[(size_t)g * RD_N + i] < m ? all[(size_t)g * RD_N + i] : m;
    red[i] = m;
}

}  // namespace

struct tw_ctx {
    std::vector<tw_shard*> sh;
    std::vector<int> dev;
    int world = 1;       // ranks of the job: this process's shards (tw_create) or the processes (tw_create_rank)
    int rank0 = 0;       // global rank of sh[0]
    Transport tp = TP_NONE;
    std::vector<ncclComm_t> comm;  // one per shard (TP_RCCL)
    std::vector<uint32_t> rep0;    // first replica of each shard, within this context
    // node-partitioned mode over several shards / ranks (tw_lp_run)
    uint32_t lp_begin = 0, lp_count = 0;
    bool lp_ready = false;                  // exchange buffers made for this load
    std::vector<uint32_t> starts;           // world + 1 node boundaries
    // COPY, per shard: made once per context, reused by every set-up (lp_copy_objects)
    std::vector<int64_t*> red_all;          // [world][RD_N]
    std::vector<hipEvent_t> ev_a, ev_b;
    std::vector<void*> scratch;             // per shard: RCCL statistics buffer
    uint32_t xcap = LP_XCAP_DEFAULT;        // exchange block stride (records per rank pair)
    // an RCCL call of this context failed: the communicators may hold a
    // collective the peers are still in, so every later communicating call
    // returns TW_ERR_COMM without entering another one (timewarp.h, tw_lp_run)
    bool comm_broken = false;
    // testing hook (nccl_test_fail): TW_TEST_FAIL_NCCL as it was when the
    // context was made (0: off), and the checked RCCL calls made since
    long test_fail_at = 0;
    std::atomic<long> test_calls{0};
    double measure_ms = 0.0;  // kernels of the last tw_measure (tw_measure_ms)
    double measure_phase_ms[MEASURE_PHASES] = {};  // ... by kernel (tw_measure_phases_ms): the slowest shard's
    // tw_set_measure_keys, and the testing hook TW_TEST_MEASURE (test_hook_init)
    MeasureCfg measure_cfg{TW_MEASURE_MAX_KEYS, TW_MEASURE_MAX_KEYS, 1024};
    // tw_measure_quantiles: the per-replica select's LDS-sort capacity (the
    // testing hook TW_TEST_QUANTILE_LDS lowers it) and the last call's device
    // time by phase (tw_measure_quantiles_ms)
    uint32_t quantile_lds = QS_LDS_MAX;
    double quantile_ms[5] = {};
    // tw_measure_series: FIRST's table entries at a time (the testing hook
    // TW_TEST_SERIES lowers it) and the last call's device time by phase
    // (tw_measure_series_ms)
    uint64_t series_entries = SERIES_MAX_ENTRIES;
    double series_ms[SERIES_PHASES] = {};
    uint32_t lp_trace_cap = 0;  // tw_lp_set_trace: records the context keeps track of (each shard holds as many)
};

namespace {

int comm_fail(ncclResult_t r, const char* what) {
    fprintf(stderr, "timewarp: %s failed: %s\n", what, ncclGetErrorString(r));
    return TW_ERR_COMM;
}
// testing hook: a context made with TW_TEST_FAIL_NCCL=k in the environment
// fails its k-th checked RCCL call (counting from 1) without making it
// (one-rank jobs in the tests).  The variable is read once, when the context
// is made (test_hook_init), not on every call.
void test_hook_init(tw_ctx* c) {
    const char* e = getenv("TW_TEST_FAIL_NCCL");
    c->test_fail_at = e ? atol(e) : 0;
    // TW_TEST_MEASURE=lds_keys:bucket_keys sends tw_measure's replicas with
    // more than lds_keys (0 .. TW_MEASURE_MAX_KEYS) matching records through
    // the partition path, with buckets of bucket_keys (1 .. 2^22) keys in the
    // mean: small shapes reach that path, and one bucket can be overfilled.
    // What tw_set_measure_keys accepts is unchanged.
    if (const char* m = getenv("TW_TEST_MEASURE")) {
        char* end = nullptr;
        const long lds = strtol(m, &end, 10);
        const long bk = (end && *end == ':') ? strtol(end + 1, nullptr, 10) : 0;
        if (lds >= 0 && lds <= (long)TW_MEASURE_MAX_KEYS && bk >= 1 && bk <= (1l << 22)) {
            c->measure_cfg.lds_keys = (uint32_t)lds;
            c->measure_cfg.bucket_keys = (uint32_t)bk;
        }
    }
    // TW_TEST_QUANTILE_LDS=n (0 .. 2048) lowers the number of latencies that
    // tw_measure_quantiles' per-replica select sorts in LDS: a replica of a few
    // dozen pairs then takes the radix path.
    if (const char* q = getenv("TW_TEST_QUANTILE_LDS")) {
        const long n = strtol(q, nullptr, 10);
        if (n >= 0 && n <= (long)QS_LDS_MAX) c->quantile_lds = (uint32_t)n;
    }
    // TW_TEST_SERIES=entries (1 .. 2^25) lowers the (replica, node) entries that
    // tw_measure_series' FIRST mode tables at a time: a few dozen replicas then
    // take several chunks.
    if (const char* s = getenv("TW_TEST_SERIES")) {
        const long long n = strtoll(s, nullptr, 10);
        if (n >= 1 && n <= (long long)SERIES_MAX_ENTRIES) c->series_entries = (uint64_t)n;
    }
}
bool nccl_test_fail(tw_ctx* c) { return c->test_fail_at > 0 && ++c->test_calls == c->test_fail_at; }
// (in a function of the context c: a failure marks it unusable)
#define NCCLCHK(x)                                   \
    do {                                             \
        ncclResult_t _r = nccl_test_fail(c) ? ncclInternalError : (x); \
        if (_r != ncclSuccess) {                     \
            c->comm_broken = true;                   \
            return comm_fail(_r, #x);                \
        }                                            \
    } while (0)
// ... between ncclGroupStart and ncclGroupEnd: a failure closes the group
// first, so the thread is not left inside it (a later group of this thread --
// a fresh context's -- would be folded into the open one).  That does not
// contain the failure: closing the group launches what was already posted, so
// peers that posted the full set stay blocked in the operations this rank
// never posted until they abort on their own.  TW_ERR_COMM reaching the
// caller must therefore abort the job.  This context's communicators are
// aborted, not destroyed, but only at tw_destroy (destroy_parts)
#define NCCLCHK_G(x)                                 \
    do {                                             \
        ncclResult_t _r = nccl_test_fail(c) ? ncclInternalError : (x); \
        if (_r != ncclSuccess) {                     \
            (void)ncclGroupEnd();                    \
            c->comm_broken = true;                   \
            return comm_fail(_r, #x);                \
        }                                            \
    } while (0)
// ... the group's end: an injected failure still closes the group
#define NCCLCHK_GEND()                               \
    do {                                             \
        const bool _inj = nccl_test_fail(c);         \
        ncclResult_t _r = ncclGroupEnd();            \
        if (_inj) _r = ncclInternalError;            \
        if (_r != ncclSuccess) {                     \
            c->comm_broken = true;                   \
            return comm_fail(_r, "ncclGroupEnd()");  \
        }                                            \
    } while (0)
#define NCCLCHK_NC(x)                                \
    do {                                             \
        ncclResult_t _r = (x);                       \
        if (_r != ncclSuccess) return comm_fail(_r, #x); \
    } while (0)
#define HIPCHK_A(x)                                  \
    do {                                             \
        hipError_t _e = (x);                         \
        if (_e != hipSuccess) {                      \
            fprintf(stderr, "timewarp: %s failed: %s\n", #x, hipGetErrorString(_e)); \
            return _e == hipErrorOutOfMemory ? TW_ERR_OOM : TW_ERR_HIP; \
        }                                            \
    } while (0)

// run f(shard index) for every shard, concurrently when there are several
// (each shard is its own device and stream; the HIP runtime is thread-safe);
// returns the first error
template <class F>
int each_shard(tw_ctx* c, F f) {
    const size_t n = c->sh.size();
    if (n == 1) return f(0);
    std::vector<int> rc(n, TW_OK);
    std::vector<std::thread> th;
    th.reserve(n);
    for (size_t i = 0; i < n; ++i) th.emplace_back([&, i] { rc[i] = f(i); });
    for (auto& t : th) t.join();
    for (int r : rc)
        if (r != TW_OK) return r;
    return TW_OK;
}

// enqueue on `st`, a stream of device dst_dev, a copy from device src_dev
int copy_async(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
    if (src_dev == dst_dev)
        HIPCHK_A(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    else
        HIPCHK_A(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
    return TW_OK;
}

int scratch_of(tw_ctx* c, size_t i, void** p) {
    if (c->scratch.size() != c->sh.size()) c->scratch.assign(c->sh.size(), nullptr);
    if (!c->scratch[i]) {
        HIPCHK_A(hipSetDevice(c->dev[i]));
        HIPCHK_A(hipMalloc(&c->scratch[i], 64 * 8));
    }
    *p = c->scratch[i];
    return TW_OK;
}

// All-reduce over the job (every shard of every rank): `sums` with SUM,
// `maxs` with MAX (int64), in place; one call per shard, enqueued as one
// RCCL group on the shards' streams.  Without RCCL the shards' values are
// combined on the host.
int job_reduce(tw_ctx* c, std::vector<std::vector<uint64_t>>& sums, std::vector<std::vector<int64_t>>& maxs) {
    const size_t n = c->sh.size();
    const size_t ns = sums[0].size(), nm = maxs[0].size();
    if (c->tp != TP_RCCL) {
        for (size_t i = 1; i < n; ++i) {
            for (size_t k = 0; k < ns; ++k) sums[0][k] += sums[i][k];
            for (size_t k = 0; k < nm; ++k) maxs[0][k] = std::max(maxs[0][k], maxs[i][k]);
        }
        for (size_t i = 1; i < n; ++i) { sums[i] = sums[0]; maxs[i] = maxs[0]; }
        return TW_OK;
    }
    std::vector<void*> buf(n);
    for (size_t i = 0; i < n; ++i) {
        int rc = scratch_of(c, i, &buf[i]);
        if (rc) return rc;
        HIPCHK_A(hipSetDevice(c->dev[i]));
        HIPCHK_A(hipMemcpy(buf[i], sums[i].data(), 8 * ns, hipMemcpyHostToDevice));
        HIPCHK_A(hipMemcpy((char*)buf[i] + 8 * ns, maxs[i].data(), 8 * nm, hipMemcpyHostToDevice));
    }
    NCCLCHK(ncclGroupStart());
    for (size_t i = 0; i < n; ++i) {
        NCCLCHK_G(ncclAllReduce(buf[i], buf[i], ns, ncclUint64, ncclSum, c->comm[i], nullptr));
        NCCLCHK_G(ncclAllReduce((char*)buf[i] + 8 * ns, (char*)buf[i] + 8 * ns, nm, ncclInt64, ncclMax, c->comm[i],
                              nullptr));
    }
    NCCLCHK_GEND();
    for (size_t i = 0; i < n; ++i) {
        HIPCHK_A(hipSetDevice(c->dev[i]));
        HIPCHK_A(hipStreamSynchronize(nullptr));
        HIPCHK_A(hipMemcpy(sums[i].data(), buf[i], 8 * ns, hipMemcpyDeviceToHost));
        HIPCHK_A(hipMemcpy(maxs[i].data(), (char*)buf[i] + 8 * ns, 8 * nm, hipMemcpyDeviceToHost));
    }
    return TW_OK;
}

// Every shard of every rank learns the worst of the shards' local codes, by
// their severity (sev_of, lp_run_plan.hpp), in one small all-reduce: a rank
// that failed locally joins the collective instead of leaving the others
// waiting in the next one
int job_agree(tw_ctx* c, const std::vector<int>& local, int* worst) {
    if (c->tp != TP_RCCL) {  // one process holds every shard
        *worst = worst_of(local);
        return TW_OK;
    }
    const size_t n = c->sh.size();
    std::vector<std::vector<uint64_t>> sums(n, std::vector<uint64_t>{0});
    std::vector<std::vector<int64_t>> maxs(n);
    for (size_t i = 0; i < n; ++i) maxs[i] = {sev_of(local[i])};
    const int rc = job_reduce(c, sums, maxs);
    if (rc) return rc;
    *worst = rc_of_sev(maxs[0][0]);
    return TW_OK;
}

int64_t dbits(double v) {
    int64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
double bitsd(int64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

// tw_stats of every shard -> the job's (sums of counts, max of times); the
// status code joins the reduction (the worst), so every rank returns it
int reduce_stats(tw_ctx* c, std::vector<tw_stats>& st, std::vector<int>& rcs, tw_stats* out, int* rc_out) {
    const size_t n = c->sh.size();
    std::vector<std::vector<uint64_t>> sums(n);
    std::vector<std::vector<int64_t>> maxs(n);
    for (size_t i = 0; i < n; ++i) {
        const tw_stats& s = st[i];
        sums[i] = {s.events, s.sends, s.delivered, s.dropped, s.undeliverable, s.replicas_done, s.replicas_error,
                   s.launches};
        maxs[i] = {s.max_final_t, dbits(s.kernel_ms), dbits(s.wall_ms), sev_of(rcs[i])};
    }
    int rc = job_reduce(c, sums, maxs);
    if (rc) return rc;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->events = sums[0][0]; out->sends = sums[0][1]; out->delivered = sums[0][2]; out->dropped = sums[0][3];
        out->undeliverable = sums[0][4]; out->replicas_done = (uint32_t)sums[0][5];
        out->replicas_error = (uint32_t)sums[0][6]; out->launches = (uint32_t)sums[0][7];
        out->max_final_t = maxs[0][0]; out->kernel_ms = bitsd(maxs[0][1]); out->wall_ms = bitsd(maxs[0][2]);
    }
    *rc_out = rc_of_sev(maxs[0][3]);
    return TW_OK;
}

// a shard's slice of a replica batch: replicas [b0, b0 + nb) of desc, with
// the replica-minor link table and the main registers cut to them
struct SubDesc {
    tw_scenario_desc d;
    std::vector<uint32_t> table;
};
void sub_desc(const tw_scenario_desc* s, uint32_t b0, uint32_t nb, SubDesc& o) {
    o.d = *s;
    o.d.n_replicas = nb;
    if (s->main_regs) o.d.main_regs = s->main_regs + (size_t)b0 * 4;
    if (s->link_table) {
        const size_t rows = (size_t)s->n_links * s->link_depth;
        o.table.resize(rows * nb);
        for (size_t i = 0; i < rows; ++i)
            std::memcpy(o.table.data() + i * nb, s->link_table + i * s->n_replicas + b0, 4ull * nb);
        o.d.link_table = o.table.data();
    }
}

int destroy_parts(tw_ctx* c) {
    // (a failed call may have left a collective the peers never joined:
    // abort, which does not wait for it, instead of destroy)
    for (size_t i = 0; i < c->comm.size(); ++i)
        if (c->comm[i]) (void)(c->comm_broken ? ncclCommAbort(c->comm[i]) : ncclCommDestroy(c->comm[i]));
    c->comm.clear();
    for (size_t i = 0; i < c->sh.size(); ++i) {
        (void)hipSetDevice(c->dev[i]);
        if (i < c->scratch.size() && c->scratch[i]) (void)hipFree(c->scratch[i]);
        if (i < c->red_all.size() && c->red_all[i]) (void)hipFree(c->red_all[i]);
        if (i < c->ev_a.size() && c->ev_a[i]) (void)hipEventDestroy(c->ev_a[i]);
        if (i < c->ev_b.size() && c->ev_b[i]) (void)hipEventDestroy(c->ev_b[i]);
        sh_destroy(c->sh[i]);
    }
    c->sh.clear();
    return TW_OK;
}

bool single(tw_ctx* c) { return c->sh.size() == 1; }

// a device buffer released on every return
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
};

// ---- tw_lp_run's host side (its arithmetic: lp_run_plan.hpp).  Set-up, once
// per load: node boundaries, the shards' exchange buffers, COPY's objects.

// node boundaries of every rank -> c->starts
int lp_boundaries(tw_ctx* c) {
    const uint32_t world = (uint32_t)c->world;
    if (!(c->tp == TP_RCCL && single(c) && world > 1)) {
        lp_starts_even(c->lp_begin, c->lp_count, world, c->starts);
        return TW_OK;
    }
    // one shard per process: all-gather (begin, count) over the ranks
    DevBuf buf;
    HIPCHK_A(hipSetDevice(c->dev[0]));
    HIPCHK_A(hipMalloc(&buf.p, 8ull * (world + 1)));
    const uint32_t mine[2] = {c->lp_begin, c->lp_count};
    HIPCHK_A(hipMemcpy((char*)buf.p + 8ull * world, mine, 8, hipMemcpyHostToDevice));
    NCCLCHK(ncclAllGather((char*)buf.p + 8ull * world, buf.p, 2, ncclUint32, c->comm[0], nullptr));
    HIPCHK_A(hipStreamSynchronize(nullptr));
    std::vector<uint32_t> h(2ull * world);
    HIPCHK_A(hipMemcpy(h.data(), buf.p, 8ull * world, hipMemcpyDeviceToHost));
    return lp_starts_gathered(h.data(), world, c->starts) ? TW_OK : TW_ERR_INVALID;
}

// COPY: every shard's staging words and two events.  They depend on world and
// the shard count alone, so what a first set-up made every later one keeps
// (and one that failed half-way is completed); destroy_parts frees them.
int lp_copy_objects(tw_ctx* c) {
    const size_t n = c->sh.size();
    c->red_all.resize(n, nullptr);
    c->ev_a.resize(n, nullptr);
    c->ev_b.resize(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        HIPCHK_A(hipSetDevice(c->dev[i]));
        if (!c->red_all[i]) HIPCHK_A(hipMalloc((void**)&c->red_all[i], 8ull * RD_N * c->world));
        if (!c->ev_a[i]) HIPCHK_A(hipEventCreateWithFlags(&c->ev_a[i], hipEventDisableTiming));
        if (!c->ev_b[i]) HIPCHK_A(hipEventCreateWithFlags(&c->ev_b[i], hipEventDisableTiming));
    }
    return TW_OK;
}

// A shard's local failure (lrc) from here on is carried to every rank by the
// agreement before the next collective: no rank is left waiting in one.
int lp_setup(tw_ctx* c, std::vector<int>& lrc) {
    int rc = lp_boundaries(c);
    if (rc) return rc;
    c->xcap = lp_parse_xcap(getenv("TW_LP_XCAP"), c->xcap);
    for (size_t i = 0; i < c->sh.size(); ++i)
        lrc[i] = sh_lp_exchange_own(c->sh[i], (uint32_t)c->world, (uint32_t)(c->rank0 + i), c->starts.data(), c->xcap);
    if (c->tp == TP_COPY) rc = lp_copy_objects(c);
    c->lp_ready = !rc;
    return rc;
}

// The transports of the loop.  What one call works on:
struct LpLoop {
    tw_ctx* c;
    std::vector<ShardXchg> x;  // per shard: its stream, blocks and window words
    size_t stride_b;           // bytes from one rank's block to the next
};
// ... and the two operations of a tick, chosen once per call
struct LpTransport {
    int (*blocks)(const LpLoop&, size_t bytes);  // block g of rank r's send -> block r of rank g's recv
    int (*words)(const LpLoop&);                 // every rank's x.red <- the ranks' minimum, word by word
};

int rccl_blocks(const LpLoop& l, size_t bytes) {
    tw_ctx* c = l.c;
    NCCLCHK(ncclGroupStart());
    for (size_t i = 0; i < l.x.size(); ++i)
        for (int g = 0; g < c->world; ++g) {
            const ShardXchg& x = l.x[i];
            NCCLCHK_G(ncclSend((char*)x.send + g * l.stride_b, bytes, ncclUint8, g, c->comm[i], x.stream));
            NCCLCHK_G(ncclRecv((char*)x.recv + g * l.stride_b, bytes, ncclUint8, g, c->comm[i], x.stream));
        }
    NCCLCHK_GEND();
    return TW_OK;
}

int rccl_words(const LpLoop& l) {
    tw_ctx* c = l.c;
    NCCLCHK(ncclGroupStart());
    for (size_t i = 0; i < l.x.size(); ++i)
        NCCLCHK_G(ncclAllReduce(l.x[i].red, l.x[i].red, RD_N, ncclInt64, ncclMin, c->comm[i], l.x[i].stream));
    NCCLCHK_GEND();
    return TW_OK;
}

int nothing_from(size_t, size_t) { return TW_OK; }
int nothing_then(size_t) { return TW_OK; }
// COPY: one event round.  Every shard records ev on its stream; then every
// shard i, its device current, makes its stream wait for each other shard g's
// event right before from(i, g) enqueues what i takes from g (from(i, i)
// waits for nothing), and runs then(i) behind all of them.
template <class From, class Then = int (*)(size_t)>
int copy_round(const LpLoop& l, const std::vector<hipEvent_t>& ev, From from, Then then = nothing_then) {
    const tw_ctx* c = l.c;
    const size_t n = l.x.size();
    for (size_t i = 0; i < n; ++i) {
        HIPCHK_A(hipSetDevice(c->dev[i]));
        HIPCHK_A(hipEventRecord(ev[i], l.x[i].stream));
    }
    for (size_t i = 0; i < n; ++i) {
        HIPCHK_A(hipSetDevice(c->dev[i]));
        for (size_t g = 0; g < n; ++g) {
            if (g != i) HIPCHK_A(hipStreamWaitEvent(l.x[i].stream, ev[g], 0));
            const int rc = from(i, g);
            if (rc) return rc;
        }
        const int rc = then(i);
        if (rc) return rc;
    }
    return TW_OK;
}

int copy_blocks(const LpLoop& l, size_t bytes) {
    const tw_ctx* c = l.c;
    return copy_round(l, c->ev_a, [&](size_t i, size_t g) {
        return copy_async((char*)l.x[i].recv + g * l.stride_b, c->dev[i], (const char*)l.x[g].send + i * l.stride_b,
                          c->dev[g], bytes, l.x[i].stream);
    });
}

int copy_words(const LpLoop& l) {
    const tw_ctx* c = l.c;
    const int rc = copy_round(l, c->ev_b, [&](size_t i, size_t g) {
        return copy_async(c->red_all[i] + g * RD_N, c->dev[i], l.x[g].red, c->dev[g], 8 * RD_N, l.x[i].stream);
    });
    if (rc) return rc;
    // every shard's copies of the others' words must land before any shard
    // overwrites its own (its next tick's fill): a second event round orders
    // the min after all copies
    return copy_round(l, c->ev_a, nothing_from, [&](size_t i) -> int {
        hipLaunchKernelGGL(tw_red_min, dim3(1), dim3(64), 0, l.x[i].stream, l.x[i].red, (const int64_t*)c->red_all[i],
                           (uint32_t)l.x.size());
        HIPCHK_A(hipGetLastError());
        return TW_OK;
    });
}

const LpTransport LP_RCCL{rccl_blocks, rccl_words}, LP_COPY{copy_blocks, copy_words};

}  // namespace

static_assert(TW_ABI_VERSION == 4u, "tw_version names ABI 4");
static_assert(RD_N == TW_LP_RED_WORDS, "the caller-owned reduction buffer (timewarp.h)");

extern "C" {

const char* tw_version(void) {
    return "timewarp-mi355x 0.6 (gfx950; lane-per-replica dense/narrow/sparse kernels, wavefront-per-replica kernel, "
           "node-partitioned LP kernel with device-driven windows, batched logical processes (tw_lpb_load); "
           "multi-GPU contexts with library-owned RCCL communicators; "
           "ABI 4)";
}

const char* tw_strerror(int code) {
    switch (code) {
    case TW_OK: return "ok";
    case TW_ERR_INVALID: return "invalid argument or scenario descriptor";
    case TW_ERR_NO_DEVICE: return "no HIP device";
    case TW_ERR_HIP: return "HIP runtime error";
    case TW_ERR_OOM: return "device out of memory";
    case TW_ERR_STATE: return "call out of order";
    case TW_ERR_REPLICA: return "replica error";
    case TW_ERR_INCOMPLETE: return "relaunch cap reached before every replica stopped";
    case TW_ERR_COMM: return "RCCL error";
    default: return "unknown error";
    }
}

int tw_create(const int* devices, int ndev, tw_ctx** out) {
    if (!out) return TW_ERR_INVALID;
    *out = nullptr;
    if (!devices || ndev < 1 || ndev > 64) return TW_ERR_INVALID;
    tw_ctx* c = new (std::nothrow) tw_ctx;
    if (!c) return TW_ERR_OOM;
    for (int i = 0; i < ndev; ++i) {
        tw_shard* s = nullptr;
        int rc = sh_create(devices[i], &s);
        if (rc) {
            destroy_parts(c);
            delete c;
            return rc;
        }
        c->sh.push_back(s);
        c->dev.push_back(devices[i]);
    }
    c->world = ndev;
    c->rank0 = 0;
    test_hook_init(c);
    if (ndev > 1) {
        std::vector<int> sorted(c->dev);
        std::sort(sorted.begin(), sorted.end());
        const bool dup = std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
        const char* t = getenv("TW_TRANSPORT");
        c->tp = (dup || (t && !strcmp(t, "copy"))) ? TP_COPY : TP_RCCL;
        if (c->tp == TP_RCCL) {
            c->comm.assign(ndev, nullptr);
            const ncclResult_t r = ncclCommInitAll(c->comm.data(), ndev, c->dev.data());
            if (r != ncclSuccess) {
                comm_fail(r, "ncclCommInitAll");
                c->comm.assign(ndev, nullptr);
                destroy_parts(c);
                delete c;
                return TW_ERR_COMM;
            }
        }
    }
    *out = c;
    return TW_OK;
}

int tw_comm_id(uint8_t* id) {
    if (!id) return TW_ERR_INVALID;
    ncclUniqueId u;
    NCCLCHK_NC(ncclGetUniqueId(&u));
    static_assert(sizeof(u) == TW_COMM_ID_BYTES, "RCCL unique id size");
    std::memcpy(id, &u, sizeof(u));
    return TW_OK;
}

int tw_create_rank(int device, int nranks, int rank, const uint8_t* id, tw_ctx** out) {
    if (!out) return TW_ERR_INVALID;
    *out = nullptr;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return TW_ERR_INVALID;
    tw_ctx* c = new (std::nothrow) tw_ctx;
    if (!c) return TW_ERR_OOM;
    tw_shard* s = nullptr;
    int rc = sh_create(device, &s);
    if (rc) {
        delete c;
        return rc;
    }
    c->sh.push_back(s);
    c->dev.push_back(device);
    c->world = nranks;
    c->rank0 = rank;
    c->tp = TP_RCCL;
    test_hook_init(c);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    c->comm.assign(1, nullptr);
    (void)hipSetDevice(device);
    const ncclResult_t r = ncclCommInitRank(&c->comm[0], nranks, u, rank);
    if (r != ncclSuccess) {
        comm_fail(r, "ncclCommInitRank");
        c->comm.assign(1, nullptr);
        destroy_parts(c);
        delete c;
        return TW_ERR_COMM;
    }
    *out = c;
    return TW_OK;
}

int tw_ctx_info(tw_ctx* c, int* ndev, int* world, int* rank0, int* transport) {
    if (!c) return TW_ERR_INVALID;
    if (ndev) *ndev = (int)c->sh.size();
    if (world) *world = c->world;
    if (rank0) *rank0 = c->rank0;
    if (transport) *transport = (int)c->tp;
    return TW_OK;
}

void tw_destroy(tw_ctx* c) {
    if (!c) return;
    destroy_parts(c);
    delete c;
}

// ------------------------------------------------------------ replica mode
static int load_split(tw_ctx* c, const tw_scenario_desc* s, bool pow2,
                      int (*ld)(tw_shard*, const tw_scenario_desc*, const void*), const void* arg) {
    const uint32_t n = (uint32_t)c->sh.size();
    if (!s || s->n_replicas < n) return TW_ERR_INVALID;
    if (pow2) {  // batched LP: every shard's block a power of two
        if (s->n_replicas % n) return TW_ERR_INVALID;
        const uint32_t b = s->n_replicas / n;
        if (b & (b - 1)) return TW_ERR_INVALID;
    }
    c->rep0.assign(n, 0);
    std::vector<SubDesc> sd(n);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t b0, nb;
        split(s->n_replicas, n, i, b0, nb);
        c->rep0[i] = b0;
        sub_desc(s, b0, nb, sd[i]);
    }
    return each_shard(c, [&](size_t i) { return ld(c->sh[i], &sd[i].d, arg); });
}

int tw_load(tw_ctx* c, const tw_scenario_desc* s) {
    if (!c) return TW_ERR_INVALID;
    c->lp_ready = false;
    if (single(c)) {
        c->rep0.assign(1, 0);
        return sh_load(c->sh[0], s);
    }
    return load_split(c, s, false, [](tw_shard* h, const tw_scenario_desc* d, const void*) { return sh_load(h, d); },
                      nullptr);
}

int tw_reset(tw_ctx* c) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_reset(s);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_run(tw_ctx* c, int64_t t_end_us, uint64_t max_events, tw_stats* out) {
    if (!c) return TW_ERR_INVALID;
    if (single(c) && c->tp == TP_NONE) return sh_run(c->sh[0], t_end_us, max_events, out);
    if (c->comm_broken) return TW_ERR_COMM;
    const size_t n = c->sh.size();
    std::vector<tw_stats> st(n);
    std::vector<int> rcs(n, TW_OK);
    auto w0 = std::chrono::steady_clock::now();
    (void)each_shard(c, [&](size_t i) {
        rcs[i] = sh_run(c->sh[i], t_end_us, max_events, &st[i]);
        return TW_OK;
    });
    for (size_t i = 0; i < n; ++i)
        if (rcs[i] != TW_OK && rcs[i] != TW_ERR_INCOMPLETE && rcs[i] != TW_ERR_REPLICA) std::memset(&st[i], 0, sizeof(tw_stats));
    int rc = TW_OK;
    tw_stats agg{};
    int e = reduce_stats(c, st, rcs, &agg, &rc);
    if (e) return e;
    agg.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    if (out) *out = agg;
    return rc;
}

int tw_tie_audit(tw_ctx* c, int64_t t_end_us, uint64_t max_events, uint32_t probes, tw_stats* out) {
    if (!c) return TW_ERR_INVALID;
    if (single(c) && c->tp == TP_NONE) return sh_tie_audit(c->sh[0], t_end_us, max_events, probes, out);
    if (c->comm_broken) return TW_ERR_COMM;
    const size_t n = c->sh.size();
    std::vector<tw_stats> st(n);
    std::vector<int> rcs(n, TW_OK);
    (void)each_shard(c, [&](size_t i) {
        rcs[i] = sh_tie_audit(c->sh[i], t_end_us, max_events, probes, &st[i]);
        return TW_OK;
    });
    int rc = TW_OK;
    int e = reduce_stats(c, st, rcs, out, &rc);
    return e ? e : rc;
}

static size_t local_replicas(tw_ctx* c) {
    size_t n = 0;
    for (tw_shard* s : c->sh) n += sh_replicas(s);
    return n;
}

int tw_read_results(tw_ctx* c, tw_replica_result* out, size_t n) {
    if (!c || !out) return TW_ERR_INVALID;
    if (n < local_replicas(c)) return TW_ERR_INVALID;
    size_t off = 0;
    for (tw_shard* s : c->sh) {
        const size_t k = sh_replicas(s);
        int rc = sh_read_results(s, out + off, k);
        if (rc) return rc;
        off += k;
    }
    return TW_OK;
}

int tw_read_hashes(tw_ctx* c, uint64_t* out, size_t n) {
    if (!c || !out) return TW_ERR_INVALID;
    size_t need = 0;
    for (tw_shard* s : c->sh) need += (size_t)sh_replicas(s) * sh_nodes(s);
    if (n < need) return TW_ERR_INVALID;
    size_t off = 0;
    for (tw_shard* s : c->sh) {
        const size_t k = (size_t)sh_replicas(s) * sh_nodes(s);
        int rc = sh_read_hashes(s, out + off, k);
        if (rc) return rc;
        off += k;
    }
    return TW_OK;
}

int tw_read_final(tw_ctx* c, int64_t* max_final_t, uint64_t* delivered, uint64_t* dropped, uint64_t* events) {
    if (!c) return TW_ERR_INVALID;
    std::vector<tw_replica_result> rr(local_replicas(c));
    int rc = tw_read_results(c, rr.data(), rr.size());
    if (rc) return rc;
    int64_t ft = 0;
    uint64_t dl = 0, dr = 0, ev = 0;
    for (auto& x : rr) {
        ft = x.final_t > ft ? x.final_t : ft;
        dl += x.delivered; dr += x.dropped; ev += x.events;
    }
    if (max_final_t) *max_final_t = ft;
    if (delivered) *delivered = dl;
    if (dropped) *dropped = dr;
    if (events) *events = ev;
    return TW_OK;
}

// Live delays: the checks and the per-link descriptors are made once
// (live_plan.hpp) and handed to every shard, whose first replica's seed is
// seed_base + its first replica's index in the batch.  Nothing changes unless
// every check passes.
int tw_set_live_delays(tw_ctx* c, const tw_live_delays* spec) {
    if (!c || c->sh.empty()) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh)
        if (!sh_loaded(s)) return TW_ERR_STATE;
    for (tw_shard* s : c->sh)
        if (sh_is_lp(s)) return TW_ERR_INVALID;  // tw_lp_load, tw_lpb_load: no replica execution order
    std::vector<LiveLink> desc;
    if (spec) {
        int rc = live_plan(spec, sh_links(c->sh[0]), desc);
        if (rc) return rc;
        if (desc.empty()) desc.resize(1);  // (a scenario without links: a non-null table all the same)
    }
    for (size_t i = 0; i < c->sh.size(); ++i) {
        const uint32_t b0 = i < c->rep0.size() ? c->rep0[i] : 0u;
        int rc = sh_set_live(c->sh[i], spec ? desc.data() : nullptr, spec ? spec->seed_base + (int64_t)b0 : 0);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_live_stats(tw_ctx* c, uint64_t* draws) {
    if (!c || !draws) return TW_ERR_INVALID;
    uint64_t n = 0;
    for (tw_shard* s : c->sh) {
        uint64_t k = 0;
        int rc = sh_live_stats(s, &k);
        if (rc) return rc;
        n += k;
    }
    *draws = n;
    return TW_OK;
}

int tw_set_trace(tw_ctx* c, uint32_t cap) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_set_trace(s, cap);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_set_trace_batch(tw_ctx* c, int on) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {  // (checked before any shard changes: a context's shards are of one kind)
        int rc = sh_set_trace_batch(s, on);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_read_trace(tw_ctx* c, uint32_t replica, tw_trace_rec* out, size_t cap, uint64_t* n_emitted) {
    if (!c) return TW_ERR_INVALID;
    for (size_t i = c->sh.size(); i-- > 0;) {
        const uint32_t b0 = i < c->rep0.size() ? c->rep0[i] : 0u;
        if (replica >= b0) return sh_read_trace(c->sh[i], replica - b0, out, cap, n_emitted);
    }
    return TW_ERR_INVALID;
}

// Every shard measures its own replicas; the host folds the shards' outputs
// (measure_combine.hpp) into temporaries and hands them out only when every
// shard succeeded, so a failing call leaves the caller's buffers untouched.
int tw_measure(tw_ctx* c, const tw_measure_spec* spec, tw_measure_out* total, uint64_t* hist,
               tw_measure_out* per_replica, size_t n) {
    if (!c || !spec) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_measure_state(s);
        if (rc) return rc;
    }
    if (!measure_spec_ok(spec)) return TW_ERR_INVALID;
    if (n == 0) per_replica = nullptr;
    if (per_replica && n != local_replicas(c)) return TW_ERR_INVALID;
    tw_measure_out tot;
    measure_empty(&tot);
    std::vector<uint64_t> h(spec->n_bins, 0), sh_h(spec->n_bins);
    std::vector<tw_measure_out> per(per_replica ? n : 0), sh_per;
    double ms = 0.0, phase[MEASURE_PHASES] = {}, sph[MEASURE_PHASES];
    size_t off = 0;
    for (tw_shard* s : c->sh) {
        const size_t k = sh_replicas(s);
        tw_measure_out st;
        double sms = 0.0;
        if (per_replica) sh_per.resize(k);
        int rc = sh_measure(s, spec, c->measure_cfg, &st, sh_h.data(), per_replica ? sh_per.data() : nullptr, &sms,
                            sph);
        if (rc) return rc;
        if (sms > ms || off == 0) std::copy(sph, sph + MEASURE_PHASES, phase);
        if (!measure_combine(&tot, h.data(), spec->n_bins, per_replica ? per.data() : nullptr, n, &st, sh_h.data(),
                             per_replica ? sh_per.data() : nullptr, off, k))
            return TW_ERR_INVALID;
        ms = sms > ms ? sms : ms;
        off += k;
    }
    if (total) *total = tot;
    if (hist) std::memcpy(hist, h.data(), (size_t)spec->n_bins * 8);
    if (per_replica) std::memcpy(per_replica, per.data(), n * sizeof(tw_measure_out));
    c->measure_ms = ms;
    std::copy(phase, phase + MEASURE_PHASES, c->measure_phase_ms);
    return TW_OK;
}

// Every shard joins its replicas with the emit variant, which leaves the pair
// latencies on its device (MeasureEmit), and selects its own replicas'
// quantiles.  The batch's are selected over all shards without moving a
// latency: qs_select (measure_select.hpp) asks every shard for the digit counts
// of a pass and takes the steps on the sums.  As in tw_measure the caller's
// buffers are written only when everything succeeded.
int tw_measure_quantiles(tw_ctx* c, uint32_t tag_from, uint32_t tag_to, const uint32_t* q_ppm, uint32_t n_q,
                         tw_quantile* total, tw_quantile* per_replica, size_t n, uint64_t* pairs,
                         uint64_t* truncated) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_measure_state(s);
        if (rc) return rc;
    }
    if (!quantile_args_ok(tag_from, tag_to, q_ppm, n_q)) return TW_ERR_INVALID;
    if (n == 0) per_replica = nullptr;
    if (per_replica && n != local_replicas(c)) return TW_ERR_INVALID;
    // the join's spec: one bin that is never counted (the emit variant stores
    // a latency where tw_measure bins it)
    tw_measure_spec spec{};
    spec.tag_from = tag_from;
    spec.tag_to = tag_to;
    spec.n_bins = 1;
    spec.bin_us = 1;
    struct Emits {  // the shards' latency buffers, released on every return path
        std::vector<MeasureEmit> e;
        ~Emits() {
            for (MeasureEmit& m : e) measure_emit_free(&m);
        }
    } em;
    em.e.resize(c->sh.size());
    tw_measure_out tot;
    measure_empty(&tot);
    std::vector<tw_quantile> per(per_replica ? n * n_q : 0);
    double ph[5] = {};
    size_t off = 0;
    for (size_t i = 0; i < c->sh.size(); ++i) {
        tw_shard* s = c->sh[i];
        const size_t k = sh_replicas(s);
        tw_measure_out st;
        double jms = 0.0, sms = 0.0;
        int rc = sh_measure(s, &spec, c->measure_cfg, &st, nullptr, nullptr, &jms, nullptr, &em.e[i]);
        if (rc) return rc;
        measure_add(&tot, &st);
        if (per_replica) {
            if (off > n || k > n - off) return TW_ERR_INVALID;
            rc = select_replicas(sh_device(s), sh_stream(s), em.e[i], (uint32_t)k, q_ppm, n_q, c->quantile_lds,
                                 per.data() + off * n_q, &sms);
            if (rc) return rc;
        }
        ph[0] = std::max(ph[0], jms);
        ph[1] = std::max(ph[1], em.e[i].offsets_ms);
        ph[2] = std::max(ph[2], sms);
        off += k;
    }
    std::vector<tw_quantile> tq(total ? n_q : 0);
    if (total && tot.pairs == 0) {
        for (tw_quantile& q : tq) quantile_empty(&q);
    } else if (total) {
        QsRanks ranks;
        qs_ranks(q_ppm, n_q, tot.pairs, &ranks);
        int64_t val[QS_MAX_RANKS];
        int rc = TW_OK;
        uint32_t passes = 0;
        auto count = [&](const uint64_t* prefix, uint32_t nk, uint32_t shift, uint64_t* hist) {
            double slowest = 0.0;
            for (size_t i = 0; i < c->sh.size() && rc == TW_OK; ++i) {
                double ms = 0.0;
                rc = select_count(sh_device(c->sh[i]), sh_stream(c->sh[i]), em.e[i], (uint32_t)sh_replicas(c->sh[i]),
                                  prefix, nk, shift, hist, &ms);
                slowest = std::max(slowest, ms);
            }
            ph[3] += slowest;
            return rc == TW_OK;
        };
        if (!qs_select(ranks, tot.min_us, tot.max_us, count, val, &passes))
            return rc ? rc : TW_ERR_STATE;  // (a rank beyond the counted: the buffers disagree with `pairs`)
        ph[4] = passes;
        for (uint32_t i = 0; i < n_q; ++i) tq[i] = tw_quantile{val[ranks.lo_at[i]], val[ranks.hi_at[i]]};
    }
    if (total) std::copy(tq.begin(), tq.end(), total);
    if (per_replica) std::copy(per.begin(), per.end(), per_replica);
    if (pairs) *pairs = tot.pairs;
    if (truncated) *truncated = tot.truncated;
    std::copy(ph, ph + 5, c->quantile_ms);
    return TW_OK;
}

int tw_measure_quantiles_ms(tw_ctx* c, double* ms, size_t cap) {
    if (!c || !ms) return TW_ERR_INVALID;
    const size_t n = cap < 5 ? cap : 5;
    std::copy(c->quantile_ms, c->quantile_ms + n, ms);
    return (int)n;
}

// Every shard bins its own replicas; the host folds the shards' outputs
// (measure_series.hpp) into temporaries handed out only when every shard
// succeeded.  The phase times are the slowest shard's of each phase.
int tw_measure_series(tw_ctx* c, const tw_series_spec* spec, tw_series_out* total, uint64_t* count,
                      tw_series_stat* stat, tw_series_out* per_replica, uint64_t* per_replica_count, size_t n) {
    if (!c || !spec) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_measure_state(s);
        if (rc) return rc;
    }
    if (!series_spec_ok(spec)) return TW_ERR_INVALID;
    if (stat && spec->mode != TW_SERIES_LATENCY) return TW_ERR_INVALID;
    if (n == 0) per_replica = nullptr, per_replica_count = nullptr;
    if ((per_replica || per_replica_count) && n != local_replicas(c)) return TW_ERR_INVALID;
    const uint32_t nb = spec->n_bins;
    tw_series_out tot;
    series_empty(&tot);
    std::vector<uint64_t> cnt(nb, 0), sh_cnt(nb);
    std::vector<tw_series_stat> st(stat ? nb : 0), sh_st(stat ? nb : 0);
    for (tw_series_stat& s : st) series_stat_empty(&s);
    std::vector<tw_series_out> per(per_replica ? n : 0), sh_per;
    std::vector<uint64_t> rows(per_replica_count ? n * nb : 0), sh_rows;
    double ph[SERIES_PHASES] = {}, sph[SERIES_PHASES];
    size_t off = 0;
    for (tw_shard* s : c->sh) {
        const size_t k = sh_replicas(s);
        tw_series_out sh_tot;
        if (per_replica) sh_per.resize(k);
        if (per_replica_count) sh_rows.resize(k * nb);
        int rc = sh_measure_series(s, spec, c->measure_cfg, c->series_entries, &sh_tot, sh_cnt.data(),
                                   stat ? sh_st.data() : nullptr, per_replica ? sh_per.data() : nullptr,
                                   per_replica_count ? sh_rows.data() : nullptr, sph);
        if (rc) return rc;
        if (!series_combine(&tot, cnt.data(), stat ? st.data() : nullptr, nb, per_replica ? per.data() : nullptr,
                            per_replica_count ? rows.data() : nullptr, n, &sh_tot, sh_cnt.data(),
                            stat ? sh_st.data() : nullptr, per_replica ? sh_per.data() : nullptr,
                            per_replica_count ? sh_rows.data() : nullptr, off, k))
            return TW_ERR_INVALID;
        for (int i = 0; i < SERIES_PHASES; ++i) ph[i] = std::max(ph[i], sph[i]);
        off += k;
    }
    if (total) *total = tot;
    if (count) std::memcpy(count, cnt.data(), (size_t)nb * 8);
    if (stat) std::memcpy(stat, st.data(), (size_t)nb * sizeof(tw_series_stat));
    if (per_replica) std::memcpy(per_replica, per.data(), n * sizeof(tw_series_out));
    if (per_replica_count) std::memcpy(per_replica_count, rows.data(), n * nb * 8);
    std::copy(ph, ph + SERIES_PHASES, c->series_ms);
    return TW_OK;
}

int tw_measure_series_ms(tw_ctx* c, double* ms, size_t cap) {
    if (!c || !ms) return TW_ERR_INVALID;
    const size_t n = cap < (size_t)SERIES_PHASES ? cap : (size_t)SERIES_PHASES;
    std::copy(c->series_ms, c->series_ms + n, ms);
    return (int)n;
}

int tw_set_measure_keys(tw_ctx* c, uint32_t max_keys) {
    if (!c || max_keys < TW_MEASURE_MAX_KEYS || max_keys > TW_MEASURE_MAX_KEYS_LARGE) return TW_ERR_INVALID;
    c->measure_cfg.max_keys = max_keys;  // (of the context: every shard's tw_measure gets it)
    return TW_OK;
}

int tw_measure_phases_ms(tw_ctx* c, double* ms, size_t cap) {
    if (!c || !ms) return TW_ERR_INVALID;
    const size_t n = cap < (size_t)MEASURE_PHASES ? cap : (size_t)MEASURE_PHASES;
    std::copy(c->measure_phase_ms, c->measure_phase_ms + n, ms);
    return (int)n;
}

int tw_measure_ms(tw_ctx* c, double* kernel_ms) {
    if (!c || !kernel_ms) return TW_ERR_INVALID;
    *kernel_ms = c->measure_ms;
    return TW_OK;
}

int tw_set_counter_base(tw_ctx* c, uint32_t seq0, uint32_t tid0) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_set_counter_base(s, seq0, tid0);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_set_tie_mode(tw_ctx* c, uint32_t mode) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_set_tie_mode(s, mode);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_set_sweep(tw_ctx* c, int on) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_set_sweep(s, on);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_set_prefix(tw_ctx* c, int on) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_set_prefix(s, on);
        if (rc) return rc;
    }
    return TW_OK;
}

int tw_prefix_stats(tw_ctx* c, int64_t* t0_us, uint64_t* events_per_replica, uint64_t* bytes_per_replica,
                    uint32_t* last_use, double* apply_ms) {
    if (!c || c->sh.empty()) return TW_ERR_INVALID;
    return sh_prefix_stats(c->sh[0], t0_us, events_per_replica, bytes_per_replica, last_use, apply_ms);
}

int tw_prefix_clean_stats(tw_ctx* c, uint32_t* claimed_slots, uint64_t* rows_skipped, uint64_t* bytes_stored_per_replica,
                          uint32_t* verified, uint64_t* audit_mismatches) {
    if (!c || c->sh.empty()) return TW_ERR_INVALID;
    return sh_prefix_clean_stats(c->sh[0], claimed_slots, rows_skipped, bytes_stored_per_replica, verified,
                                 audit_mismatches);
}

int tw_prefix_rows_stats(tw_ctx* c, tw_prefix_rows* out) {
    if (!c || c->sh.empty()) return TW_ERR_INVALID;
    return sh_prefix_rows_stats(c->sh[0], out);
}

int tw_sweep_stats(tw_ctx* c, uint64_t* killers, uint64_t* victims, uint64_t* refused_replicas) {
    if (!c) return TW_ERR_INVALID;
    uint64_t k = 0, v = 0, f = 0;
    for (tw_shard* s : c->sh) {
        uint64_t a = 0, b = 0, d = 0;
        int rc = sh_sweep_stats(s, &a, &b, &d, nullptr);
        if (rc) return rc;
        k += a; v += b; f += d;
    }
    if (killers) *killers = k;
    if (victims) *victims = v;
    if (refused_replicas) *refused_replicas = f;
    return TW_OK;
}

int tw_sweep_path_stats(tw_ctx* c, uint64_t* terminal_replicas, uint64_t* fast_entries, uint64_t* slow_entries) {
    if (!c) return TW_ERR_INVALID;
    uint64_t k = 0, v = 0, f = 0;
    for (tw_shard* s : c->sh) {
        uint64_t a = 0, b = 0, d = 0;
        int rc = sh_sweep_path_stats(s, &a, &b, &d);
        if (rc) return rc;
        k += a; v += b; f += d;
    }
    if (terminal_replicas) *terminal_replicas = k;
    if (fast_entries) *fast_entries = v;
    if (slow_entries) *slow_entries = f;
    return TW_OK;
}

int tw_geometry(tw_ctx* c) {
    if (!c) return TW_ERR_INVALID;
    return sh_geometry(c->sh[0]);
}

int tw_last_launch_ms(tw_ctx* c, double* out, size_t cap) {
    if (!c || !out) return TW_ERR_INVALID;
    size_t n = 0;
    for (tw_shard* s : c->sh) {
        int k = sh_last_launch_ms(s, out + n, cap - n);
        if (k < 0) return k;
        n += (size_t)k;
    }
    return (int)n;
}

// ------------------------------------------------- node-partitioned (LP) mode
int tw_lp_load(tw_ctx* c, const tw_scenario_desc* s, uint32_t lp_begin, uint32_t lp_count, int64_t lookahead_us,
               uint32_t inbox_cap, uint32_t outbox_cap) {
    if (!c || !s) return TW_ERR_INVALID;
    c->lp_ready = false;
    c->lp_begin = lp_begin;
    c->lp_count = lp_count;
    const uint32_t n = (uint32_t)c->sh.size();
    if (n == 1) return sh_lp_load(c->sh[0], s, lp_begin, lp_count, lookahead_us, inbox_cap, outbox_cap);
    if (lp_count < n) return TW_ERR_INVALID;
    return each_shard(c, [&](size_t i) {
        uint32_t b0, nb;
        split(lp_count, n, (uint32_t)i, b0, nb);
        return sh_lp_load(c->sh[i], s, lp_begin + b0, nb, lookahead_us, inbox_cap, outbox_cap);
    });
}

int tw_lpb_load(tw_ctx* c, const tw_scenario_desc* s, int64_t lookahead_us, const uint32_t* node_inbox_cap,
                uint32_t inbox_cap, uint32_t outbox_cap) {
    if (!c) return TW_ERR_INVALID;
    c->lp_ready = false;
    if (single(c)) {
        c->rep0.assign(1, 0);
        return sh_lpb_load(c->sh[0], s, lookahead_us, node_inbox_cap, inbox_cap, outbox_cap);
    }
    struct A { int64_t L; const uint32_t* caps; uint32_t ib, ob; } a{lookahead_us, node_inbox_cap, inbox_cap, outbox_cap};
    return load_split(c, s, true,
                      [](tw_shard* h, const tw_scenario_desc* d, const void* p) {
                          const A* q = (const A*)p;
                          return sh_lpb_load(h, d, q->L, q->caps, q->ib, q->ob);
                      },
                      &a);
}

int tw_lpb_windows(tw_ctx* c, uint64_t* windows, uint64_t* ticks) {
    if (!c) return TW_ERR_INVALID;
    uint64_t w = 0, t = 0;
    for (tw_shard* s : c->sh) {
        uint64_t a = 0, b = 0;
        int rc = sh_lpb_windows(s, &a, &b);
        if (rc) return rc;
        w = std::max(w, a);
        t = std::max(t, b);
    }
    if (windows) *windows = w;
    if (ticks) *ticks = t;
    return TW_OK;
}

int tw_lpb_batch(tw_ctx* c, uint64_t* batched, uint64_t* due_records) {
    if (!c) return TW_ERR_INVALID;
    uint64_t b = 0, d = 0;
    for (tw_shard* s : c->sh) {
        uint64_t x = 0, y = 0;
        int rc = sh_lpb_batch(s, &x, &y);
        if (rc) return rc;
        b += x;
        d += y;
    }
    if (batched) *batched = b;
    if (due_records) *due_records = d;
    return TW_OK;
}

// the host-driven window loop and the caller-driven device loop speak for one
// shard (the caller moves the records between contexts / ranks)
#define ONE_SHARD(c)                                  \
    do {                                              \
        if (!(c)) return TW_ERR_INVALID;              \
        if (!single(c)) return TW_ERR_STATE;          \
    } while (0)

int tw_lp_window(tw_ctx* c, int64_t t_end_excl, int64_t* next_t, uint64_t* n_foreign) {
    ONE_SHARD(c);
    return sh_lp_window(c->sh[0], t_end_excl, next_t, n_foreign);
}
int tw_lp_take_outbox(tw_ctx* c, tw_lp_record* out, size_t cap, size_t* n) {
    ONE_SHARD(c);
    return sh_lp_take_outbox(c->sh[0], out, cap, n);
}
int tw_lp_inject(tw_ctx* c, const tw_lp_record* recs, size_t n, int64_t* next_t) {
    ONE_SHARD(c);
    return sh_lp_inject(c->sh[0], recs, n, next_t);
}
int tw_set_stream(tw_ctx* c, void* hs) {
    ONE_SHARD(c);
    return sh_set_stream(c->sh[0], hs);
}
int tw_lp_exchange_setup(tw_ctx* c, uint32_t world, uint32_t rank, const uint32_t* starts, void* send, void* recv,
                         uint32_t cap, int64_t* red) {
    ONE_SHARD(c);
    c->lp_ready = false;
    return sh_lp_exchange_setup(c->sh[0], world, rank, starts, send, recv, cap, red);
}
int tw_lp_loop_begin(tw_ctx* c) {
    ONE_SHARD(c);
    return sh_lp_loop_begin(c->sh[0]);
}
int tw_lp_tick(tw_ctx* c) {
    ONE_SHARD(c);
    return sh_lp_tick(c->sh[0]);
}
int tw_lp_tick_import(tw_ctx* c) {
    ONE_SHARD(c);
    return sh_lp_tick_import(c->sh[0]);
}
int tw_lp_tick_end(tw_ctx* c) {
    ONE_SHARD(c);
    return sh_lp_tick_end(c->sh[0]);
}
int tw_lp_progress(tw_ctx* c, tw_lp_state* out) {
    ONE_SHARD(c);
    return sh_lp_progress(c->sh[0], out);
}
int tw_lp_run_windows(tw_ctx* c, uint64_t max_ticks, tw_lp_state* out) {
    ONE_SHARD(c);
    return sh_lp_run_windows(c->sh[0], max_ticks, out);
}

// Results of a node-partitioned run: the whole job's (every shard of every
// rank: counts summed, final time / status / main exception the largest,
// node hashes summed mod 2^64).
int tw_lp_results(tw_ctx* c, tw_replica_result* agg, uint64_t* node_hashes, size_t n_nodes) {
    if (!c || !agg) return TW_ERR_INVALID;
    if (single(c) && c->tp == TP_NONE) return sh_lp_results(c->sh[0], agg, node_hashes, n_nodes);
    if (c->comm_broken) return TW_ERR_COMM;
    const size_t n = c->sh.size();
    std::vector<std::vector<uint64_t>> sums(n);
    std::vector<std::vector<int64_t>> maxs(n);
    std::vector<std::vector<uint64_t>> hs(n);
    for (size_t i = 0; i < n; ++i) {
        tw_replica_result a{};
        hs[i].assign(n_nodes, 0);
        // a local failure joins the reduction (every rank returns it) instead
        // of leaving the other ranks in the all-reduce
        const int lrc = sh_lp_results(c->sh[i], &a, node_hashes ? hs[i].data() : nullptr, n_nodes);
        sums[i] = {a.events, a.delivered, a.dropped, a.undeliverable, a.threads};
        maxs[i] = {a.final_t, (int64_t)a.status, (int64_t)a.main_exc, sev_of(lrc)};
    }
    int rc = job_reduce(c, sums, maxs);
    if (rc) return rc;
    if (maxs[0][3]) return rc_of_sev(maxs[0][3]);
    std::memset(agg, 0, sizeof(*agg));
    agg->events = sums[0][0]; agg->delivered = sums[0][1]; agg->dropped = sums[0][2];
    agg->undeliverable = sums[0][3]; agg->threads = sums[0][4];
    agg->final_t = maxs[0][0]; agg->status = (uint32_t)maxs[0][1]; agg->main_exc = (uint32_t)maxs[0][2];
    if (node_hashes) {
        if (c->tp == TP_RCCL) {
            std::vector<void*> buf(n);
            for (size_t i = 0; i < n; ++i) {
                HIPCHK_A(hipSetDevice(c->dev[i]));
                HIPCHK_A(hipMalloc(&buf[i], 8 * n_nodes + 8));
                HIPCHK_A(hipMemcpy(buf[i], hs[i].data(), 8 * n_nodes, hipMemcpyHostToDevice));
            }
            NCCLCHK(ncclGroupStart());
            for (size_t i = 0; i < n; ++i)
                NCCLCHK_G(ncclAllReduce(buf[i], buf[i], n_nodes, ncclUint64, ncclSum, c->comm[i], nullptr));
            NCCLCHK_GEND();
            for (size_t i = 0; i < n; ++i) {
                HIPCHK_A(hipSetDevice(c->dev[i]));
                HIPCHK_A(hipStreamSynchronize(nullptr));
                if (i == 0) HIPCHK_A(hipMemcpy(node_hashes, buf[i], 8 * n_nodes, hipMemcpyDeviceToHost));
                HIPCHK_A(hipFree(buf[i]));
            }
        } else {
            for (size_t k = 0; k < n_nodes; ++k) {
                uint64_t h = 0;
                for (size_t i = 0; i < n; ++i) h += hs[i][k];
                node_hashes[k] = h;
            }
        }
    }
    return TW_OK;
}

// ---- TRACE records of a node-partitioned context (lp_trace_plan.hpp holds
// the counting rule, the gather offsets and the merge).  Every shard keeps up
// to `cap` records of its own node block; the context sums the counts.
int tw_lp_set_trace(tw_ctx* c, uint32_t cap) {
    if (!c) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {  // (checked before any shard changes)
        int rc = sh_lp_kind(s);
        if (rc) return rc;
    }
    for (tw_shard* s : c->sh) {
        int rc = sh_lp_set_trace(s, cap);
        if (rc) {
            for (tw_shard* u : c->sh) (void)sh_lp_set_trace(u, 0);  // all or none: tracing off
            c->lp_trace_cap = 0;
            return rc;
        }
    }
    c->lp_trace_cap = cap;
    return TW_OK;
}

namespace {
// the shards' emitted counts, each read behind its shard's last run
int lp_trace_counts(tw_ctx* c, std::vector<uint64_t>& counts) {
    counts.assign(c->sh.size(), 0);
    for (size_t i = 0; i < c->sh.size(); ++i) {
        int rc = sh_lp_trace_count(c->sh[i], &counts[i]);
        if (rc) return rc;
    }
    return TW_OK;
}

// The shards' kept records of a context that is not truncated (p.emitted of
// them, > 0), gathered into one buffer on shard 0's device by copies ordered on
// shard 0's stream, with the one replica's emitted count behind them.  The
// caller synchronises that stream before the buffer goes.
struct LpGather : DevBuf {
    uint64_t* d_n = nullptr;
};
int lp_gather(tw_ctx* c, const LpTracePlan& p, LpGather* buf) {
    const int dev0 = c->dev[0];
    hipStream_t st = sh_stream(c->sh[0]);
    HIPCHK_A(hipSetDevice(dev0));
    // the records, then the replica's emitted count
    if (hipMalloc(&buf->p, (size_t)p.emitted * 32 + 8) != hipSuccess) {
        (void)hipGetLastError();  // (not sticky: the context stays usable)
        return TW_ERR_OOM;
    }
    for (size_t i = 0; i < c->sh.size(); ++i) {
        if (!p.kept[i]) continue;
        const int rc = copy_async((char*)buf->p + (size_t)p.off[i] * 32, dev0, sh_lp_trace_dev(c->sh[i]), c->dev[i],
                                  (size_t)p.kept[i] * 32, st);
        if (rc) return rc;
    }
    buf->d_n = (uint64_t*)((char*)buf->p + (size_t)p.emitted * 32);
    HIPCHK_A(hipMemcpyAsync(buf->d_n, &p.emitted, 8, hipMemcpyHostToDevice, st));
    return TW_OK;
}
}  // namespace

int tw_lp_read_trace(tw_ctx* c, tw_trace_rec* out, size_t cap, uint64_t* n_emitted) {
    if (!c || (cap && !out)) return TW_ERR_INVALID;
    std::vector<uint64_t> counts;
    int rc = lp_trace_counts(c, counts);
    if (rc) return rc;
    const LpTracePlan p = lp_trace_plan(counts.data(), counts.size(), c->lp_trace_cap);
    const size_t k = lp_trace_clip(p.emitted, c->lp_trace_cap, cap);
    if (k) {
        const size_t n = c->sh.size();
        std::vector<std::vector<tw_trace_rec>> recs(n);
        std::vector<const tw_trace_rec*> lists(n);
        for (size_t i = 0; i < n; ++i) {
            recs[i].resize((size_t)p.kept[i]);
            rc = sh_lp_trace_fetch(c->sh[i], recs[i].data(), recs[i].size());
            if (rc) return rc;
            lp_trace_sort(recs[i].data(), recs[i].size());  // (claim order says nothing)
            lists[i] = recs[i].data();
        }
        std::vector<tw_trace_rec> merged(k);
        if (lp_trace_merge(lists.data(), p.kept.data(), n, merged.data(), k) != k) return TW_ERR_STATE;
        std::memcpy(out, merged.data(), k * sizeof(tw_trace_rec));
    }
    if (n_emitted) *n_emitted = p.emitted;
    return TW_OK;
}

// The join over the context's one replica: the shards' kept records are
// gathered into one buffer on shard 0's device (device-to-device or peer
// copies on shard 0's stream, after every shard's stream was synchronised by
// the count read), and tw_measure's pass runs there over one replica of E
// records.  The buffer lives for the call; the caller's buffers are written
// only on success.
int tw_lp_measure(tw_ctx* c, const tw_measure_spec* spec, tw_measure_out* out, uint64_t* hist) {
    if (!c || !spec) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_lp_trace_state(s);
        if (rc) return rc;
    }
    if (!measure_spec_ok(spec)) return TW_ERR_INVALID;
    if (c->world != (int)c->sh.size()) return TW_ERR_INVALID;  // a rank of a larger job: no job-wide gather
    std::vector<uint64_t> counts;
    int rc = lp_trace_counts(c, counts);
    if (rc) return rc;
    const LpTracePlan p = lp_trace_plan(counts.data(), counts.size(), c->lp_trace_cap);
    tw_measure_out tot;
    measure_empty(&tot);
    std::vector<uint64_t> h(spec->n_bins, 0);
    double ms = 0.0, phase[MEASURE_PHASES] = {};
    if (p.truncated) {
        tot.truncated = 1;  // (contributes nothing else; no gather)
    } else if (p.emitted) {
        LpGather buf;
        rc = lp_gather(c, p, &buf);
        if (rc) return rc;
        const int dev0 = c->dev[0];
        hipStream_t st = sh_stream(c->sh[0]);
        rc = measure_run(dev0, st, (const uint4*)buf.p, buf.d_n, 1, (uint32_t)p.emitted, spec, c->measure_cfg, &tot,
                         h.data(), nullptr, &ms, phase);
        HIPCHK_A(hipStreamSynchronize(st));  // (before the buffer goes)
        if (rc) return rc;
    }
    if (out) *out = tot;
    if (hist) std::memcpy(hist, h.data(), (size_t)spec->n_bins * 8);
    c->measure_ms = ms;
    std::copy(phase, phase + MEASURE_PHASES, c->measure_phase_ms);
    return TW_OK;
}

// EVENTS and FIRST: every shard bins the records of its own node block (the
// blocks are disjoint, so a node's first time is one shard's) and the host adds
// the outputs: no gather, no merge.  LATENCY: a pair may span shards, so the
// records are gathered as for tw_lp_measure and binned on the first device.
int tw_lp_measure_series(tw_ctx* c, const tw_series_spec* spec, tw_series_out* total, uint64_t* count,
                         tw_series_stat* stat) {
    if (!c || !spec) return TW_ERR_INVALID;
    for (tw_shard* s : c->sh) {
        int rc = sh_lp_trace_state(s);
        if (rc) return rc;
    }
    if (!series_spec_ok(spec)) return TW_ERR_INVALID;
    const bool is_lat = spec->mode == TW_SERIES_LATENCY;
    if (stat && !is_lat) return TW_ERR_INVALID;
    if (is_lat && c->world != (int)c->sh.size()) return TW_ERR_INVALID;  // a rank of a larger job: no job-wide gather
    std::vector<uint64_t> counts;
    int rc = lp_trace_counts(c, counts);
    if (rc) return rc;
    const LpTracePlan p = lp_trace_plan(counts.data(), counts.size(), c->lp_trace_cap);
    const uint32_t nb = spec->n_bins;
    tw_series_out tot;
    series_empty(&tot);
    std::vector<uint64_t> cnt(nb, 0), sh_cnt(nb);
    std::vector<tw_series_stat> st(stat ? nb : 0);
    for (tw_series_stat& s : st) series_stat_empty(&s);
    double ph[SERIES_PHASES] = {}, sph[SERIES_PHASES];
    if (p.truncated) {
        tot.truncated = 1;  // (contributes nothing else)
    } else if (is_lat && p.emitted) {
        LpGather buf;
        rc = lp_gather(c, p, &buf);
        if (rc) return rc;
        hipStream_t s0 = sh_stream(c->sh[0]);
        rc = series_run(c->dev[0], s0, (const uint4*)buf.p, buf.d_n, 1, (uint32_t)p.emitted, 1u /* no table: not FIRST */,
                        c->series_entries, spec, c->measure_cfg, &tot, cnt.data(), stat ? st.data() : nullptr, nullptr,
                        nullptr, ph);
        HIPCHK_A(hipStreamSynchronize(s0));  // (before the buffer goes)
        if (rc) return rc;
    } else if (!is_lat) {
        for (tw_shard* s : c->sh) {
            tw_series_out sh_tot;
            rc = sh_lp_measure_series(s, spec, c->measure_cfg, c->series_entries, &sh_tot, sh_cnt.data(), sph);
            if (rc) return rc;
            series_combine(&tot, cnt.data(), nullptr, nb, nullptr, nullptr, 0, &sh_tot, sh_cnt.data(), nullptr, nullptr,
                           nullptr, 0, 0);
            for (int i = 0; i < SERIES_PHASES; ++i) ph[i] = std::max(ph[i], sph[i]);
        }
    }
    if (total) *total = tot;
    if (count) std::memcpy(count, cnt.data(), (size_t)nb * 8);
    if (stat) std::memcpy(stat, st.data(), (size_t)nb * sizeof(tw_series_stat));
    std::copy(ph, ph + SERIES_PHASES, c->series_ms);
    return TW_OK;
}

// The whole device window loop of a node-partitioned scenario from t = 0 (after
// tw_reset), over every shard and rank, with the exchange the library owns:
// per tick every shard's event kernel + packing, then the record blocks
// between ranks (RCCL send/recv, or device copies), the import, the
// all-reduce(min) of the window words (RCCL, or a device min), the advance.
// Blocks travel at the size the ranks last agreed on (the largest per-rank
// demand of a tick, rounded up, re-chosen every 16 ticks from the reduced
// words, so every rank picks the same); records beyond it wait a tick in the
// carry buffer.  One host synchronisation per 16 ticks.  A shard that failed
// locally (lrc) stops launching but keeps taking part in the exchange and the
// reduction until the batch's agreement.
int tw_lp_run(tw_ctx* c, uint64_t max_ticks, tw_lp_state* out) {
    if (!c || !out) return TW_ERR_INVALID;
    if (c->comm_broken) return TW_ERR_COMM;
    for (tw_shard* s : c->sh)
        if (!sh_is_lp(s)) return TW_ERR_STATE;
    if (single(c) && c->tp == TP_NONE) {
        // one context, no transport: the shard's own loop
        const uint32_t st2[2] = {c->lp_begin, c->lp_begin + c->lp_count};
        int rc = sh_lp_exchange_setup(c->sh[0], 1, 0, st2, nullptr, nullptr, 0, nullptr);
        if (!rc) rc = sh_lp_loop_begin(c->sh[0]);
        if (!rc) rc = sh_lp_run_windows(c->sh[0], max_ticks, out);
        return rc;
    }
    const size_t n = c->sh.size();
    std::vector<int> lrc(n, TW_OK);  // each shard's first local failure
    auto live = [&](auto f) {        // f on every shard that has not failed
        for (size_t i = 0; i < n; ++i)
            if (!lrc[i]) lrc[i] = f(c->sh[i]);
    };
    int worst = TW_OK;
    int rc = c->lp_ready ? TW_OK : lp_setup(c, lrc);
    if (rc) return rc;
    LpLoop l{c, std::vector<ShardXchg>(n), 0};
    uint32_t cap_eff = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!lrc[i]) lrc[i] = sh_lp_loop_begin(c->sh[i]);
        if (lrc[i]) continue;
        sh_lp_exchange_info(c->sh[i], &l.x[i]);
        cap_eff = lp_first_block(l.x[i].stride);
    }
    live([&](tw_shard* s) { return sh_lp_set_block(s, cap_eff); });
    rc = job_agree(c, lrc, &worst);
    if (rc) return rc;
    if (worst) {
        c->lp_ready = false;  // (set up again by the next call)
        return worst;
    }
    const uint32_t stride = l.x[0].stride;
    l.stride_b = lp_block_bytes(stride);
    const LpTransport& tp = c->tp == TP_RCCL ? LP_RCCL : LP_COPY;
    // testing hook: TW_TEST_FAIL_TICK=shard:tick makes that local shard's
    // launches at that tick fail (TW_ERR_STATE), as a HIP or launch error
    // would -- the other shards and ranks must still leave together
    const LpFailAt fail = lp_parse_fail_tick(getenv("TW_TEST_FAIL_TICK"));
    std::vector<tw_lp_state> st(n);
    for (uint64_t done_ticks = 0; done_ticks < max_ticks;) {
        const uint64_t batch = std::min<uint64_t>(max_ticks - done_ticks, 16);
        const size_t bytes = lp_block_bytes(cap_eff);
        for (uint64_t k = 0; k < batch; ++k) {
            live(sh_lp_tick);
            for (size_t i = 0; i < n; ++i)
                if (!lrc[i] && fail.hit(i, done_ticks + k)) lrc[i] = TW_ERR_STATE;
            rc = tp.blocks(l, bytes);
            if (rc) return rc;
            live(sh_lp_tick_import);
            rc = tp.words(l);
            if (rc) return rc;
            live(sh_lp_tick_end);
        }
        done_ticks += batch;
        bool done = true;
        for (size_t i = 0; i < n; ++i) {
            if (!lrc[i]) lrc[i] = sh_lp_progress(c->sh[i], &st[i]);
            done = done && st[i].done;
        }
        rc = job_agree(c, lrc, &worst);
        if (rc) return rc;
        if (worst) return worst;
        *out = st[0];
        for (size_t i = 1; i < n; ++i) out->err |= st[i].err;
        if (out->err) return TW_ERR_REPLICA;
        if (done) return TW_OK;
        // the largest demand any rank had in one tick is reduced, so every
        // rank picks the same next block
        cap_eff = lp_next_block(sh_lp_xmax(c->sh[0]), stride, cap_eff);
        live([&](tw_shard* s) {
            const int e = sh_lp_set_block(s, cap_eff);
            return e ? e : sh_lp_clear_xmax(s);
        });
    }
    rc = job_agree(c, lrc, &worst);
    if (rc) return rc;
    return worst ? worst : TW_ERR_INCOMPLETE;
}

#ifdef TW_STATS
int tw_prof_read(tw_ctx* c, unsigned long long* out, size_t cap, int reset) {
    if (!c) return TW_ERR_INVALID;
    return sh_prof_read(c->sh[0], out, cap, reset);
}
// device time of the last tw_run's sweep kernels (tools/stats_probe.py)
int tw_sweep_ms(tw_ctx* c, double* ms) {
    if (!c || !ms) return TW_ERR_INVALID;
    return sh_sweep_stats(c->sh[0], nullptr, nullptr, nullptr, ms);
}
#endif

}  // extern "C"
