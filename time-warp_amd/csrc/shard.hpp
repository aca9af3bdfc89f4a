// shard.hpp — one device's engine context (engine.hip) as seen by the public
// C ABI (abi.hip).  A tw_ctx (include/timewarp.h) holds one shard per device
// of this process; each shard is the single-device engine of rounds 1-2: one
// HIP device, one stream, its replicas (or logical processes) in HBM.  These
// entry points are internal to libtimewarp.so (hidden symbols).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/timewarp.h"

struct tw_shard;

namespace tw {

#define TW_HIDDEN __attribute__((visibility("hidden")))

TW_HIDDEN int sh_create(int device, tw_shard** out);
TW_HIDDEN void sh_destroy(tw_shard* c);
TW_HIDDEN int sh_load(tw_shard* c, const tw_scenario_desc* s);
TW_HIDDEN int sh_lp_load(tw_shard* c, const tw_scenario_desc* s, uint32_t lp_begin, uint32_t lp_count,
                         int64_t lookahead_us, uint32_t inbox_cap, uint32_t outbox_cap);
TW_HIDDEN int sh_lpb_load(tw_shard* c, const tw_scenario_desc* s, int64_t lookahead_us, const uint32_t* node_inbox_cap,
                          uint32_t inbox_cap, uint32_t outbox_cap);
TW_HIDDEN int sh_reset(tw_shard* c);
TW_HIDDEN int sh_run(tw_shard* c, int64_t t_end_us, uint64_t max_events, tw_stats* out);
TW_HIDDEN int sh_read_results(tw_shard* c, tw_replica_result* out, size_t n);
TW_HIDDEN int sh_read_hashes(tw_shard* c, uint64_t* out, size_t n);
TW_HIDDEN int sh_tie_audit(tw_shard* c, int64_t t_end_us, uint64_t max_events, uint32_t probes, tw_stats* out);
TW_HIDDEN int sh_geometry(tw_shard* c);
TW_HIDDEN int sh_set_counter_base(tw_shard* c, uint32_t seq0, uint32_t tid0);
TW_HIDDEN int sh_set_tie_mode(tw_shard* c, uint32_t mode);
// killThread sweeps (sweep.hip): the switch, and the last sh_run's counts with
// the sweep kernels' device time
TW_HIDDEN int sh_set_sweep(tw_shard* c, int on);
TW_HIDDEN int sh_sweep_stats(tw_shard* c, uint64_t* killers, uint64_t* victims, uint64_t* refused, double* ms);
TW_HIDDEN int sh_sweep_path_stats(tw_shard* c, uint64_t* terminal, uint64_t* fast, uint64_t* slow);
// the send-free prefix (prefix.hip): the switch; the image's T0, the cached
// snapshot's events and bytes per replica (0: none), what the last sh_run did
// (TW_PREFIX_*) and its apply's device time
TW_HIDDEN int sh_set_prefix(tw_shard* c, int on);
TW_HIDDEN int sh_prefix_stats(tw_shard* c, int64_t* t0, uint64_t* events, uint64_t* bytes, uint32_t* last, double* ms);
// rows the apply leaves unstored (prefix_clean.hpp): the snapshot's claimed
// slots, the last sh_run's apply (rows skipped, bytes stored per replica),
// whether that run verified, the testing hook's mismatch count
TW_HIDDEN int sh_prefix_clean_stats(tw_shard* c, uint32_t* claimed, uint64_t* rows_skipped, uint64_t* bytes_stored,
                                    uint32_t* verified, uint64_t* audit);
// ... and per row class of §3v: the last apply's skipped rows and bytes, the snapshot's classification
TW_HIDDEN int sh_prefix_rows_stats(tw_shard* c, tw_prefix_rows* out);
// live delays (tw_set_live_delays): desc = live_plan.hpp's descriptors of the
// loaded links (null: off), seed0 = the seed of the shard's first replica;
// TW_ERR_INVALID for a node-partitioned or batched LP shard.  sh_live_stats:
// the shard's generator steps since the last reset
struct LiveLink;
TW_HIDDEN int sh_set_live(tw_shard* c, const LiveLink* desc, int64_t seed0);
TW_HIDDEN int sh_live_stats(tw_shard* c, uint64_t* draws);
TW_HIDDEN int sh_set_trace(tw_shard* c, uint32_t cap);
// batched LP, tracing on: tw_lp_batch<true> runs the due runs' batchable prefixes
// and records their TRACEs (off: they stay on the chain); from the next sh_reset
TW_HIDDEN int sh_set_trace_batch(tw_shard* c, int on);
TW_HIDDEN int sh_read_trace(tw_shard* c, uint32_t replica, tw_trace_rec* out, size_t cap, uint64_t* n_emitted);
// tw_measure on one shard: sh_measure_state is its state check alone
// (TW_ERR_STATE nothing loaded / tracing off, TW_ERR_INVALID node-partitioned
// contexts and batched LP contexts with tracing off);
// sh_measure writes total, hist[n_bins] (or NULL), per[sh_replicas] (or NULL)
// and the kernels' device time (phase_ms: MEASURE_PHASES entries or NULL)
// only on success.  MeasureCfg is the context's setting (tw_set_measure_keys)
// with the testing hook's two values (TW_TEST_MEASURE; abi.hip)
TW_HIDDEN int sh_measure_state(tw_shard* c);
struct MeasureCfg {
    uint32_t max_keys;     // matching records a non-truncated replica may hold
    uint32_t lds_keys;     // replicas with more take the partition path (TW_MEASURE_MAX_KEYS but under the hook)
    uint32_t bucket_keys;  // mean keys per bucket (1024 but under the hook)
};
// tw_measure's kernels in launch order of their kind: count, plan,
// part<false>, ranges, part<true>, join, join_large
constexpr int MEASURE_PHASES = 7;
// tw_measure_quantiles: the join's emit variant leaves every pair's latency in
// device memory, segmented by replica -- replica r's are lat[off[r] ..
// off[r] + fill[r]), its segment of off[r + 1] - off[r] places filled from the
// front in no particular order.  Made by sh_measure / measure_run when `emit`
// is given (no histogram is counted then; hist and the under / overflow read
// 0), owned by the caller whatever they return: measure_emit_free.
struct MeasureEmit {
    void* buf = nullptr;               // off[R + 1] | digits[32 x 256] | fill[R]
    unsigned long long* off = nullptr;
    unsigned long long* digits = nullptr;  // select_count's device histogram
    uint32_t* fill = nullptr;
    long long* lat = nullptr;
    // tw_measure_series' LATENCY mode sets with_t before the call: every pair's
    // t_from is then stored as well, at its latency's place (tfrom: the second
    // half of lat's allocation)
    bool with_t = false;
    long long* tfrom = nullptr;
    uint64_t places = 0;               // off[R]
    double offsets_ms = 0.0;           // device time of the offsets scan
};
TW_HIDDEN void measure_emit_free(MeasureEmit* e);
TW_HIDDEN int sh_measure(tw_shard* c, const tw_measure_spec* spec, const MeasureCfg& cfg, tw_measure_out* total,
                         uint64_t* hist, tw_measure_out* per, double* kernel_ms, double* phase_ms,
                         MeasureEmit* emit = nullptr);
// the measure pass itself (measure.hip) over a shard's trace buffer
// ([cap][R][2] quads) and its per-replica emitted counts (R: replicas)
TW_HIDDEN int measure_run(int device, hipStream_t stream, const uint4* trace, const uint64_t* emitted, uint32_t R,
                          uint32_t cap, const tw_measure_spec* spec, const MeasureCfg& cfg, tw_measure_out* total,
                          uint64_t* hist, tw_measure_out* per, double* kernel_ms, double* phase_ms,
                          MeasureEmit* emit = nullptr);
// the selects over a MeasureEmit of R replicas (measure_select.hip), blocking:
// select_replicas writes out[R][n_q] (host), a replica at a time per workgroup
// -- sorted in LDS up to lds_cap latencies (at most QS_LDS_MAX), radix-selected
// beyond; select_count adds to hist[n_ranks][256] (host) the digit at `shift`
// of every latency of the shard whose key matches prefix[j] above it.
constexpr uint32_t QS_LDS_MAX = 2048;
TW_HIDDEN int select_replicas(int device, hipStream_t stream, const MeasureEmit& e, uint32_t R, const uint32_t* q_ppm,
                              uint32_t n_q, uint32_t lds_cap, tw_quantile* out, double* ms);
TW_HIDDEN int select_count(int device, hipStream_t stream, const MeasureEmit& e, uint32_t R, const uint64_t* prefix,
                           uint32_t n_ranks, uint32_t shift, uint64_t* hist, double* ms);
// tw_measure_series on one shard (measure_series.hip): the states of
// sh_measure_state; outputs (any may be NULL: total, count[n_bins],
// stat[n_bins], per[sh_replicas], per_count[sh_replicas][n_bins]) and the
// device time by phase (SERIES_PHASES entries, measure_series.hpp) written only
// on success.  max_entries: FIRST's table entries at a time (0: the limit).
// sh_lp_measure_series: EVENTS / FIRST over the node block of one shard of a
// traced node-partitioned context, its one replica (states: sh_lp_trace_state).
// series_run is the pass itself over a trace buffer, as measure_run.
TW_HIDDEN int sh_measure_series(tw_shard* c, const tw_series_spec* spec, const MeasureCfg& cfg, uint64_t max_entries,
                                tw_series_out* total, uint64_t* count, tw_series_stat* stat, tw_series_out* per,
                                uint64_t* per_count, double* phase_ms);
TW_HIDDEN int sh_lp_measure_series(tw_shard* c, const tw_series_spec* spec, const MeasureCfg& cfg, uint64_t max_entries,
                                   tw_series_out* total, uint64_t* count, double* phase_ms);
TW_HIDDEN int series_run(int device, hipStream_t stream, const uint4* trace, const uint64_t* emitted, uint32_t R,
                         uint32_t cap, uint32_t n_nodes, uint64_t max_entries, const tw_series_spec* spec,
                         const MeasureCfg& cfg, tw_series_out* total, uint64_t* count, tw_series_stat* stat,
                         tw_series_out* per, uint64_t* per_count, double* phase_ms);
// tw_lp_set_trace ... on one shard of a node-partitioned context: the shard
// keeps up to cap records of its node block under one counter.
// sh_lp_trace_state: TW_ERR_STATE nothing loaded / tracing off, TW_ERR_INVALID
// any other kind of context; sh_lp_trace_count synchronises the shard's stream
// and reads the emitted count; sh_lp_trace_fetch copies the first k (<= cap)
// records out in claim order; sh_lp_trace_dev / sh_stream: what the gather of
// tw_lp_measure copies from, and the stream it is ordered on
TW_HIDDEN int sh_lp_kind(tw_shard* c);  // TW_OK: a loaded node-partitioned shard
TW_HIDDEN int sh_lp_trace_state(tw_shard* c);
TW_HIDDEN int sh_lp_set_trace(tw_shard* c, uint32_t cap);
TW_HIDDEN int sh_lp_trace_count(tw_shard* c, uint64_t* n);
TW_HIDDEN int sh_lp_trace_fetch(tw_shard* c, tw_trace_rec* out, size_t k);
TW_HIDDEN const uint4* sh_lp_trace_dev(tw_shard* c);
TW_HIDDEN hipStream_t sh_stream(tw_shard* c);
TW_HIDDEN int sh_last_launch_ms(tw_shard* c, double* out, size_t cap);
TW_HIDDEN int sh_prof_read(tw_shard* c, unsigned long long* out, size_t cap, int reset);
// shape of what a shard holds: replicas its results cover (batched LP: the
// replica count, not the lanes), nodes per replica, LP node range
TW_HIDDEN uint32_t sh_replicas(tw_shard* c);
TW_HIDDEN uint32_t sh_nodes(tw_shard* c);
TW_HIDDEN bool sh_is_lp(tw_shard* c);
TW_HIDDEN bool sh_loaded(tw_shard* c);
TW_HIDDEN uint32_t sh_links(tw_shard* c);  // links of the loaded scenario
TW_HIDDEN int sh_device(tw_shard* c);

// node-partitioned (LP) mode
TW_HIDDEN int sh_lp_window(tw_shard* c, int64_t t_end_excl, int64_t* next_t, uint64_t* n_foreign);
TW_HIDDEN int sh_lp_take_outbox(tw_shard* c, tw_lp_record* out, size_t cap, size_t* n);
TW_HIDDEN int sh_lp_inject(tw_shard* c, const tw_lp_record* recs, size_t n, int64_t* next_t);
TW_HIDDEN int sh_lp_results(tw_shard* c, tw_replica_result* agg, uint64_t* node_hashes, size_t n_nodes);
TW_HIDDEN int sh_lpb_windows(tw_shard* c, uint64_t* windows, uint64_t* ticks);
TW_HIDDEN int sh_lpb_batch(tw_shard* c, uint64_t* batched, uint64_t* due);
TW_HIDDEN int sh_set_stream(tw_shard* c, void* hip_stream);
TW_HIDDEN int sh_lp_exchange_setup(tw_shard* c, uint32_t world, uint32_t rank, const uint32_t* starts, void* send,
                                   void* recv, uint32_t cap, int64_t* red);
TW_HIDDEN int sh_lp_loop_begin(tw_shard* c);
TW_HIDDEN int sh_lp_tick(tw_shard* c);
TW_HIDDEN int sh_lp_tick_import(tw_shard* c);
TW_HIDDEN int sh_lp_tick_end(tw_shard* c);
TW_HIDDEN int sh_lp_progress(tw_shard* c, tw_lp_state* out);
TW_HIDDEN int sh_lp_run_windows(tw_shard* c, uint64_t max_ticks, tw_lp_state* out);

// the library-driven exchange (abi.hip): library-owned blocks of `cap`
// records per rank, of which the first cap_eff travel each tick
struct ShardXchg {
    int device;
    hipStream_t stream;
    void* send;       // world blocks of (stride + 1) x 32 B: header + records
    void* recv;
    int64_t* red;     // RD_COUNT words, all-reduced with MIN
    uint32_t world, stride, cap_eff;
};
TW_HIDDEN int sh_lp_exchange_own(tw_shard* c, uint32_t world, uint32_t rank, const uint32_t* starts, uint32_t cap);
TW_HIDDEN void sh_lp_exchange_info(tw_shard* c, ShardXchg* x);
TW_HIDDEN int sh_lp_set_block(tw_shard* c, uint32_t cap_eff);
TW_HIDDEN int64_t sh_lp_xmax(tw_shard* c);
TW_HIDDEN int sh_lp_clear_xmax(tw_shard* c);

}  // namespace tw
