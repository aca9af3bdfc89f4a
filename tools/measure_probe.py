"""tw_measure against the host path on a hotspot batch: the round-trip latency
TAG_PING_SENT -> TAG_PONG of senders x messages x replicas, joined and reduced
on the GPU (Engine.measure), and the same join done the old way -- one
tw_read_trace per replica plus measures_from_trace in the interpreter -- timed
on a sample of replicas and scaled to the batch (an extrapolation).  The
device's per-replica entries of the sample must equal measure_reference.

--geometry lpb runs the batch in the batched logical-process mode (a power of
two of at most 32768 replicas per GPU): its traced run keeps every due record on
the node's chain (tw_lp_batch is off while tracing is on) unless --trace-batch
turns Engine.set_trace_batch on, and Engine.trace returns a replica's records in
canonical order, so the host sample is compared as sorted tuples.

--max-keys N raises the context's key limit (Engine.set_measure_keys): replicas
with more than 2,048 keys of the round trip (senders x messages > 1,024) then
take the partition path, and every call's line is followed by the kernels' time
by phase with the bytes each phase moves by design (records scanned x 32 B, keys
written or read x 16 B; a model, not a counter).  The reference bench's own
message count: --senders 256 --msgs 1000 --replicas 256 --geometry lpb
--max-keys 524288 --host-sample 2.

--quantiles adds Engine.measure_quantiles on the same run: p50 / p99 / p99.9 of
the round trip, batch-wide and per replica, with the call's device time by phase
(the join with its emit, the offsets scan, the per-replica select, the
batch-wide digit passes) beside tw_measure's; the sampled replicas' entries and,
when the whole batch is sampled, the total must equal quantile_reference.

--series adds Engine.measure_series on the same run: the Pong curve (events),
the senders' first Pongs (first) and the round trip by send time (latency: the
mean and the largest latency of every send-time bin, which is where a hotspot's
growing backlog shows), each with the call's device time by phase; the sampled
replicas' per-replica entries and rows must equal series_reference.

--config gossip [--nodes 1048576] [--shards 1] is another run altogether: a
traced node-partitioned gossip run (LPEngine, lp_set_trace), whose propagation
curve -- every node's first receipt, TAG_RUMOR_FIRST -- is binned on the device
(LPEngine.lp_measure_series) and, on the same run, by the host path it replaces:
lp_trace() plus measures.first_receipts.  The two curves must be equal.

usage: python tools/measure_probe.py [--senders 8] [--msgs 40] [--replicas 65536] [--geometry lpb]
                                     [--trace-batch] [--max-keys N] [--host-sample 256] [--quantiles]
                                     [--series] [--config gossip [--nodes N] [--shards K]]
                                     [--out profiles/measure/probe.log]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "time-warp_amd"))
from timewarp import scenarios  # noqa: E402
from timewarp.engine import Engine, LPEngine, draw_link_table, lp_scenario  # noqa: E402
from timewarp.measures import (first_receipts, measure_reference, measures_from_trace, quantile_reference,  # noqa: E402
                               series_reference, trace_tuples)
from timewarp.scenarios import TAG_PING_SENT, TAG_PONG, TAG_RUMOR_FIRST  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--senders", type=int, default=8)
ap.add_argument("--msgs", type=int, default=40)
ap.add_argument("--replicas", type=int, default=65536)
ap.add_argument("--host-sample", type=int, default=256)
ap.add_argument("--max-keys", type=int, default=0, help="Engine.set_measure_keys (default: the library's 2048)")
ap.add_argument("--geometry", default=None, help="Engine.load's geometry (default: the library's choice)")
ap.add_argument("--trace-batch", action="store_true",
                help="lpb: the traced run with Engine.set_trace_batch on (tw_lp_batch<true> records the due runs)")
ap.add_argument("--quantiles", action="store_true", help="also Engine.measure_quantiles: p50 / p99 / p99.9")
ap.add_argument("--series", action="store_true",
                help="also Engine.measure_series: the Pong curve, first Pongs and the round trip by send time")
ap.add_argument("--config", default="hotspot", choices=("hotspot", "gossip"),
                help="gossip: the propagation curve of a traced node-partitioned run, device series against lp_trace()")
ap.add_argument("--nodes", type=int, default=1 << 20, help="--config gossip: nodes")
ap.add_argument("--shards", type=int, default=1, help="--config gossip: shards of GPU 0 the nodes are split over")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure", "probe.log"))
a = ap.parse_args()
if a.trace_batch and a.geometry != "lpb":
    ap.error("--trace-batch needs --geometry lpb")

S, M, R = a.senders, a.msgs, a.replicas
cap = 4 * S * M  # four measure events per message
spec = dict(tag_from=TAG_PING_SENT, tag_to=TAG_PONG, lo_us=2000, bin_us=250, n_bins=40)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def say_phases(e):
    """The last measure()'s kernels by phase, when the partition path ran."""
    ph = e.measure_phases_ms()
    if not ph["join_large"]:
        return
    rec, key = cap * R * 32, 2 * S * M * R * 16   # every record is kept; two of a message's four are keys
    moved = {"count": (rec, 0), "part_count": (rec, 0), "part_scatter": (rec, key), "join_large": (key, 0)}
    for k, ms in ph.items():
        rd, wr = moved.get(k, (0, 0))
        rate = f", reads {rd / 1e9:.2f} GB, writes {wr / 1e9:.2f} GB: {(rd + wr) / ms / 1e6:.0f} GB/s" if rd and ms else ""
        say(f"    {k:12s} {ms:9.3f} ms{rate}")


def gossip_probe():
    """The propagation curve of a traced node-partitioned gossip run: the device
    series (every shard bins its own nodes' TAG_RUMOR_FIRST records) beside the
    host path it replaces, lp_trace() -- gather, sort and k-way merge of every
    shard's records -- plus first_receipts, on the same run."""
    N, k = a.nodes, a.shards
    t0 = time.perf_counter()
    scn = scenarios.gossip(n_nodes=N, seed=0)
    say(f"gossip {N} nodes over {k} shard(s) of one GPU; scenario built in {time.perf_counter() - t0:.1f} s")
    curve = dict(t0_us=1_000_000, bin_us=2000, n_bins=32)
    with LPEngine(lp_scenario(scn), 0, N, int(scn.meta["lookahead_us"]), devices=[0] * k) as e:
        e.lp_set_trace(N + 1024)
        e.reset()
        e.run_lp()
        e.reset()                 # (every timed run is a second one)
        t0 = time.perf_counter()
        st = e.run_lp()
        say(f"traced run: {(time.perf_counter() - t0) * 1e3:.1f} ms wall, done {st.done}")
        for mode in ("first", "events"):
            for i in range(3):
                t0 = time.perf_counter()
                tot, count, _stat = e.lp_measure_series(TAG_RUMOR_FIRST, mode=mode, **curve)
                wall = (time.perf_counter() - t0) * 1e3
                ph = e.measure_series_ms()
                say(f"tw_lp_measure_series {mode} call {i}: wall {wall:.2f} ms; device: table fill {ph['first_fill']:.3f} ms, "
                    f"binning {ph['bin']:.3f} ms (the slowest shard's)")
            say(f"  {mode}: {tot}")
            say(f"  count[{curve['t0_us']} + i * {curve['bin_us']} us] {count.tolist()}")
            if mode == "first":
                first = (tot, count)
        for i in range(2):
            t0 = time.perf_counter()
            recs, emitted = e.lp_trace(cap=N + 1024)
            t1 = time.perf_counter()
            times, hist = first_receipts(recs, TAG_RUMOR_FIRST, lo_us=curve["t0_us"], bin_us=curve["bin_us"],
                                         n_bins=curve["n_bins"])
            t2 = time.perf_counter()
            say(f"host path call {i}: lp_trace {(t1 - t0) * 1e3:.1f} ms ({emitted} records, {len(recs) * 24 / 2**20:.1f} MiB "
                f"handed out) + first_receipts {(t2 - t1) * 1e3:.1f} ms = {(t2 - t0) * 1e3:.1f} ms")
        tot, count = first
        assert np.array_equal(hist, count) and tot["counted"] == len(times) and tot["truncated"] == 0
        assert (tot["t_min"], tot["t_max"]) == (int(times[0]), int(times[-1]))
        say(f"the device curve equals first_receipts over lp_trace(): {tot['counted']} nodes reached, "
            f"{tot['t_min']} .. {tot['t_max']} us")


if a.config == "gossip":
    gossip_probe()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0)

scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M, drawer=draw_link_table)
with Engine(0) as e:
    e.load(scn, geometry=a.geometry)
    if a.max_keys:
        e.set_measure_keys(a.max_keys)
    if a.geometry == "lpb":  # what tracing costs there: the same batch untraced, tw_lp_batch on
        e.reset().run()      # (every timed run is a second one: the first loads code and captures the tick graph)
        e.reset()
        st = e.run()
        batched, due = e.lpb_batch()
        say(f"lpb untraced: event kernels {st.kernel_ms:.1f} ms, tw_run wall {st.wall_ms:.1f} ms; {due} due records, "
            f"{batched} of them run by tw_lp_batch")
    e.set_trace(cap)
    if a.trace_batch:
        e.set_trace_batch(True)
    e.reset().run()
    e.reset()
    st = e.run()
    say(f"hotspot {S} senders x {M} messages x {R} replicas, geometry {e.geometry()}: {st.events} events, "
        f"event kernels {st.kernel_ms:.1f} ms, tw_run wall {st.wall_ms:.1f} ms; {cap * R} trace records "
        f"({cap * R * 32 / 2**30:.2f} GiB)")
    if a.geometry == "lpb":
        batched, due = e.lpb_batch()
        how = "tw_lp_batch<true>: set_trace_batch on" if a.trace_batch else "off while tracing is on"
        say(f"lpb: {due} due records, {batched} of them run by tw_lp_batch ({how})")
    # device path: every replica, with the per-replica array
    for i in range(3):
        t0 = time.perf_counter()
        total, hist, per = e.measure(spec["tag_from"], spec["tag_to"], spec["lo_us"], spec["bin_us"], spec["n_bins"],
                                     per_replica=True)
        wall = (time.perf_counter() - t0) * 1e3
        say(f"tw_measure call {i}: wall {wall:.2f} ms, kernels {e.measure_ms():.3f} ms (HIP events); the rest, "
            f"{wall - e.measure_ms():.2f} ms, is the call's scratch allocation and release, two host reads and the copy out")
        say_phases(e)
    t0 = time.perf_counter()
    e.measure(spec["tag_from"], spec["tag_to"], spec["lo_us"], spec["bin_us"], spec["n_bins"])
    say(f"tw_measure without per_replica: wall {(time.perf_counter() - t0) * 1e3:.2f} ms, "
        f"kernels {e.measure_ms():.3f} ms")
    say(f"total {total}")
    if a.quantiles:
        qs = (500000, 990000, 999000)

        def say_quantiles(what, wall):
            ph = e.measure_quantiles_ms()
            dev = ph["join_emit"] + ph["offsets"] + ph["select_replicas"] + ph["select_total"]
            say(f"tw_measure_quantiles {what}: wall {wall:.2f} ms, device {dev:.3f} ms = join with emit "
                f"{ph['join_emit']:.3f} + offsets {ph['offsets']:.3f} + per-replica select {ph['select_replicas']:.3f} + "
                f"batch select {ph['select_total']:.3f} ({int(ph['total_passes'])} digit passes)")

        for i in range(3):
            t0 = time.perf_counter()
            qtot, qper, qpairs, qtrunc = e.measure_quantiles(spec["tag_from"], spec["tag_to"], qs, per_replica=True)
            say_quantiles(f"call {i}", (time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        qtot2, _, _, _ = e.measure_quantiles(spec["tag_from"], spec["tag_to"], qs)
        say_quantiles("without per_replica", (time.perf_counter() - t0) * 1e3)
        assert qtot2.tobytes() == qtot.tobytes() and (qpairs, qtrunc) == (total["pairs"], total["truncated"])
        for q, v in zip(qs, qtot):
            say(f"  p{q / 1e4:g}: lo {int(v['lo_us'])} us, hi {int(v['hi_us'])} us")
        # the histogram brackets every quantile's bin
        edges = np.concatenate([[0], np.cumsum(hist)])
        for q, v in zip(qs, qtot):
            b = (int(v["lo_us"]) - spec["lo_us"]) // spec["bin_us"]
            if total["underflow"] == 0 and 0 <= b < spec["n_bins"]:
                assert edges[b] <= q * (qpairs - 1) // 1000000 < edges[b + 1], (q, b)
    if a.series:
        # 16 bins over the run: the sends are 1 ms apart from 1 ms on, the Pongs follow 4 .. 9 ms behind
        width = max((M + 12) * 1000 // 16, 1)
        series = {"pong curve": dict(tag=TAG_PONG, mode="events", t0_us=0, bin_us=width, n_bins=16),
                  "first pongs": dict(tag=TAG_PONG, mode="first", t0_us=0, bin_us=width, n_bins=16),
                  "round trip by send time": dict(tag=TAG_PING_SENT, tag_to=TAG_PONG, mode="latency", t0_us=0,
                                                  bin_us=width, n_bins=16)}
        series_got = {}
        for what, sp in series.items():
            kw = dict(t0_us=sp["t0_us"], bin_us=sp["bin_us"], n_bins=sp["n_bins"], mode=sp["mode"], tag_to=sp.get("tag_to", 0))
            for per_replica in (True, True, True, False):
                t0 = time.perf_counter()
                got = e.measure_series(sp["tag"], per_replica=per_replica, **kw)
                wall = (time.perf_counter() - t0) * 1e3
                ph = e.measure_series_ms()
                say(f"tw_measure_series {what}{'' if per_replica else ' without per_replica'}: wall {wall:.2f} ms, device "
                    f"{sum(ph.values()):.3f} ms = join with emit {ph['join_emit']:.3f} + table fill {ph['first_fill']:.3f} + "
                    f"binning {ph['bin']:.3f} + latency fold {ph['latency_fold']:.3f}")
                if per_replica:
                    series_got[what] = got
                else:
                    assert got[0] == series_got[what][0] and np.array_equal(got[1], series_got[what][1])
            stot, scount, sstat = series_got[what][:3]
            say(f"  {stot}")
            say(f"  count[i * {width} us] {scount.tolist()}")
            if sstat is not None:
                mean = [int(s) // int(c) if c else None for s, c in zip(sstat["sum_us"], scount)]
                say(f"  mean round trip by send-time bin (us) {mean}")
                say(f"  max  round trip by send-time bin (us) {[int(x) if c else None for x, c in zip(sstat['max_us'], scount)]}")
                assert stot["counted"] == total["pairs"]
    say(f"hist[{spec['lo_us']} + i * {spec['bin_us']} us] {hist.tolist()}")
    assert total["pairs"] == S * M * R and total["truncated"] == 0, total

    # host path on a sample: Engine.trace + measures_from_trace per replica
    n = min(a.host_sample, R)
    sample = np.linspace(0, R - 1, n).astype(np.int64)
    recs, emitted = [], []
    t0 = time.perf_counter()
    for r in sample:
        rr, em = e.trace(int(r), cap=cap)
        tup = sorted(trace_tuples(rr))  # (lpb: canonical order already; the join does not depend on order)
        ms = measures_from_trace(tup)
        lat = [m["PongReceived"] - m["PingSent"] for m in ms.values() if m and "PongReceived" in m and "PingSent" in m]
        recs.append(tup)
        emitted.append(em)
    host = time.perf_counter() - t0
    say(f"host path (Engine.trace + measures_from_trace) on {n} replicas: {host * 1e3:.1f} ms = "
        f"{host / n * 1e3:.3f} ms per replica; scaled to {R} replicas (extrapolated): {host / n * R:.1f} s")
    rtot, _rhist, rper = measure_reference(recs, emitted, cap, spec)
    for f in per.dtype.names:
        assert np.array_equal(per[f][sample], rper[f]), f
    for f in ("pairs", "open_from", "open_to", "repeated", "truncated"):
        assert int(per[f][sample].sum()) == rtot[f], f
    assert int(per["min_us"][sample].min()) == rtot["min_us"] and int(per["max_us"][sample].max()) == rtot["max_us"]
    assert int(per["sum_us"][sample].sum()) == rtot["sum_us"]
    say(f"device per_replica entries of the {n} sampled replicas equal measure_reference: "
        f"pairs {rtot['pairs']}, min {rtot['min_us']}, max {rtot['max_us']}, sum {rtot['sum_us']}")
    if a.quantiles:
        wtot, wper, _, _ = quantile_reference(recs, emitted, cap, spec["tag_from"], spec["tag_to"], qs)
        assert np.array_equal(qper["lo_us"][sample], wper[:, :, 0]) and np.array_equal(qper["hi_us"][sample], wper[:, :, 1])
        if n == R:
            assert qtot.tolist() == [tuple(x) for x in wtot]
        say(f"device per-replica quantiles of the {n} sampled replicas equal quantile_reference"
            + ("; so does the batch's" if n == R else ""))
    if a.series:
        for what, sp in series.items():
            _t, _c, _s, wper, wrows = series_reference(recs, emitted, cap, sp)
            _tot, _count, _stat, sper, srows = series_got[what]
            assert sper[sample].tobytes() == wper.tobytes() and np.array_equal(srows[sample], wrows), what
        say(f"device per-replica series of the {n} sampled replicas equal series_reference")

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
