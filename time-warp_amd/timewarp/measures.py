"""bench/Network measures from emulation traces.

The reference's network bench logs one line per measure event
(`logMeasure`, bench/Network/Common/Bench/Network/Commons.hs:121-171: PingSent
at the sender before `send`, PingReceived and PongSent at the receiver,
PongReceived at the sender) and its LogReader folds them into measures.csv
(bench/Network/LogReader/Main.hs:85-119): one row per message id with the
payload size and the four timestamps, "-" for a missing event, and no row for
an id with a repeated event.  Here the events are the hotspot scenario's
TRACE records (`Engine.trace`, or the oracle's trace log), with virtual time in
µs as the timestamp.
"""
from typing import Dict, Iterable, Tuple

from .scenarios import TAG_PING, TAG_PING_SENT, TAG_PONG, TAG_PONG_SENT

# MeasureEvent in declaration order (Commons.hs:121-127) and its Buildable
# rendering (:129-133), which is the csv header
EVENTS = ("PingSent", "PingReceived", "PongSent", "PongReceived")
EVENT_TEXT = {"PingSent": "• → ", "PingReceived": " → •",
              "PongSent": " ← •", "PongReceived": "• ← "}
TAG_EVENT = {TAG_PING_SENT: "PingSent", TAG_PING: "PingReceived", TAG_PONG_SENT: "PongSent",
             TAG_PONG: "PongReceived"}


def measures_from_trace(records: Iterable[Tuple[int, int, int, int]]) -> Dict[int, Dict[str, int]]:
    """records: (t, node, tag, val) in execution order, val = message id.
    Returns {msg_id: {event: t}}; an id with a repeated event maps to None
    (LogReader's `uniqMap` drops it)."""
    out: Dict[int, Dict[str, int]] = {}
    for t, _node, tag, val in records:
        ev = TAG_EVENT.get(int(tag))
        if ev is None:
            continue
        m = out.setdefault(int(val), {})
        if m is None:
            continue
        if ev in m:
            out[int(val)] = None
            continue
        m[ev] = int(t)
    return out


def format_measures_csv(measures: Dict[int, Dict[str, int]], size: int = 0) -> str:
    """measures.csv as LogReader prints it: rows sorted by id, each cell padded
    on the right to 7, 7, 18, 18, 18, 18 characters and joined with ","."""
    widths = (7, 7) + (18,) * len(EVENTS)

    def row(cells):
        return ",".join(c.ljust(w) for c, w in zip(cells, widths)) + "\n"

    lines = [row(["MsgId", "Size"] + [EVENT_TEXT[e] for e in EVENTS])]
    for mid in sorted(measures):
        m = measures[mid]
        if m is None:
            continue
        lines.append(row([str(mid), str(size)] + [str(m[e]) if e in m else "-" for e in EVENTS]))
    return "".join(lines)


# ------------------------------------------------ host restatement of tw_measure
# (include/timewarp.h).  The yardstick of the GPU pass: plain Python over
# (t, node, tag, val) tuples, no engine call.
_I64_MAX, _I64_MIN = (1 << 63) - 1, -(1 << 63)


def _wrap64(x: int) -> int:
    """x as a two's-complement int64."""
    return ((int(x) + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def pair_latencies(records: Iterable[Tuple[int, int, int, int]], tag_from: int, tag_to: int):
    """One replica's join of `tag_from` and `tag_to` records on equal `val`.
    Returns (latencies, counts): the latency t_to - t_from of every id with
    exactly one record of each tag (in ascending id order), and the class
    counts {"pairs", "open_from", "open_to", "repeated"}; an id with either tag
    more than once is `repeated` and has no latency (LogReader's uniqMap)."""
    if tag_from == tag_to:
        raise ValueError("tag_from and tag_to must differ")
    ids: Dict[int, Tuple[list, list]] = {}
    for t, _node, tag, val in records:
        if int(tag) == tag_from:
            ids.setdefault(int(val), ([], []))[0].append(int(t))
        elif int(tag) == tag_to:
            ids.setdefault(int(val), ([], []))[1].append(int(t))
    counts = {"pairs": 0, "open_from": 0, "open_to": 0, "repeated": 0}
    lat = []
    for val in sorted(ids):
        tf, tt = ids[val]
        if len(tf) > 1 or len(tt) > 1:
            counts["repeated"] += 1
        elif tf and tt:
            counts["pairs"] += 1
            lat.append(_wrap64(tt[0] - tf[0]))
        elif tf:
            counts["open_from"] += 1
        else:
            counts["open_to"] += 1
    return lat, counts


def measure_reference(per_replica_records, emitted, cap: int, spec: dict):
    """tw_measure restated on the host.  per_replica_records[r]: replica r's
    (t, node, tag, val) tuples in execution order (at least its first
    min(emitted[r], cap)); emitted[r]: the records it emitted; cap: the trace
    cap; spec: {"tag_from", "tag_to", "lo_us", "bin_us", "n_bins"}.  Returns
    (total dict, hist uint64[n_bins], per-replica MEASURE_DTYPE array)."""
    import numpy as np

    from .abi import MEASURE_DTYPE

    lo, width, n_bins = int(spec.get("lo_us", 0)), int(spec.get("bin_us", 1)), int(spec.get("n_bins", 1))
    if n_bins < 1 or width < 1:
        raise ValueError("n_bins and bin_us must be >= 1")
    per = np.zeros(len(per_replica_records), MEASURE_DTYPE)
    hist = [0] * n_bins
    under = over = 0
    for r, recs in enumerate(per_replica_records):
        per[r]["min_us"], per[r]["max_us"] = _I64_MAX, _I64_MIN
        if int(emitted[r]) > cap:
            per[r]["truncated"] = 1
            continue
        lat, counts = pair_latencies(list(recs)[:int(emitted[r])], int(spec["tag_from"]), int(spec["tag_to"]))
        for f, v in counts.items():
            per[r][f] = v
        if lat:
            per[r]["min_us"], per[r]["max_us"] = min(lat), max(lat)
        per[r]["sum_us"] = _wrap64(sum(lat))
        for d in lat:
            if d < lo:
                under += 1
            elif (d - lo) // width >= n_bins:
                over += 1
            else:
                hist[(d - lo) // width] += 1
    total = {f: int(per[f].sum()) for f in ("pairs", "open_from", "open_to", "repeated", "truncated")}
    total["underflow"], total["overflow"] = under, over
    total["min_us"] = int(per["min_us"].min()) if len(per) else _I64_MAX
    total["max_us"] = int(per["max_us"].max()) if len(per) else _I64_MIN
    total["sum_us"] = _wrap64(sum(int(x) for x in per["sum_us"]))
    return total, np.array(hist, dtype=np.uint64), per


def quantile_of_sorted(d, q_ppm: int):
    """(lo, hi) of tw_measure_quantiles for the ascending list `d`: with
    pos = q_ppm * (len(d) - 1), lo = d[pos div 10^6] and hi = d[pos div 10^6 +
    (pos mod 10^6 != 0)]; (INT64_MAX, INT64_MIN) for an empty list."""
    if not 0 <= int(q_ppm) <= 1_000_000:
        raise ValueError("q_ppm must be in 0 .. 1,000,000")
    if not d:
        return _I64_MAX, _I64_MIN
    i, rem = divmod(int(q_ppm) * (len(d) - 1), 1_000_000)
    return d[i], d[i + (1 if rem else 0)]


def quantile_reference(per_replica_records, emitted, cap: int, tag_from: int, tag_to: int, q_ppm):
    """tw_measure_quantiles restated on the host, from pair_latencies and
    Python's sorted.  Arguments as measure_reference's, q_ppm a sequence of
    parts per million.  Returns (total, per_replica, pairs, truncated): total a
    list of (lo_us, hi_us) per quantile over all pairs of the batch,
    per_replica an int64 array [replicas][len(q_ppm)][2]; a truncated replica
    contributes to `truncated` alone and its entries are the empty one."""
    import numpy as np

    q_ppm = [int(q) for q in q_ppm]
    per = np.zeros((len(per_replica_records), len(q_ppm), 2), np.int64)
    every, pairs, truncated = [], 0, 0
    for r, recs in enumerate(per_replica_records):
        lat = []
        if int(emitted[r]) > cap:
            truncated += 1
        else:
            lat = sorted(pair_latencies(list(recs)[:int(emitted[r])], int(tag_from), int(tag_to))[0])
        pairs += len(lat)
        every += lat
        for i, q in enumerate(q_ppm):
            per[r, i] = quantile_of_sorted(lat, q)
    every.sort()
    return [quantile_of_sorted(every, q) for q in q_ppm], per, pairs, truncated


def series_reference(per_replica_records, emitted, cap: int, spec: dict):
    """tw_measure_series restated on the host, in plain Python over tuples.
    per_replica_records, emitted, cap: as measure_reference's; spec: {"tag",
    "tag_to" (latency), "mode" ("events", "first" or "latency"), "t0_us",
    "bin_us", "n_bins"}.  Returns (total dict, count uint64[n_bins], stat
    (n_bins, 3) int64 of (sum_us, min_us, max_us) for "latency" else None,
    per-replica SERIES_DTYPE array, per-replica counts uint64
    [replicas][n_bins])."""
    import numpy as np

    from .abi import SERIES_DTYPE

    mode, tag, tag_to = spec.get("mode", "events"), int(spec["tag"]), int(spec.get("tag_to", 0))
    t0, width, n_bins = int(spec.get("t0_us", 0)), int(spec.get("bin_us", 1)), int(spec.get("n_bins", 1))
    if mode not in ("events", "first", "latency"):
        raise ValueError("mode must be events, first or latency")
    if mode == "latency" and tag == tag_to:
        raise ValueError("tag and tag_to must differ")
    if n_bins < 1 or width < 1 or t0 < 0:
        raise ValueError("n_bins and bin_us must be >= 1, t0_us >= 0")
    n = len(per_replica_records)
    per = np.zeros(n, SERIES_DTYPE)
    rows = np.zeros((n, n_bins), np.uint64)
    sums, mins, maxs = [0] * n_bins, [_I64_MAX] * n_bins, [_I64_MIN] * n_bins
    for r, recs in enumerate(per_replica_records):
        per[r]["t_min"], per[r]["t_max"] = _I64_MAX, _I64_MIN
        if int(emitted[r]) > cap:
            per[r]["truncated"] = 1
            continue
        kept = [(int(t), int(node), int(k), int(v)) for t, node, k, v in list(recs)[:int(emitted[r])]]
        if mode == "events":
            items = [(t, None) for t, _node, k, _v in kept if k == tag]
        elif mode == "first":
            first: Dict[int, int] = {}
            for t, node, k, _v in kept:
                if k == tag and (node not in first or t < first[node]):
                    first[node] = t
            items = [(t, None) for t in first.values()]
        else:
            # pair_latencies' pairs, each with the time of its tag_from record
            sides: Dict[int, Tuple[list, list]] = {}
            for t, _node, k, v in kept:
                if k in (tag, tag_to):
                    sides.setdefault(v, ([], []))[k == tag_to].append(t)
            items = [(tf[0], _wrap64(tt[0] - tf[0])) for _v, (tf, tt) in sorted(sides.items())
                     if len(tf) == 1 and len(tt) == 1]
            assert [d for _t, d in items] == pair_latencies(kept, tag, tag_to)[0]   # (both ascend by id)
        for t, d in items:
            per[r]["counted"] += 1
            per[r]["t_min"], per[r]["t_max"] = min(int(per[r]["t_min"]), t), max(int(per[r]["t_max"]), t)
            if t < t0:
                per[r]["underflow"] += 1
            elif (t - t0) // width >= n_bins:
                per[r]["overflow"] += 1
            else:
                b = (t - t0) // width
                rows[r, b] += 1
                if d is not None:
                    sums[b], mins[b], maxs[b] = sums[b] + d, min(mins[b], d), max(maxs[b], d)
    total = {f: int(per[f].sum()) for f in ("counted", "underflow", "overflow", "truncated")}
    total["t_min"] = int(per["t_min"].min()) if n else _I64_MAX
    total["t_max"] = int(per["t_max"].max()) if n else _I64_MIN
    stat = None
    if mode == "latency":
        stat = np.array([[_wrap64(s) for s in sums], mins, maxs], dtype=np.int64).T.copy()
    return total, rows.sum(axis=0, dtype=np.uint64), stat, per, rows


def first_receipts(records, tag: int, lo_us: int = 0, bin_us: int = 1000, n_bins: int = 16):
    """The first-receipt distribution of `tag` (gossip's TAG_RUMOR_FIRST: the
    propagation curve) from canonical records -- LPEngine.lp_trace's, an
    "lpb" Engine.trace's or the oracle's trace log.  A node counts once, at its
    earliest record of the tag.  Returns (times, hist): the nodes' first times
    in ascending order (int64) and the uint64 counts of the bins
    [lo_us + i * bin_us, lo_us + (i + 1) * bin_us); times outside the bins are
    in `times` only."""
    import numpy as np

    if n_bins < 1 or bin_us < 1:
        raise ValueError("n_bins and bin_us must be >= 1")
    first: Dict[int, int] = {}
    for t, node, k, _val in trace_tuples(records):
        if k == int(tag) and (node not in first or t < first[node]):
            first[node] = t
    times = np.array(sorted(first.values()), dtype=np.int64)
    hist = np.zeros(n_bins, np.uint64)
    for t in times:
        b = (int(t) - int(lo_us)) // int(bin_us)
        if 0 <= b < n_bins:
            hist[b] += 1
    return times, hist


def trace_tuples(recs) -> list:
    """Engine.trace records (TRACE_DTYPE) or oracle traces -> (t, node, tag, val) tuples."""
    if hasattr(recs, "dtype"):
        return [(int(r["t"]), int(r["node"]), int(r["tag"]), int(r["val"])) for r in recs]
    return [(int(t), int(n), int(k), int(v)) for t, n, k, v in recs]
