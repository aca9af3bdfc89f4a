"""ctypes mirror of include/timewarp.h structs (no torch types cross the ABI)."""
from __future__ import annotations

import ctypes as C

from . import isa


class TwScenarioDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_replicas", C.c_uint32),
        ("n_nodes", C.c_uint32),
        ("n_insns", C.c_uint32),
        ("insns", C.c_void_p),
        ("n_consts", C.c_uint32),
        ("consts", C.c_void_p),
        ("main_pc", C.c_uint32),
        ("main_node", C.c_uint32),
        ("n_listener_sets", C.c_uint32),
        ("n_msg_kinds", C.c_uint32),
        ("listener_pc", C.c_void_p),
        ("n_links", C.c_uint32),
        ("out_off", C.c_void_p),
        ("link_dst", C.c_void_p),
        ("link_rev", C.c_void_p),
        ("link_depth", C.c_uint32),
        ("link_table", C.c_void_p),
        ("node_vars", C.c_void_p),
        ("main_regs", C.c_void_p),
        ("node_listen", C.c_void_p),
        ("max_slots", C.c_uint32),
        ("queue_capacity", C.c_uint32),
        ("near_horizon_us", C.c_int64),
        ("max_timeouts", C.c_uint32),
        ("run_capacity", C.c_uint32),
        ("max_frames", C.c_uint32),
        ("msg_bytes", C.c_void_p),
        ("link_bw", C.c_void_p),
    ]


class TwReplicaResult(C.Structure):
    _fields_ = [
        ("final_t", C.c_int64),
        ("events", C.c_uint64),
        ("delivered", C.c_uint64),
        ("dropped", C.c_uint64),
        ("undeliverable", C.c_uint64),
        ("status", C.c_uint32),
        ("main_exc", C.c_uint32),
        ("threads", C.c_uint64),
        ("tie_flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class TwStats(C.Structure):
    _fields_ = [
        ("events", C.c_uint64),
        ("sends", C.c_uint64),
        ("delivered", C.c_uint64),
        ("dropped", C.c_uint64),
        ("undeliverable", C.c_uint64),
        ("max_final_t", C.c_int64),
        ("replicas_done", C.c_uint32),
        ("replicas_error", C.c_uint32),
        ("launches", C.c_uint32),
        ("reserved", C.c_uint32),
        ("kernel_ms", C.c_double),
        ("wall_ms", C.c_double),
    ]


# the fields a run produces (tie_flags is set by tw_tie_audit only)
class TwLpState(C.Structure):
    """tw_lp_state: the device-driven window loop's progress."""
    _fields_ = [
        ("windows", C.c_uint64),
        ("ticks", C.c_uint64),
        ("t", C.c_int64),
        ("done", C.c_uint32),
        ("err", C.c_uint32),
    ]


class TwTableDraw(C.Structure):
    """tw_table_draw: a link-table draw on the GPU (tw_draw_link_table)."""
    _fields_ = [
        ("n_links", C.c_uint32),
        ("link_depth", C.c_uint32),
        ("n_replicas", C.c_uint32),
        ("drop_log2", C.c_int32),
        ("seed_base", C.c_int64),
        ("drawn", C.c_void_p),
        ("lo", C.c_void_p),
        ("hi", C.c_void_p),
    ]


class TwLiveDelays(C.Structure):
    """tw_live_delays: per-link kind / lo / hi and the batch's seed base."""
    _fields_ = [
        ("kind", C.c_void_p),
        ("lo", C.c_void_p),
        ("hi", C.c_void_p),
        ("seed_base", C.c_int64),
    ]


class TwPrefixRows(C.Structure):
    """tw_prefix_rows: the rows an apply leaves unstored, by class."""
    _fields_ = [
        ("rows_hdr", C.c_uint64),
        ("rows_run", C.c_uint64),
        ("rows_reset", C.c_uint64),
        ("bytes_hdr", C.c_uint64),
        ("bytes_run", C.c_uint64),
        ("bytes_reset", C.c_uint64),
        ("bytes_stored", C.c_uint64),
        ("class_rows", C.c_uint64 * 5),
        ("class_bytes", C.c_uint64 * 5),
        ("apply_form", C.c_uint64),
        ("host_pairs", C.c_uint64),
        ("list_pairs", C.c_uint64),
        ("audit_rows", C.c_uint64 * 5),
    ]


class TwMeasureSpec(C.Structure):
    """tw_measure_spec: the two TRACE tags to join and the histogram's shape."""
    _fields_ = [
        ("tag_from", C.c_uint32),
        ("tag_to", C.c_uint32),
        ("n_bins", C.c_uint32),
        ("reserved", C.c_uint32),
        ("lo_us", C.c_int64),
        ("bin_us", C.c_int64),
    ]


class TwMeasureOut(C.Structure):
    """tw_measure_out: class counts and min / max / sum of one latency."""
    _fields_ = [
        ("pairs", C.c_uint64),
        ("open_from", C.c_uint64),
        ("open_to", C.c_uint64),
        ("repeated", C.c_uint64),
        ("truncated", C.c_uint64),
        ("underflow", C.c_uint64),
        ("overflow", C.c_uint64),
        ("min_us", C.c_int64),
        ("max_us", C.c_int64),
        ("sum_us", C.c_int64),
    ]


class TwSeriesSpec(C.Structure):
    """tw_series_spec: what tw_measure_series bins, and the bins."""
    _fields_ = [
        ("tag", C.c_uint32),
        ("tag_to", C.c_uint32),
        ("mode", C.c_uint32),
        ("n_bins", C.c_uint32),
        ("t0_us", C.c_int64),
        ("bin_us", C.c_int64),
        ("reserved", C.c_uint64),
    ]


class TwSeriesOut(C.Structure):
    """tw_series_out: the items of a series, counted."""
    _fields_ = [
        ("counted", C.c_uint64),
        ("underflow", C.c_uint64),
        ("overflow", C.c_uint64),
        ("truncated", C.c_uint64),
        ("t_min", C.c_int64),
        ("t_max", C.c_int64),
    ]


class TwSeriesStat(C.Structure):
    """tw_series_stat: the latencies of one bin's pairs (TW_SERIES_LATENCY)."""
    _fields_ = [
        ("sum_us", C.c_int64),
        ("min_us", C.c_int64),
        ("max_us", C.c_int64),
    ]


SERIES_EVENTS, SERIES_FIRST, SERIES_LATENCY = 0, 1, 2   # TW_SERIES_*
SERIES_MODES = {"events": SERIES_EVENTS, "first": SERIES_FIRST, "latency": SERIES_LATENCY}
SERIES_MAX_BINS = 8192       # TW_SERIES_MAX_BINS (events, first)
SERIES_MAX_LAT_BINS = 1024   # TW_SERIES_MAX_LAT_BINS (latency)

MEASURE_MAX_KEYS = 2048   # TW_MEASURE_MAX_KEYS
MEASURE_MAX_KEYS_LARGE = 4194304   # TW_MEASURE_MAX_KEYS_LARGE (tw_set_measure_keys)
MEASURE_MAX_BINS = 4096   # TW_MEASURE_MAX_BINS

RESULT_FIELDS = ["final_t", "events", "delivered", "dropped", "undeliverable", "status", "main_exc", "threads"]

# numpy dtype with the same layout as tw_replica_result (for bulk reads)
import numpy as _np  # noqa: E402

RESULT_DTYPE = _np.dtype([
    ("final_t", _np.int64), ("events", _np.uint64), ("delivered", _np.uint64),
    ("dropped", _np.uint64), ("undeliverable", _np.uint64), ("status", _np.uint32),
    ("main_exc", _np.uint32), ("threads", _np.uint64), ("tie_flags", _np.uint32), ("reserved", _np.uint32),
])
assert RESULT_DTYPE.itemsize == C.sizeof(TwReplicaResult)

# numpy dtype with the same layout as tw_measure_out (tw_measure's per-replica array)
MEASURE_DTYPE = _np.dtype([(f, _np.int64 if t is C.c_int64 else _np.uint64) for f, t in TwMeasureOut._fields_])
assert MEASURE_DTYPE.itemsize == C.sizeof(TwMeasureOut)
# tw_quantile (tw_measure_quantiles' entries)
QUANTILE_DTYPE = _np.dtype([("lo_us", _np.int64), ("hi_us", _np.int64)])
MEASURE_MAX_QUANTILES = 16   # TW_MEASURE_MAX_QUANTILES
# tw_series_out / tw_series_stat (tw_measure_series' arrays)
SERIES_DTYPE = _np.dtype([(f, _np.int64 if t is C.c_int64 else _np.uint64) for f, t in TwSeriesOut._fields_])
SERIES_STAT_DTYPE = _np.dtype([(f, _np.int64) for f, _ in TwSeriesStat._fields_])
assert SERIES_DTYPE.itemsize == C.sizeof(TwSeriesOut) and SERIES_STAT_DTYPE.itemsize == C.sizeof(TwSeriesStat)
assert isa.ABI_VERSION == 4
