"""The bookkeeping of tw_run's launch loop: tw_stats.launches, tw_stats.kernel_ms
and the order of tw_last_launch_ms.

Every launch of the event kernel is timed between two HIP events; so are the
sweep kernels behind a launch while a sweep stop is ahead, and the prefix
apply.  The times are listed in stream order: the pilot's launches, the prefix
apply, then per round of four launches each event kernel's time, followed by
its sweep's time in a segment that still has a stop ahead.  `launches` counts
the event kernel's only, `kernel_ms` is the sum of the list.  bench.py sums the
list; nothing else in the suite looks at it.

The token ring of test_gpu_prefix.py (4 nodes, one message in four dropped,
killed at 20 s: one sweep stop) under its (geometry, replicas) pairs; every
run is also compared with the oracle.

The device time of the sweeps alone is exported by the diagnostic build only
(tw_sweep_ms, -DTW_STATS): the sum of the sweep entries is compared with it
where the loaded library has the symbol.
"""
import ctypes as C
import math

import pytest

from timewarp import scenarios
from test_gpu_prefix import GEOS, _engine, _oracle, _ring, _same

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

PER_CHECK = 4  # launches of a replica run between two host checks


def _run(e, tag, ores, oh):
    """one reset / run pair: its stats and launch times, checked against the oracle"""
    e.reset()
    st = e.run()
    ms = e.launch_ms().tolist()
    _same(tag, e.results(), e.hashes(), ores, oh)
    print(tag, "launches", st.launches, "entries", len(ms), "kernel_ms", st.kernel_ms, "sum", math.fsum(ms))
    # the same float times added in double: only the order of the rounding differs
    assert math.isclose(st.kernel_ms, math.fsum(ms), rel_tol=1e-9), (tag, st.kernel_ms, math.fsum(ms))
    return st, ms


def _sweep_ms(e):
    """device time of the last run's sweeps, or None (the product build does not export it)"""
    try:
        fn = e.lib.tw_sweep_ms
    except AttributeError:
        return None
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    v = C.c_double(0.0)
    assert fn(e.ctx, C.byref(v)) == 0
    return v.value


def _swept(tag, e, st, ms):
    """`ms`: a run with a sweep stop ahead, behind any prefix entry"""
    n = len(ms) - st.launches
    assert n >= PER_CHECK and n % PER_CHECK == 0, (tag, len(ms), st.launches)
    assert e.sweep_stats()["killers"] > 0, tag
    want = _sweep_ms(e)
    if want is not None:
        assert math.isclose(math.fsum(ms[1:2 * n:2]), want, rel_tol=1e-9), (tag, want)
    return n


@pytest.mark.parametrize("geo,R", GEOS)
def test_plain_run(engine_mod, oracle_mod, geo, R):
    scn = _ring(4, R)
    ores, oh = _oracle(oracle_mod, scn)
    with _engine(engine_mod, scn, "fifo", geo, prefix=False, sweep=False) as e:
        st, ms = _run(e, (geo, "plain"), ores, oh)
        assert len(ms) == st.launches and st.launches % PER_CHECK == 0 and st.launches > 0


@pytest.mark.parametrize("geo,R", GEOS)
def test_sweep_entries_follow_their_launch(engine_mod, oracle_mod, geo, R):
    scn = _ring(4, R)
    ores, oh = _oracle(oracle_mod, scn)
    with _engine(engine_mod, scn, "fifo", geo, prefix=False, sweep=False) as e:
        st0, _ = _run(e, (geo, "sweep off"), ores, oh)
        e.set_sweep(True)
        st, ms = _run(e, (geo, "sweep on"), ores, oh)
        _swept((geo, "sweep on"), e, st, ms)
        # (the ring's replicas all end in the sweep: the segment's round is the run's only one)
        assert st.launches == st0.launches == PER_CHECK, (st.launches, st0.launches)


@pytest.mark.parametrize("geo,R", GEOS)
def test_prefix_entry_leads(engine_mod, oracle_mod, geo, R):
    scn = _ring(4, R)
    ores, oh = _oracle(oracle_mod, scn)
    with _engine(engine_mod, scn, "fifo", geo) as e:
        st, ms = _run(e, (geo, "piloted"), ores, oh)
        px = e.prefix_stats()
        assert px["last"] == "piloted" and px["apply_ms"] in ms
        # the pilot's launches are counted and listed; the apply's entry and the sweeps' are not
        assert st.launches >= 2 * PER_CHECK and st.launches % PER_CHECK == 0
        n = len(ms) - 1 - st.launches
        assert n >= PER_CHECK and n % PER_CHECK == 0, (len(ms), st.launches)
        st, ms = _run(e, (geo, "applied"), ores, oh)
        px = e.prefix_stats()
        assert px["last"] == "applied" and ms[0] == px["apply_ms"]
        _swept((geo, "applied"), e, st, ms[1:])


def test_lpb_one_entry(engine_mod, oracle_mod):
    """the batched window loop is timed as one launch"""
    scn = scenarios.hotspot(n_senders=8, n_replicas=64, msg_num=30)
    ores, oh = _oracle(oracle_mod, scn)
    with engine_mod.Engine(0) as e:
        e.load(scn, geometry="lpb")
        st, ms = _run(e, ("lpb",), ores, oh)
        assert st.launches == 1 and len(ms) == 1 and ms[0] == st.kernel_ms
