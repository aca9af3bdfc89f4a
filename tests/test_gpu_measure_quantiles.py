"""tw_measure_quantiles on the GPU: exact order statistics of one latency over
tw_measure's pairs -- per replica (sorted in LDS, or radix-selected) and over
the whole batch (digit counts per shard, the digits picked on the host).  Every
expectation is timewarp.measures.quantile_reference fed with the oracle's trace
log, never with the engine's own records; everything is integer and compared
for equality."""
import ctypes as C

import numpy as np
import pytest

import progs
from timewarp import scenarios
from timewarp.abi import MEASURE_MAX_KEYS, QUANTILE_DTYPE, RESULT_FIELDS
from timewarp.measures import quantile_reference
from timewarp.program import Program
from timewarp.scenarios import TAG_PING, TAG_PING_SENT, TAG_PONG

pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
ERR_INVALID, ERR_STATE = -1, -5
S, M, R = 6, 12, 70          # hotspot: senders, messages per sender, replicas (not a multiple of 64)
CAP = 1 << 11
QS = (0, 1, 250000, 499999, 500000, 500001, 990000, 999000, 999999, 1000000)
TAG_A, TAG_B = 40, 41


def _oracle_traces(oracle_mod, scn, rows=None):
    """Per-replica oracle trace logs (replicas with equal `rows` entries run
    the same thing: one oracle run serves them)."""
    seen, out = {}, []
    for r in range(scn.n_replicas):
        key = r if rows is None else rows[r]
        if key not in seen:
            seen[key] = oracle_mod.run(scn, replica=r, trace_cap=1 << 14).traces
            assert len(seen[key]) < (1 << 14)
        out.append(seen[key])
    return out


def _reference(traces, cap, tag_from, tag_to, qs=QS):
    return quantile_reference(traces, [len(t) for t in traces], cap, tag_from, tag_to, qs)


def _same(got, want, tag=""):
    (tot, per, pairs, trunc), (rtot, rper, rpairs, rtrunc) = got, want
    print(tag, "gpu", tot.tolist(), pairs, trunc, "ref", rtot, rpairs, rtrunc)
    assert (pairs, trunc) == (rpairs, rtrunc), tag
    assert tot.dtype == QUANTILE_DTYPE and tot.tolist() == [tuple(x) for x in rtot], tag
    if per is not None:
        assert per.dtype == QUANTILE_DTYPE and per.shape == rper.shape[:2]
        for i, f in enumerate(("lo_us", "hi_us")):
            assert np.array_equal(per[f], rper[:, :, i]), (tag, f, np.argwhere(per[f] != rper[:, :, i])[:8])


def _check(e, traces, cap, tag_from, tag_to, tag="", qs=QS):
    want = _reference(traces, cap, tag_from, tag_to, qs)
    got = e.measure_quantiles(tag_from, tag_to, qs, per_replica=True)
    _same(got, want, tag)
    only_total = e.measure_quantiles(tag_from, tag_to, qs)            # without the per-replica select
    assert only_total[1] is None
    _same(only_total, want, tag + " (total only)")
    return got, want


@pytest.fixture(scope="module")
def hotspot_ref(oracle_mod):
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=M)
    return scn, _oracle_traces(oracle_mod, scn)


def test_hotspot_every_geometry(engine_mod, hotspot_ref):
    scn, traces = hotspot_ref
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        res0, h0 = e.results(), e.hashes()
        m0 = e.measure(TAG_PING_SENT, TAG_PONG, lo_us=2000, bin_us=250, n_bins=40, per_replica=True)
        for tag_to, name in ((TAG_PONG, "round trip"), (TAG_PING, "one way")):
            (tot, per, pairs, trunc), _ = _check(e, traces, CAP, TAG_PING_SENT, tag_to, f"{e.geometry()} {name}")
            assert pairs == R * S * M and trunc == 0
            # q_ppm = 0 and 10^6 are tw_measure's min_us / max_us, pairs and truncated its counts
            mt, _, mper = e.measure(TAG_PING_SENT, tag_to, per_replica=True)
            assert (pairs, trunc) == (mt["pairs"], mt["truncated"])
            assert tot[0].tolist() == (mt["min_us"], mt["min_us"]) and tot[-1].tolist() == (mt["max_us"], mt["max_us"])
            assert np.array_equal(per["lo_us"][:, 0], mper["min_us"]) and np.array_equal(per["hi_us"][:, 0], mper["min_us"])
            assert np.array_equal(per["lo_us"][:, -1], mper["max_us"]) and np.array_equal(per["hi_us"][:, -1], mper["max_us"])
        ph = e.measure_quantiles_ms()
        print("phases", ph)
        assert ph["join_emit"] > 0 and 1 <= ph["total_passes"] <= 8
        # the call changes nothing: results, hashes and a following tw_measure
        res1, h1 = e.results(), e.hashes()
        for f in RESULT_FIELDS:
            assert np.array_equal(res0[f], res1[f]), f
        assert np.array_equal(h0, h1)
        m1 = e.measure(TAG_PING_SENT, TAG_PONG, lo_us=2000, bin_us=250, n_bins=40, per_replica=True)
        assert m0[0] == m1[0] and np.array_equal(m0[1], m1[1]) and m0[2].tobytes() == m1[2].tobytes()


@pytest.mark.one_geometry
def test_swapped_spec_is_negative(engine_mod, hotspot_ref):
    scn, traces = hotspot_ref
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        (tot, per, pairs, _), _ = _check(e, traces, CAP, TAG_PONG, TAG_PING_SENT, "swapped")
        assert pairs == R * S * M and (tot["hi_us"] < 0).all() and (per["hi_us"] < 0).all()


@pytest.mark.one_geometry
def test_drops_leave_uneven_replicas(engine_mod, oracle_mod):
    # a dropped link loses all of a sender's messages, so a replica's pairs are
    # a multiple of the message count: 11 of them give both parities
    odd_m = 11
    scn = scenarios.hotspot(n_senders=S, n_replicas=R, msg_num=odd_m, drop_log2=2)
    traces = _oracle_traces(oracle_mod, scn)
    want = _reference(traces, CAP, TAG_PING_SENT, TAG_PONG, (500000,))
    # pair counts per replica from the reference (a Pong received closes a pair)
    counts = [len([1 for t in tr if t[2] == TAG_PONG]) for tr in traces]
    assert want[2] == sum(counts) and 0 < want[2] < R * S * odd_m
    assert any(c and c % 2 == 0 for c in counts) and any(c % 2 == 1 for c in counts) and len(set(counts)) > 2
    assert sum(1 for tr in traces for t in tr if t[2] == TAG_PING_SENT) == R * S * odd_m   # the rest are open ids
    print("pairs per replica", sorted(set(counts)))   # (this seed has a replica of 0 pairs; 1 pair: test_scripted_latencies)
    assert 0 in counts
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(CAP).reset()
        e.run()
        _check(e, traces, CAP, TAG_PING_SENT, TAG_PONG, "drops")


# ------------------------------------------------------- scripted latencies
def scripted(rows, n_replicas):
    """One main thread per replica with registers (n, w, mode, 0) =
    rows[r % len].  Every replica: id 7 twice under TAG_A and once under TAG_B
    (repeated), id 8 under TAG_A only, id 9 under TAG_B only -- none of them a
    pair.  mode 0: nothing else.  mode 1: n times TAG_A, wait w, TAG_B of the
    same id: n latencies equal to w.  mode 2: TAG_A of ids 100000 + i, each
    followed by a wait of w + i; TAG_B of ids 200000 + i, likewise; then, all
    at the final time T, TAG_B of 100000 + i (latency T - t_i > 0), TAG_A of
    200000 + i (latency t_i - T < 0) and both tags of 300000 + i (latency 0):
    3 n pairs."""
    p = Program()
    c = p.function("main")
    c.nstore(0, 0).nstore(1, 1).nstore(2, 2)
    c.seti(0, 7).trace(TAG_A, 0).trace(TAG_A, 0).trace(TAG_B, 0)
    c.seti(0, 8).trace(TAG_A, 0)
    c.seti(0, 9).trace(TAG_B, 0)

    def loop(body):   # r3 = i over 0 .. n - 1
        c.seti(3, 0)
        top, done = c.here(), c.label()
        c.nload(1, 0).jle(1, 3, done)
        body()
        c.addi(3, 1).jmp(top)
        c.bind(done)

    def ident(base):
        return c.mov(0, 3).addi(0, base)

    mode2, fin = c.label(), c.label()
    c.nload(1, 2).jnei(1, 1, mode2)
    loop(lambda: (ident(1000).trace(TAG_A, 0), c.nload(1, 1).wait_reg(1), ident(1000).trace(TAG_B, 0)))
    c.jmp(fin)
    c.bind(mode2)
    c.nload(1, 2).jnei(1, 2, fin)
    loop(lambda: (ident(100000).trace(TAG_A, 0), c.nload(1, 1).add(1, 3).wait_reg(1)))
    loop(lambda: (ident(200000).trace(TAG_B, 0), c.nload(1, 1).add(1, 3).wait_reg(1)))
    loop(lambda: (ident(100000).trace(TAG_B, 0), ident(200000).trace(TAG_A, 0),
                  ident(300000).trace(TAG_A, 0).trace(TAG_B, 0)))
    c.bind(fin)
    c.end()
    scn = progs.single(p, "scripted_latencies", n_replicas=n_replicas)
    keys = [tuple(rows[r % len(rows)]) for r in range(n_replicas)]
    scn.main_regs = np.array([list(k) + [0] for k in keys], dtype=np.int64)
    return scn, keys


# (n, w, mode).  The waits of rows 3 and 5 are above 2^32 us: the latencies of
# the batch span -2^36 .. 2^41, so the batch-wide select fixes all eight digits
ROWS = [(0, 0, 0),                  # no pairs
        (1, 5, 1),                  # one pair
        (9, 1234, 1),               # nine equal latencies
        (6, 1 << 33, 2),            # negative, zero and positive, 18 pairs: above 2^32 either side
        (40, 3, 2),                 # the same, small: 120 pairs
        (4, (1 << 40) + 7, 1)]      # four equal, large
SCRIPTED_R = 67
SCRIPTED_CAP = 1 << 10


@pytest.fixture(scope="module")
def scripted_ref(oracle_mod):
    scn, keys = scripted(ROWS, SCRIPTED_R)
    traces = _oracle_traces(oracle_mod, scn, rows=keys)
    assert [len(t) for t in traces[:6]] == [5, 7, 23, 5 + 6 * 6, 5 + 6 * 40, 13]
    return scn, traces


def _check_scripted(e, traces, tag):
    (tot, per, pairs, trunc), want = _check(e, traces, SCRIPTED_CAP, TAG_A, TAG_B, tag)
    med = QS.index(500000)
    # what the rows say, by hand: replica 0 is empty, 1 holds the one latency 5,
    # 2 nine times 1234, 5 four times 2^40 + 7; 3 and 4 hold n negative, n zero
    # and n positive latencies: the median is 0
    assert per[0].tolist() == [(I64_MAX, I64_MIN)] * len(QS)
    assert per[1].tolist() == [(5, 5)] * len(QS) and per[2].tolist() == [(1234, 1234)] * len(QS)
    assert per[5].tolist() == [((1 << 40) + 7,) * 2] * len(QS)
    for r in (3, 4):
        assert per[r][0]["lo_us"] < 0 < per[r][-1]["hi_us"] and per[r][med].tolist() == (0, 0)
    assert per[3][0]["lo_us"] < -(1 << 35) and per[3][-1]["hi_us"] > 1 << 35
    reps = [sum(1 for r in range(SCRIPTED_R) if r % 6 == k) for k in range(6)]
    assert pairs == reps[1] + 9 * reps[2] + 18 * reps[3] + 120 * reps[4] + 4 * reps[5] and trunc == 0
    assert tot[0]["lo_us"] < -(1 << 35) and tot[-1]["hi_us"] == (1 << 40) + 7
    _check(e, traces, SCRIPTED_CAP, TAG_B, TAG_A, tag + " swapped")
    return tot, per


@pytest.mark.one_geometry
def test_scripted_latencies(engine_mod, scripted_ref):
    scn, traces = scripted_ref
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(SCRIPTED_CAP).reset()
        e.run()
        _check_scripted(e, traces, "scripted")
        assert e.measure_quantiles_ms()["total_passes"] == 8       # min < 0 < max: no shared digit
        # one quantile, sixteen of them, and the same one sixteen times
        _check(e, traces, SCRIPTED_CAP, TAG_A, TAG_B, "one", qs=(500000,))
        _check(e, traces, SCRIPTED_CAP, TAG_A, TAG_B, "sixteen", qs=tuple(31250 + i * 62500 for i in range(16)))
        _check(e, traces, SCRIPTED_CAP, TAG_A, TAG_B, "repeated", qs=(999000,) * 16)
        # tags nobody traced: no pairs anywhere
        tot, per, pairs, trunc = e.measure_quantiles(50, 51, QS, per_replica=True)
        assert pairs == trunc == 0 and tot.tolist() == [(I64_MAX, I64_MIN)] * len(QS)
        assert (per["lo_us"] == I64_MAX).all() and (per["hi_us"] == I64_MIN).all()


@pytest.mark.one_geometry
def test_trace_cap_truncates_replicas(engine_mod, scripted_ref):
    scn, traces = scripted_ref
    cap = 40                                  # rows 3 (41 records) and 4 (245) emit more
    want = _reference(traces, cap, TAG_A, TAG_B)
    reps = [sum(1 for r in range(SCRIPTED_R) if r % 6 == k) for k in range(6)]
    assert want[3] == reps[3] + reps[4] and want[2] == reps[1] + 9 * reps[2] + 4 * reps[5]
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(cap).reset()
        e.run()
        (tot, per, pairs, trunc), _ = _check(e, traces, cap, TAG_A, TAG_B, "truncated")
        assert trunc == reps[3] + reps[4]
        for r in (3, 4, 9, 10):               # truncated: the empty entry
            assert per[r].tolist() == [(I64_MAX, I64_MIN)] * len(QS)
        assert tot[0].tolist() == (5, 5) and tot[-1].tolist() == ((1 << 40) + 7,) * 2   # the negative ones are gone


@pytest.mark.one_geometry
@pytest.mark.parametrize("measure_hook,lds_hook", [("0:1024", None), (None, "8"), ("0:1024", "8"), ("0:4", "0")])
def test_hooks_reach_the_other_paths(engine_mod, hotspot_ref, scripted_ref, monkeypatch, measure_hook, lds_hook):
    """TW_TEST_MEASURE sends every replica with a key through the partition path
    (tw_measure_join_large's emit), TW_TEST_QUANTILE_LDS=8 every replica of more
    than 8 pairs through the radix select; both are read when the context is
    made.  The results are the same function of the records."""
    if measure_hook:
        monkeypatch.setenv("TW_TEST_MEASURE", measure_hook)
    if lds_hook:
        monkeypatch.setenv("TW_TEST_QUANTILE_LDS", lds_hook)
    scn, traces = scripted_ref
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(SCRIPTED_CAP).reset()
        e.run()
        _check_scripted(e, traces, f"hooks {measure_hook} {lds_hook}")
        if measure_hook:
            e.measure(TAG_A, TAG_B)
            assert e.measure_phases_ms()["join_large"] > 0
        scn, traces = hotspot_ref
        e.load(scn).set_trace(CAP).reset()
        e.run()
        _check(e, traces, CAP, TAG_PING_SENT, TAG_PONG, "hotspot under the hooks")
        _check(e, traces, CAP, TAG_PONG, TAG_PING_SENT, "hotspot swapped under the hooks")


def _boundary(pad):
    """Replica 0: (MEASURE_MAX_KEYS - 6) / 2 pairs of latency i + 1 .. plus the
    scripted noise: 2,048 matching records, + `pad` TAG_A-only ones."""
    n = (MEASURE_MAX_KEYS - 6) // 2
    p = Program()
    c = p.function("main")
    c.nstore(0, 0)
    c.seti(0, 7).trace(TAG_A, 0).trace(TAG_A, 0).trace(TAG_B, 0)
    c.seti(0, 8).trace(TAG_A, 0)
    c.seti(0, 9).trace(TAG_B, 0)
    c.seti(0, 10).trace(TAG_B, 0)
    for k in range(pad):
        c.seti(0, 11 + k).trace(TAG_A, 0)
    c.seti(3, 0).seti(2, 1)
    top, done = c.here(), c.label()
    c.nload(1, 0).jle(1, 3, done)
    c.mov(0, 3).addi(0, 1000).trace(TAG_A, 0)
    c.wait_reg(2)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    top2, fin = c.here(), c.label()
    c.jeqi(3, 0, fin)
    c.addi(3, -1)
    c.mov(0, 3).addi(0, 1000).trace(TAG_B, 0)
    c.jmp(top2)
    c.bind(fin)
    c.end()
    scn = progs.single(p, "boundary", n_replicas=3)
    rows = [(n, 0, 0, 0), (5, 0, 0, 0), (0, 0, 0, 0)]
    scn.main_regs = np.array(rows, dtype=np.int64)
    return scn, rows, n


@pytest.mark.one_geometry
def test_key_boundary(engine_mod, oracle_mod):
    q = np.array(QS, np.uint32)
    for pad in (0, 1):
        scn, rows, n = _boundary(pad)
        traces = _oracle_traces(oracle_mod, scn, rows=rows)
        assert len(traces[0]) == MEASURE_MAX_KEYS + pad
        with engine_mod.Engine() as e:
            e.load(scn).set_trace(2 * CAP).reset()
            e.run()
            if pad:
                # over the LDS join's limit: refused, nothing written ...
                tot = np.frombuffer(bytearray(b"\xa5" * (16 * len(QS))), QUANTILE_DTYPE)
                per = np.frombuffer(bytearray(b"\xa5" * (16 * len(QS) * 3)), QUANTILE_DTYPE)
                pairs, trunc = C.c_uint64(77), C.c_uint64(78)
                rc = e.lib.tw_measure_quantiles(e.ctx, TAG_A, TAG_B, q.ctypes.data, q.size, tot.ctypes.data,
                                                per.ctypes.data, 3, C.byref(pairs), C.byref(trunc))
                assert rc == ERR_INVALID and (pairs.value, trunc.value) == (77, 78)
                assert tot.tobytes() == b"\xa5" * (16 * len(QS)) and per.tobytes() == b"\xa5" * (16 * len(QS) * 3)
                e.set_measure_keys(4096)      # ... until the limit is raised: the partition path
            (tot, per, pairs, _), _ = _check(e, traces, 2 * CAP, TAG_A, TAG_B, f"boundary + {pad}")
            assert pairs == n + 5 and tot[0].tolist() == (1, 1) and tot[-1].tolist() == (n, n)
            assert per[0][QS.index(500000)].tolist() == ((n + 1) // 2, (n + 1) // 2 + (n % 2 == 0))
            if pad:
                e.measure(TAG_A, TAG_B)
                assert e.measure_phases_ms()["join_large"] > 0


@pytest.mark.one_geometry
def test_two_shards_of_one_gpu(engine_mod, hotspot_ref, scripted_ref):
    for (scn, traces), cap, tags in ((hotspot_ref, CAP, (TAG_PING_SENT, TAG_PONG)),
                                     (scripted_ref, SCRIPTED_CAP, (TAG_A, TAG_B))):
        with engine_mod.Engine() as e:
            e.load(scn).set_trace(cap).reset()
            e.run()
            one = e.measure_quantiles(*tags, QS, per_replica=True)
        with engine_mod.Engine(devices=[0, 0]) as e:
            e.load(scn).set_trace(cap).reset()
            e.run()
            (tot, per, pairs, trunc), want = _check(e, traces, cap, *tags, "two shards")
        assert tot.tobytes() == one[0].tobytes() and per.tobytes() == one[1].tobytes() and (pairs, trunc) == one[2:]
        # the second shard's first replica
        half = scn.n_replicas // 2 if scn.n_replicas == R else None
        if half is not None:
            assert half == 35 and np.array_equal(per["lo_us"][35], want[1][35, :, 0])


@pytest.mark.one_geometry
@pytest.mark.parametrize("trace_batch", [False, True])
def test_traced_lpb_context(engine_mod, oracle_mod, trace_batch):
    scn = scenarios.hotspot(n_senders=16, n_replicas=64, msg_num=10, drop_log2=2)
    traces = _oracle_traces(oracle_mod, scn)
    with engine_mod.Engine() as e:
        e.load(scn, geometry="lpb").set_trace(CAP).set_trace_batch(trace_batch).reset()
        assert e.geometry() == "lpb"
        e.run()
        (_, _, pairs, trunc), _ = _check(e, traces, CAP, TAG_PING_SENT, TAG_PONG, f"lpb batch={trace_batch}")
        assert 0 < pairs < 64 * 16 * 10 and trunc == 0
        _check(e, traces, CAP, TAG_PONG, TAG_PING, "lpb another spec")


def _raw(e, tag_from, tag_to, qs, n, n_q=None, null_q=False):
    """tw_measure_quantiles straight through ctypes into prefilled buffers;
    returns the status and whether every output is untouched."""
    q = np.array(qs, np.uint32)
    n_q = len(qs) if n_q is None else n_q
    tot = np.frombuffer(bytearray(b"\xa5" * (16 * 17)), QUANTILE_DTYPE)
    per = np.frombuffer(bytearray(b"\xa5" * (16 * 17 * max(n, 1))), QUANTILE_DTYPE)
    pairs, trunc = C.c_uint64(77), C.c_uint64(78)
    rc = e.lib.tw_measure_quantiles(e.ctx, tag_from, tag_to, None if null_q else q.ctypes.data, n_q, tot.ctypes.data,
                                    per.ctypes.data, n, C.byref(pairs), C.byref(trunc))
    clean = (tot.tobytes() == b"\xa5" * tot.nbytes and per.tobytes() == b"\xa5" * per.nbytes
             and (pairs.value, trunc.value) == (77, 78))
    return rc, clean


@pytest.mark.one_geometry
def test_refusals_write_nothing(engine_mod):
    scn = scenarios.hotspot(n_senders=2, n_replicas=4, msg_num=3)
    with engine_mod.Engine() as e:
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 4) == (ERR_STATE, True)        # nothing loaded
        e.load(scn)
        e.run()
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 4) == (ERR_STATE, True)        # tracing is off
        e.set_trace(64).reset()
        e.run()
        assert _raw(e, TAG_PONG, TAG_PONG, (500000,), 4) == (ERR_INVALID, True)           # equal tags
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 4, n_q=0) == (ERR_INVALID, True)
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (1,) * 17, 4) == (ERR_INVALID, True)      # above the maximum
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (0, 1000001), 4) == (ERR_INVALID, True)   # a q_ppm above 10^6
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 4, null_q=True) == (ERR_INVALID, True)
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 3) == (ERR_INVALID, True)      # n is not the replica count
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 5) == (ERR_INVALID, True)
        rc, clean = _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 4)
        assert rc == 0 and not clean
        with pytest.raises(engine_mod.EngineError) as ei:
            e.measure_quantiles(TAG_PING_SENT, TAG_PONG, (1000001,))
        assert ei.value.code == ERR_INVALID
        tot, per, pairs, trunc = e.measure_quantiles(TAG_PING_SENT, TAG_PONG)             # the context stays usable
        assert pairs == 4 * 2 * 3 and per is None and tot.shape == (1,)
        e.set_trace(0)
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 4) == (ERR_STATE, True)        # tracing off again
    lpb = scenarios.hotspot(n_senders=16, n_replicas=64, msg_num=30)
    with engine_mod.Engine() as e:
        e.load(lpb, geometry="lpb")
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 64) == (ERR_INVALID, True)     # lpb, tracing off
    gos = scenarios.gossip(256, seed=1)
    with engine_mod.LPEngine(engine_mod.lp_scenario(gos), 0, gos.n_nodes, int(gos.meta["lookahead_us"])) as e:
        assert _raw(e, TAG_PING_SENT, TAG_PONG, (500000,), 0) == (ERR_INVALID, True)      # a tw_lp_load context


@pytest.mark.one_geometry
def test_overfilled_bucket_table_is_a_status(engine_mod, oracle_mod, monkeypatch):
    """TW_TEST_MEASURE=2048:1048576 makes a replica of 2,500 distinct ids per
    tag one bucket, more than its table's 2,048 slots: TW_ERR_INVALID, nothing
    written, and the context stays usable."""
    p = Program()
    c = p.function("main")
    c.seti(3, 0).seti(2, 2500).seti(1, 1)
    top, done = c.here(), c.label()
    c.jle(2, 3, done)
    c.mov(0, 3).trace(TAG_A, 0).wait_reg(1).trace(TAG_B, 0)
    c.addi(3, 1).jmp(top)
    c.bind(done)
    c.end()
    scn = progs.single(p, "one_bucket", n_replicas=2)
    monkeypatch.setenv("TW_TEST_MEASURE", "2048:1048576")
    with engine_mod.Engine() as e:
        e.load(scn).set_trace(8192).set_measure_keys(8192).reset()
        e.run()
        assert _raw(e, TAG_A, TAG_B, (500000,), 2) == (ERR_INVALID, True)
        assert _raw(e, 50, 51, (500000,), 2)[0] == 0           # tags nobody traced: the context is usable
