"""The further rows a prefix apply leaves unstored against the
oracle and against the same context with the prefix off: every result field and
every node hash bit-exact in every step, with TW_TEST_PREFIX_AUDIT=1
everywhere -- the hook's read-only pass compares every element of every row the
apply skipped, of every class, with the snapshot's.

Beside quads 1 - 3 of the claimed slots (3o, tw_prefix_clean_stats) an apply
skips, by class (tw_prefix_rows_stats): the header quad of a claimed slot when
the verifying sweep ended every replica it carried out (CF_HDR_OK); the run
entry of a kill wake the sweep compared with the table's; and the rows of
nvars, hash, bind, bind_own, bind_rel and tmo_done whose snapshot value is what
tw_reset leaves -- those whether or not the last run verified, since a cached
apply is the first device work behind a reset.  The pilot's apply stores
everything.  TW_TEST_PREFIX_ROWS=0 (read when the context is made) turns the
three classes off and leaves tw_prefix_clean_stats as it is with them on.

70 and 301 replicas are no multiple of 16: the 8-, 4- and 1-byte rows of the
last class start and end off a 16-byte boundary.
"""
import dataclasses
import functools
import os

import numpy as np
import pytest

from timewarp import scenarios
from timewarp.abi import RESULT_FIELDS
from timewarp.timeunits import sec

from test_gpu_sweep_table import units

pytestmark = [pytest.mark.gpu, pytest.mark.one_geometry]

FIELDS = [f for f in RESULT_FIELDS if f != "tie_flags"]
ORACLE_MODE = {"fifo": 0, "forkfirst": 5}
T_KILL = sec(20)
GEOS = [("dense", 301), ("narrow", 70), ("half", 301)]
ORDERS = ["fifo", "forkfirst"]

_ORACLE = {}


@pytest.fixture(autouse=True)
def _audit_hook(monkeypatch):
    monkeypatch.setenv("TW_TEST_PREFIX_AUDIT", "1")  # (read when a context is made)


@functools.lru_cache(maxsize=None)
def _ring(n_nodes, n_replicas, link_depth=1):
    return scenarios.token_ring(n_nodes=n_nodes, n_replicas=n_replicas, launch_duration=T_KILL, drop_log2=2,
                                link_depth=link_depth)


def _oracle(oracle_mod, scn, order):
    key = (id(scn), order)  # (the builders are cached: one object per scenario)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.run_batch(scn, mode=ORACLE_MODE[order], threads=8)
    return _ORACLE[key]


def _same(tag, res, h, ores, oh):
    for f in FIELDS:
        assert np.array_equal(res[f], ores[f]), (tag, f, res[f][:6], ores[f][:6])
    assert np.array_equal(h, oh), tag


def _engine(engine_mod, scn, order, geo, prefix=True):
    e = engine_mod.Engine(0)
    e.load(scn, geometry=geo)
    e.set_tie_mode(order)
    if not prefix:
        e.set_prefix(False)
    return e


def _rows_off_engine(engine_mod, monkeypatch, scn, order, geo):
    """the same context with the classes of 3v off"""
    monkeypatch.setenv("TW_TEST_PREFIX_ROWS", "0")
    e = _engine(engine_mod, scn, order, geo)
    monkeypatch.delenv("TW_TEST_PREFIX_ROWS")
    return e


def _step(e, runs=({},)):
    """reset, the tw_run calls `runs`: results, hashes, tw_prefix_stats, tw_prefix_clean_stats and
    tw_prefix_rows_stats (the apply is the first call's: its counts are read behind that call)"""
    e.reset()
    cs = None
    for kw in runs:
        e.run(**kw)
        if cs is None:
            cs, ps, rs = e.prefix_clean_stats(), e.prefix_stats(), e.prefix_rows_stats()
    cs["verified"] = e.prefix_clean_stats()["verified"]  # (of the last call)
    print(ps["last"], cs, {k: v for k, v in rs.items() if not k.startswith("class_")}, rs["class_rows"])
    return e.results(), e.hashes(), ps, cs, rs


def _off(engine_mod, scn, order, geo, **kw):
    """the same context with the prefix off"""
    with _engine(engine_mod, scn, order, geo, prefix=False) as e0:
        e0.reset()
        e0.run(**kw)
        assert e0.prefix_stats()["last"] == "not_eligible"
        return e0.results(), e0.hashes()


def _adds_up(ps, cs, rs):
    """audit 0; stored plus skipped bytes over all classes are the snapshot's"""
    assert cs["audit_mismatches"] == 0, cs
    assert rs["bytes_hdr"] == 16 * rs["rows_hdr"] and rs["bytes_run"] == 16 * rs["rows_run"], rs
    assert cs["bytes_stored"] + 16 * cs["rows_skipped"] == ps["bytes"], (ps, cs)
    assert rs["bytes_stored"] + 16 * cs["rows_skipped"] + rs["bytes_hdr"] + rs["bytes_run"] + rs["bytes_reset"] \
        == ps["bytes"], (ps, cs, rs)
    assert sum(rs["class_bytes"].values()) == ps["bytes"], (ps, rs)
    assert rs["class_rows"]["body"] == 3 * cs["claimed_slots"], (cs, rs)
    assert rs["class_rows"]["hdr"] in (0, cs["claimed_slots"]), (cs, rs)  # (0: TW_TEST_PREFIX_ROWS=0)
    # the device's own count of the rows its flags let the apply skip (the hook's kernel), by class,
    # against the host's, which come from its copy of the flags and its classification
    assert rs["audit_rows"] == {"none": 0, "body": cs["rows_skipped"], "hdr": rs["rows_hdr"], "run": rs["rows_run"],
                                "reset": rs["rows_reset"]}, (cs, rs)


def _form(rs, cs, rows_on=True, spans=1):
    """How a cached apply ran: over the list unless TW_TEST_PREFIX_LIST=0 or TW_TEST_PREFIX_ROWS=0; the
    device listed as many pairs as the host launched workgroups; with one span per row (R * 16 <= 64 KiB)
    that is one pair per row it stored"""
    want = "list" if rows_on and os.environ.get("TW_TEST_PREFIX_LIST") != "0" else "grid"
    assert rs["apply_form"] == want, rs
    if want == "grid":
        assert rs["list_pairs"] == rs["host_pairs"] == 0, rs
        return
    stored = sum(rs["class_rows"].values()) - cs["rows_skipped"] - rs["rows_hdr"] - rs["rows_run"] - rs["rows_reset"]
    assert rs["list_pairs"] == rs["host_pairs"] > 0, rs
    assert rs["list_pairs"] == stored if spans == 1 else rs["list_pairs"] > stored, (stored, rs)


def _stores_all(ps, cs, rs, want="piloted"):
    """the pilot's apply: nothing of any class"""
    assert ps["last"] == want, ps
    _adds_up(ps, cs, rs)
    assert cs["rows_skipped"] == 0 and rs["rows_hdr"] == rs["rows_run"] == rs["rows_reset"] == 0, (cs, rs)
    assert rs["bytes_stored"] == cs["bytes_stored"] == ps["bytes"], (ps, cs, rs)
    assert rs["apply_form"] == "grid" and rs["list_pairs"] == 0, rs


def _reset_rows(rs):
    """class 4: exactly the rows the host's classification reports, and their bytes"""
    assert rs["rows_reset"] == rs["class_rows"]["reset"] > 0, rs
    assert rs["bytes_reset"] == rs["class_bytes"]["reset"] > 0, rs


def _skips(ps, cs, rs, hdr=True, some=True, spans=1):
    """A cached apply behind a verifying run.  One dirty byte per claimed slot
    decides for its quads 1 - 3, its header and, if it is a killer, its run
    entry: with CF_HDR_OK the header rows skipped are a third of 3o's rows,
    and the run entries at most as many.  some: more than none of each; not
    some: none of any (every claimed slot is dirty in some replica: the
    4-node ring), only the reset-valued rows."""
    assert ps["last"] == "applied", ps
    _adds_up(ps, cs, rs)
    _form(rs, cs, spans=spans)
    assert cs["rows_skipped"] <= 3 * cs["claimed_slots"], cs
    assert rs["rows_hdr"] <= cs["claimed_slots"], (cs, rs)
    assert rs["rows_hdr"] * 3 == (cs["rows_skipped"] if hdr else 0), (cs, rs)
    assert rs["rows_run"] <= rs["class_rows"]["run"], rs  # (one row per claimable position)
    assert 3 * rs["rows_run"] <= cs["rows_skipped"], (cs, rs)
    if some:
        assert cs["rows_skipped"] > 0 and rs["rows_run"] > 0 and (rs["rows_hdr"] > 0 or not hdr), (cs, rs)
    else:
        assert cs["rows_skipped"] == rs["rows_hdr"] == rs["rows_run"] == 0, (cs, rs)
    _reset_rows(rs)


def _reset_only(ps, cs, rs):
    """a cached apply behind a run that did not verify, or behind a state-writing call"""
    assert ps["last"] == "applied", ps
    _adds_up(ps, cs, rs)
    assert cs["rows_skipped"] == 0 and rs["rows_hdr"] == 0 and rs["rows_run"] == 0, (cs, rs)
    _form(rs, cs)
    _reset_rows(rs)


CS_KEYS = ("claimed_slots", "rows_skipped", "bytes_stored", "verified", "audit_mismatches")


def _rows_off(cs, cs0, rs0):
    """TW_TEST_PREFIX_ROWS=0: tw_prefix_clean_stats as with the classes on, none of their rows skipped or classed"""
    assert {k: cs[k] for k in CS_KEYS} == {k: cs0[k] for k in CS_KEYS}, (cs, cs0)
    assert rs0["rows_hdr"] == rs0["rows_run"] == rs0["rows_reset"] == 0, rs0
    assert rs0["class_rows"]["hdr"] == rs0["class_rows"]["run"] == rs0["class_rows"]["reset"] == 0, rs0
    assert rs0["bytes_stored"] == cs0["bytes_stored"], (cs0, rs0)
    _form(rs0, cs0, rows_on=False)


# --------------------------------------------------------- pilot, then skipping applies
def _main_case(engine_mod, oracle_mod, monkeypatch, scn, order, geo, steps=4, some=True, spans=1):
    ores, oh = _oracle(oracle_mod, scn, order)
    res0, h0 = _off(engine_mod, scn, order, geo)
    _same((order, geo, "off"), res0, h0, ores, oh)
    with _engine(engine_mod, scn, order, geo) as e, _rows_off_engine(engine_mod, monkeypatch, scn, order, geo) as er:
        for i in range(steps):
            res, h, ps, cs, rs = _step(e)
            resr, hr, psr, csr, rsr = _step(er)
            _same((order, geo, i), res, h, ores, oh)
            _same((order, geo, i, "off"), res, h, res0, h0)
            _same((order, geo, i, "rows off"), resr, hr, ores, oh)
            assert cs["verified"], cs
            _rows_off(cs, csr, rsr)
            _adds_up(psr, csr, rsr)
            if i == 0:
                _stores_all(ps, cs, rs)
            else:
                _skips(ps, cs, rs, some=some, spans=spans)


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("N", [40, 4])
def test_ring_skips_every_class(engine_mod, oracle_mod, monkeypatch, N, order, geo, R):
    """40 nodes: most are never visited, their threads' rows of every class are
    skipped.  4 nodes: the token passes every worker in some replica, which
    marks its position's three slots, so every claimed slot is dirty (3o's own
    rows_skipped is 0 there, tests/test_gpu_prefix_clean.py): no header row
    and no run entry may be skipped either, and the test asserts 0 of each,
    by the host's count and the device's; only the reset-valued rows are
    skipped (28 of them, 12 claimed slots)."""
    _main_case(engine_mod, oracle_mod, monkeypatch, _ring(N, R), order, geo, some=N != 4)


@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("form", ["0", "1"])
def test_both_forms_of_the_apply(engine_mod, oracle_mod, monkeypatch, form, geo, R):
    """TW_TEST_PREFIX_LIST: the early-exit grid (0) and the compact list (1) skip and store the same rows"""
    monkeypatch.setenv("TW_TEST_PREFIX_LIST", form)
    _main_case(engine_mod, oracle_mod, monkeypatch, _ring(40, R), "forkfirst", geo, steps=3)


@pytest.mark.parametrize("form", ["0", "1"])
def test_rows_of_several_spans(engine_mod, oracle_mod, monkeypatch, form):
    """4,500 replicas: a 16-byte row is 72,000 B, two 64-KiB spans, an 8-byte
    row one -- the list holds two pairs for the wide rows and one for the
    narrow ones, and the grid's second workgroup of a narrow row returns"""
    monkeypatch.setenv("TW_TEST_PREFIX_LIST", form)
    _main_case(engine_mod, oracle_mod, monkeypatch, _ring(40, 4500), "forkfirst", "dense", steps=3, spans=2)


def test_link_depth(engine_mod, oracle_mod, monkeypatch):
    _main_case(engine_mod, oracle_mod, monkeypatch, _ring(40, 70, link_depth=3), "fifo", "narrow", steps=3)


# ------------------------------------------------------------------ CF_HDR_OK false
@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
@pytest.mark.parametrize("order", ORDERS)
def test_surviving_replicas_keep_the_header_rows(engine_mod, oracle_mod, order, geo, R):
    """Where the ping arrives a thread sleeps past T: that replica's sweep takes
    the general path and stores dead headers; where it is dropped the replica
    ends on the terminal path; both kinds share every wave.  A run that stops at
    T verifies (no replica has work left before it), and the next apply skips
    the claimed slots' quads 1 - 3 and the run entries but no header row."""
    K = 40
    scn = units("survivor", K, R, 1)
    ores, oh = _oracle(oracle_mod, scn, order)
    with _engine(engine_mod, scn, order, geo) as e:
        res, h, ps, cs, rs = _step(e, ({"t_end": T_KILL},))
        _stores_all(ps, cs, rs)
        assert cs["verified"], cs
        term = e.sweep_path_stats()["terminal_replicas"]
        assert 0 < term < R, term
        for i in range(2):
            res, h, ps, cs, rs = _step(e, ({"t_end": T_KILL},))
            _skips(ps, cs, rs, hdr=False)
            assert cs["verified"], cs
        # on to the end from such an apply: the oracle's results at the later time
        res, h, ps, cs, rs = _step(e)
        _skips(ps, cs, rs, hdr=False)
        _same((order, geo, "to the end"), res, h, ores, oh)
        assert not cs["verified"]  # (the survivors had work left behind the sweep)
        res, h, ps, cs, rs = _step(e)
        _reset_only(ps, cs, rs)
        _same((order, geo, "again"), res, h, ores, oh)


@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
def test_all_terminal_units_skip_the_header_rows(engine_mod, oracle_mod, geo, R):
    """the same program without the survivor: every replica is terminal"""
    scn = units("plain", 40, R, 1)
    ores, oh = _oracle(oracle_mod, scn, "fifo")
    with _engine(engine_mod, scn, "fifo", geo) as e:
        _stores_all(*_step(e)[2:])
        for i in range(2):
            res, h, ps, cs, rs = _step(e)
            _skips(ps, cs, rs)
            _same((geo, i), res, h, ores, oh)
            # (the ping's handler touches no parked thread: every claimed slot is clean)
            assert rs["rows_hdr"] == cs["claimed_slots"] and rs["rows_run"] == rs["class_rows"]["run"], (cs, rs)


# ------------------------------------------------------------------ invalidation
@pytest.mark.parametrize("geo,R", GEOS)
@pytest.mark.parametrize("order", ORDERS)
def test_runs_that_do_not_verify(engine_mod, oracle_mod, order, geo, R):
    """the sweep off, a run in pieces that stops before T, the sweep refused at
    the event cap: the next apply skips the reset-valued rows alone"""
    scn = _ring(40, R)
    ores, oh = _oracle(oracle_mod, scn, order)
    cap = int(ores["events"].min()) - 1
    res0, h0 = _off(engine_mod, scn, order, geo, max_events=cap)
    with _engine(engine_mod, scn, order, geo) as e:
        _stores_all(*_step(e)[2:])
        _skips(*_step(e)[2:])
        e.set_sweep(False)
        res, h, ps, cs, rs = _step(e)
        _reset_only(ps, cs, rs)
        assert not cs["verified"]
        _same((order, geo, "sweep off"), res, h, ores, oh)
        e.set_sweep(True)
        res, h, ps, cs, rs = _step(e)
        _reset_only(ps, cs, rs)
        assert cs["verified"]
        _same((order, geo, "sweep on"), res, h, ores, oh)
        _skips(*_step(e)[2:])
        # in pieces, stopping before T; then reset
        res, h, ps, cs, rs = _step(e, ({"t_end": sec(5)}, {"t_end": T_KILL - 1}))
        _skips(ps, cs, rs)
        assert not cs["verified"]
        res, h, ps, cs, rs = _step(e)
        _reset_only(ps, cs, rs)
        _same((order, geo, "after pieces"), res, h, ores, oh)
        # in pieces across T: the piece that holds the sweep verifies
        res, h, ps, cs, rs = _step(e, ({"t_end": sec(5)}, {"t_end": T_KILL}))
        _skips(ps, cs, rs)
        assert cs["verified"]
        _same((order, geo, "pieces to T"), res, h, ores, oh)
        _skips(*_step(e)[2:])
        # the event cap inside the sweep: refused
        res, h, ps, cs, rs = _step(e, ({"max_events": cap},))
        _skips(ps, cs, rs)
        assert not cs["verified"] and e.sweep_stats()["killers"] == 0
        _same((order, geo, "cap"), res, h, res0, h0)
        res, h, ps, cs, rs = _step(e)
        _reset_only(ps, cs, rs)
        _same((order, geo, "after cap"), res, h, ores, oh)
        res, h, ps, cs, rs = _step(e)
        _skips(ps, cs, rs)
        _same((order, geo, "again"), res, h, ores, oh)


@pytest.mark.parametrize("geo,R", GEOS)
def test_setters_and_state_writing_calls(engine_mod, oracle_mod, geo, R):
    scn = _ring(40, R)
    ores, oh = _oracle(oracle_mod, scn, "fifo")
    with _engine(engine_mod, scn, "fifo", geo) as e, _engine(engine_mod, scn, "fifo", geo, prefix=False) as e0:

        def verified_step():
            out = _step(e)
            assert out[3]["verified"]
            return out

        _stores_all(*verified_step()[2:])
        _skips(*verified_step()[2:])
        # a tie-mode change and a counter base re-pilot: the pilot's apply stores everything
        for order in ("forkfirst", "fifo"):
            e.set_tie_mode(order)
            res, h, ps, cs, rs = verified_step()
            _stores_all(ps, cs, rs)
            _same((geo, order, "piloted"), res, h, *_oracle(oracle_mod, scn, order))
            res, h, ps, cs, rs = verified_step()
            _skips(ps, cs, rs)
            _same((geo, order, "applied"), res, h, *_oracle(oracle_mod, scn, order))
        e.set_counter_base(1000, 77)
        e0.set_counter_base(1000, 77)
        e0.reset()
        e0.run()
        res0, h0 = e0.results(), e0.hashes()
        for i in range(2):
            res, h, ps, cs, rs = verified_step()
            _stores_all(ps, cs, rs) if i == 0 else _skips(ps, cs, rs)
            _same((geo, "base", i), res, h, res0, h0)
        e.set_counter_base(0, 1)
        _stores_all(*verified_step()[2:])
        _skips(*verified_step()[2:])
        # calls between the verifying run and the next apply: none writes what
        # tw_reset fills, so the reset-valued rows stay skipped
        for name, call in (("set_prefix", lambda: e.set_prefix(True)), ("set_trace", lambda: e.set_trace(0)),
                           ("tie_audit", lambda: e.tie_audit(probes=1))):
            call()
            res, h, ps, cs, rs = verified_step()
            _reset_only(ps, cs, rs)
            _same((geo, name), res, h, ores, oh)
            res, h, ps, cs, rs = verified_step()
            _skips(ps, cs, rs)
            _same((geo, name, "again"), res, h, ores, oh)
        # read-only calls between them leave the verification alone
        e.results(); e.hashes(); e.prefix_stats(); e.prefix_rows_stats(); e.sweep_stats(); e.launch_ms()
        _skips(*verified_step()[2:])


# --------------------------------------------------- non-zero nv_init, a listen_init
@pytest.mark.parametrize("geo,R", [("dense", 301), ("narrow", 70)])
def test_reset_values_from_the_load(engine_mod, oracle_mod, geo, R):
    """Node variables that start non-zero on some nodes and a listener bound at
    t = 0 on main's node alone: tw_reset leaves those values, the snapshot
    still holds them (the program stores no variable), and the rows are
    skipped all the same; a variable row is of the class whatever its value."""
    K = 40
    base = units("plain", K, R, 1)
    nv = np.zeros((K + 1, 4), np.int64)
    nv[::3, 1] = 7
    nv[1::4, 2] = -5
    nv[K, 3] = 1 << 40
    listen = np.zeros(K + 1, np.uint32)
    listen[K] = 1  # (the program's one listener set, bound where no server binds it)
    scn = dataclasses.replace(base, name=base.name + "_init", node_vars=nv, node_listen=listen)
    ores, oh = oracle_mod.run_batch(scn, mode=ORACLE_MODE["fifo"], threads=8)
    res0, h0 = _off(engine_mod, scn, "fifo", geo)
    _same((geo, "off"), res0, h0, ores, oh)
    with _engine(engine_mod, scn, "fifo", geo) as e, _engine(engine_mod, base, "fifo", geo) as eb:
        _stores_all(*_step(e)[2:])
        _stores_all(*_step(eb)[2:])
        for i in range(2):
            res, h, ps, cs, rs = _step(e)
            _skips(ps, cs, rs)
            _same((geo, i), res, h, ores, oh)
            rsb = _step(eb)[4]
            # every variable row, zero or not, and main's node's bind row, bound or not:
            # the same rows as without the initial values
            assert rs["class_rows"]["reset"] >= 4 * (K + 1) + 1, rs
            assert rs["class_rows"]["reset"] == rsb["class_rows"]["reset"], (rs, rsb)
