"""The load's host logic (csrc/load_plan.hpp), CPU only: a stand-alone program
built with ASan + UBSan runs the descriptor and argument checks, the two image
classifiers (classify_pcs: which events the wave kernel may batch;
classify_batch: which handlers tw_lp_due runs data-parallel), the batched
mode's plan and the geometry choice over hand-made inputs, and the classifiers
and the plan over real scenarios handed over as text: the CPU side of what
test_gpu_lpb.py asserts on the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from timewarp import isa, scenarios
from timewarp.engine import lpb_lookahead, lpb_short_link_destinations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("load") / "load_plan"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "load_plan_main.cpp")], check=True)
    return str(exe)


def _run(exe, path) -> dict:
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        out[key] = vals
    return out


def classify(exe, scn, path):
    """(classify_pcs's classes per pc, classify_batch's flags as [set][kind]) of the scenario's image"""
    img = scn.image
    with open(path, "w") as f:
        f.write(f"image {len(img.insns)} {img.n_listener_sets} {img.n_msg_kinds}\n")
        for w0, imm in img.insns.tolist():
            f.write(f"{w0} {imm - (1 << 32) if imm >= (1 << 31) else imm}\n")
        f.write(" ".join(str(int(x)) for x in img.listener_pc[:img.n_listener_sets].ravel()) + "\n")
    out = _run(exe, path)
    cls = np.array(out["cls"], int)
    bat = np.array(out["bat"], int).reshape(img.n_listener_sets, img.n_msg_kinds)
    assert cls.shape == (len(img.insns) + 1,) and cls[-1] == 0
    return cls, bat


def plan(exe, scn, lookahead, caps, path, outbox_cap=1 << 16):
    """tw_lpb_load's check and plan of the scenario"""
    lt = scn.link_table
    with open(path, "w") as f:
        f.write(f"plan {scn.n_nodes} {lt.shape[0]} {scn.n_replicas} {lt.shape[1]} {int(lookahead)} {outbox_cap}\n")
        for a in (scn.topo.out_off, scn.topo.dst, lt, np.broadcast_to(np.asarray(caps), (scn.n_nodes,))):
            f.write(" ".join(str(int(x)) for x in np.asarray(a).ravel()) + "\n")
    return _run(exe, path)


def _fields(out) -> dict:
    """the named values behind the plan's status"""
    return dict(zip(out["status"][1::2], out["status"][2::2]))


def test_hand_made_inputs_under_sanitizers(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "load plan ok" in r.stdout


def _handler(scn, name):
    """(set, kind) of the listener entries dispatching to the handler `name`"""
    img = scn.image
    lpc = img.listener_pc[:img.n_listener_sets]
    hit = np.argwhere((lpc != isa.PC_NONE) & ((lpc & ~np.uint32(isa.LPC_INLINE)) == img.pc_of(name)))
    assert hit.shape[0] >= 1
    return [tuple(x) for x in hit.tolist()]


def test_hotspot_ping_handler_is_batchable(plan_exe, tmp_path):
    # bench/Network's receiver: `reply Pong` behind two traces (test_lpb_batched_delivery_heavy_receiver)
    scn = scenarios.hotspot(n_senders=64, n_replicas=32, msg_num=60)
    cls, bat = classify(plan_exe, scn, tmp_path / "spot.txt")
    for s, k in _handler(scn, "on_ping"):
        assert bat[s, k] == 1
    # the fixed stubs: the deliverer's resume is a DELIVER step, the watchdog's fire runs alone
    assert cls[isa.PC_DELIVER_STUB + 1] == 2 and cls[isa.PC_WATCHDOG_STUB + 1] == 0


def test_hotspot_counting_handler_is_not(plan_exe, tmp_path):
    # the handler stores to a node variable (test_lpb_batched_delivery_refuses_a_stateful_handler)
    scn = scenarios.hotspot(n_senders=64, n_replicas=16, msg_num=40, receiver_counter=True)
    _, bat = classify(plan_exe, scn, tmp_path / "count.txt")
    for s, k in _handler(scn, "on_ping"):
        assert bat[s, k] == 0


def test_hotspot_inline_handler_is_not(plan_exe, tmp_path):
    # ForkStrategy `const id`: the handler runs in the deliverer; every DELIVER step then runs alone
    scn = scenarios.hotspot(n_senders=8, n_replicas=8, msg_num=10, fork_strategy="inline")
    cls, bat = classify(plan_exe, scn, tmp_path / "inline.txt")
    for name in ("on_ping", "on_pong"):
        for s, k in _handler(scn, name):
            assert bat[s, k] == 0
    assert cls[isa.PC_DELIVER_STUB + 1] == 0


def test_token_ring_plan(plan_exe, tmp_path):
    # test_lpb_host.py's ring: only the observer, fed by 0 µs links, runs in phase 1
    N = 16
    scn = scenarios.token_ring(n_nodes=N, n_replicas=8, launch_duration=5_000_000)
    L = lpb_lookahead(scn)
    out = plan(plan_exe, scn, L, scn.meta.get("lp_inbox_cap", 32), tmp_path / "ring.txt")
    assert out["check"] == ["0"]
    st = _fields(out)
    assert out["status"][0] == "0" and st["rep_lg"] == "3" and st["has_ph1"] == "1"
    assert [int(x) for x in out["phase1"]] == lpb_short_link_destinations(scn, L).tolist() == [N]
    caps = np.broadcast_to(np.asarray(scn.meta.get("lp_inbox_cap", 32)), (scn.n_nodes,))
    off = np.array(out["ib_off"], np.int64)
    assert off.tolist() == [0] + np.cumsum(caps).tolist()
    assert int(st["ib_entries"]) == int(off[-1]) * 8 and st["heavy_ok"] == str(int((caps > 32).any()))


def test_hotspot_plan_and_refusals(plan_exe, tmp_path):
    scn = scenarios.hotspot(n_senders=32, n_replicas=16, msg_num=10)
    caps = scn.meta["lp_inbox_cap"]
    out = plan(plan_exe, scn, lpb_lookahead(scn), caps, tmp_path / "spot.txt")
    st = _fields(out)
    assert out["check"] == ["0"] and out["status"][0] == "0"
    assert st["has_ph1"] == "0" and st["heavy_ok"] == "1" and out["phase1"] == []
    assert [int(x) for x in out["ib_off"]] == [0] + np.cumsum(caps).tolist()
    # six replicas are no power of two: refused by the check (tw_lpb_load keeps the previous load)
    bad = scenarios.hotspot(n_senders=8, n_replicas=6, msg_num=10)
    assert plan(plan_exe, bad, lpb_lookahead(bad), 32, tmp_path / "six.txt")["check"] == ["-1"]
    # a cap of 0 and a cap above the heavy cap
    for cap in (0, 2049):
        c = np.array(caps).copy()
        c[0] = cap
        assert plan(plan_exe, scn, lpb_lookahead(scn), c, tmp_path / "cap.txt")["check"] == ["-1"]


def test_short_link_out_of_a_phase1_node(plan_exe, tmp_path):
    # test_lpb_rejects_short_link_out_of_phase1: the check passes, the plan refuses
    scn = scenarios.gossip(n_nodes=64, fanout=2)
    lt = scn.link_table.copy()
    l_ab = int(scn.topo.out_off[0])
    l_bc = int(scn.topo.out_off[int(scn.topo.dst[l_ab])])
    lt[l_ab] = 0
    lt[l_bc] = 0
    scn.link_table = lt
    out = plan(plan_exe, scn, 1000, 32, tmp_path / "gossip.txt")
    assert out["check"] == ["0"] and out["status"][0] == "-1"
