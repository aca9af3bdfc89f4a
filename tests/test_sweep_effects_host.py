"""The effects table beside the kill table (csrc/prefix_clean.hpp),
CPU only: a stand-alone program built with ASan + UBSan builds it from
hand-made parked states (one and two refs; killer and victims on one, two and
three nodes: the merged hash adds; F_OWNS on the killer, a victim, all three;
the static verdict of victims with a frame that catches ThreadKilled, a finally
frame, three frames, an exception pending, not started, a kill-stub entry, a
node out of range; a victim named by two positions and by both refs of one:
not exclusive; a window that wraps its ring; operands out of range and a table
whose rows are gone) and, for the token-ring image at 4 and 40 nodes, from a
parked state laid out around the image's own kill stub and sweep time."""
import os
import shutil
import subprocess

import pytest

from timewarp import scenarios
from timewarp.timeunits import sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def effects_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("effects") / "effects"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "sweep_effects_main.cpp")], check=True)
    return str(exe)


def test_hand_made_snapshots_under_sanitizers(effects_exe):
    r = subprocess.run([effects_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "effects ok" in r.stdout


@pytest.mark.parametrize("n_nodes", [4, 40])
def test_token_ring_image(effects_exe, tmp_path, n_nodes):
    scn = scenarios.token_ring(n_nodes=n_nodes, n_replicas=1, launch_duration=sec(20))
    img = scn.image
    path = tmp_path / "ring.txt"
    with open(path, "w") as f:
        f.write(f"{len(img.insns)} {len(img.consts)}\n")
        for w0, imm in img.insns.tolist():
            f.write(f"{w0} {imm - (1 << 32) if imm >= (1 << 31) else imm}\n")
        f.write("\n".join(str(int(k)) for k in img.consts) + "\n")
    r = subprocess.run([effects_exe, str(path), str(n_nodes)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(zip(r.stdout.split()[::2], (int(x) for x in r.stdout.split()[1::2])))
    k = n_nodes + 1
    # every position claimable and exclusive; killer and victims on one node:
    # one add with two ThreadKilled terms; the second victim owns its listener
    assert got == {"positions": k, "rows": k, "verdict": k, "exclusive": k, "adds": k, "kills": 2 * k,
                   "releases": k, "all_exclusive": 1}
