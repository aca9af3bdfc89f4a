"""The kill table and the claimed slots of a snapshot (csrc/prefix_clean.hpp,
DESIGN §3o), CPU only: a stand-alone program built with ASan + UBSan builds
them from hand-made parked states (one and two refs, a stale ref, a victim
that is not queued, main or slot 0 as victim, a victim named twice, a run
window that wraps its ring, no entry at T, operands out of range) and, for the
token-ring image at 4 and 40 nodes, from a parked state laid out around the
image's own kill stub and sweep time (the real snapshot is the GPU tests')."""
import os
import shutil
import subprocess

import pytest

from timewarp import scenarios
from timewarp.timeunits import sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def clean_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("clean") / "clean"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "prefix_clean_main.cpp")], check=True)
    return str(exe)


def test_hand_made_snapshots_under_sanitizers(clean_exe):
    r = subprocess.run([clean_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clean ok" in r.stdout


@pytest.mark.parametrize("n_nodes", [4, 40])
def test_token_ring_image(clean_exe, tmp_path, n_nodes):
    scn = scenarios.token_ring(n_nodes=n_nodes, n_replicas=1, launch_duration=sec(20))
    img = scn.image
    path = tmp_path / "ring.txt"
    with open(path, "w") as f:
        f.write(f"{len(img.insns)} {len(img.consts)}\n")
        for w0, imm in img.insns.tolist():
            f.write(f"{w0} {imm - (1 << 32) if imm >= (1 << 31) else imm}\n")
        f.write("\n".join(str(int(k)) for k in img.consts) + "\n")
    r = subprocess.run([clean_exe, str(path), str(n_nodes)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(zip(r.stdout.split()[::2], (int(x) for x in r.stdout.split()[1::2])))
    k = n_nodes + 1
    assert got == {"positions": k, "claimable": k, "claimed": 3 * k, "tagged": 9 * k}
