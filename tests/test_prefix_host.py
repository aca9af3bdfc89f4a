"""The send-free prefix's load-time bound (csrc/prefix_classify.hpp), CPU
only: a stand-alone program built with ASan + UBSan runs it over hand-made
images (a send at t = 0, behind each kind of wait, in a forked child, in a
catch handler a throwTo reaches at t = 0, in a timeout's handler, only in a
listener handler, none at all, operands out of range) and over the token-ring
and ping-pong images, whose first sends' times are read off their programs."""
import os
import shutil
import subprocess

import pytest

from timewarp import scenarios
from timewarp.timeunits import sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def classify_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("prefix") / "classify"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "prefix_classify_main.cpp")], check=True)
    return str(exe)


def image_t0(exe, scn, path) -> int:
    img = scn.image
    with open(path, "w") as f:
        f.write(f"{len(img.insns)} {len(img.consts)} {scn.main_pc}\n")
        for w0, imm in img.insns.tolist():
            f.write(f"{w0} {imm - (1 << 32) if imm >= (1 << 31) else imm}\n")
        f.write("\n".join(str(int(k)) for k in img.consts) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    key, val = r.stdout.strip().split()
    assert key == "t0"
    return int(val)


def test_hand_made_images_under_sanitizers(classify_exe):
    r = subprocess.run([classify_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prefix ok" in r.stdout


@pytest.mark.parametrize("n_nodes", [4, 4096])
def test_token_ring_image(classify_exe, tmp_path, n_nodes):
    # the first send is node 0's `invoke (after 1 sec)` (launch_node): the forks
    # in front of it count for nothing in the bound; the worker's sends sit in
    # a handler only accept_token's throwTo reaches, a listener handler
    scn = scenarios.token_ring(n_nodes=n_nodes, n_replicas=1, launch_duration=sec(120))
    assert image_t0(classify_exe, scn, tmp_path / "ring.txt") == 1_000_000


def test_ping_pong_image(classify_exe, tmp_path):
    # ping_main: `wait (for 2 sec)`, then `send Ping`; every other send is in a listener handler
    scn = scenarios.ping_pong(n_replicas=1)
    assert image_t0(classify_exe, scn, tmp_path / "pp.txt") == sec(2)
