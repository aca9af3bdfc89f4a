"""The killThread sweep's load-time classifier (csrc/sweep_classify.hpp), CPU
only: a stand-alone program built with ASan + UBSan runs it over hand-made
images (stubs of 0 to 3 throwTos, a stub behind a conditional jump, a wait
without a constant, more sweep times than the cap) and over the token-ring
image, whose kill pair and launch duration it must find."""
import os
import shutil
import subprocess

import pytest

from timewarp import isa, scenarios
from timewarp.timeunits import sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def classify_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("sweep") / "classify"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "sweep_classify_main.cpp")], check=True)
    return str(exe)


def test_hand_made_images_under_sanitizers(classify_exe):
    r = subprocess.run([classify_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "classify ok" in r.stdout


def test_token_ring_image(classify_exe, tmp_path):
    launch = sec(120)
    scn = scenarios.token_ring(n_nodes=8, n_replicas=1, launch_duration=launch)
    img = scn.image
    path = tmp_path / "ring.txt"
    with open(path, "w") as f:
        f.write(f"{len(img.insns)} {len(img.consts)}\n")
        for w0, imm in img.insns.tolist():
            f.write(f"{w0} {imm - (1 << 32) if imm >= (1 << 31) else imm}\n")
        f.write("\n".join(str(int(k)) for k in img.consts) + "\n")
    r = subprocess.run([classify_exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) if " " in l else (l, "") for l in r.stdout.strip().split("\n"))
    assert [int(t) for t in lines["times"].split()] == [launch]
    stubs = {int(s.split(":")[0]): tuple(int(x) for x in s.split(":")[1:]) for s in lines["stubs"].split()}
    kp = img.pc_of("kill_pair")
    # the pair itself (throwTo r1 ; throwTo r2 ; END), its second half, and the
    # `wait (at launchDuration) ; jmp kill_pair` stubs of the two `schedule`s
    assert stubs[kp] == (2, 1, 2)
    assert stubs[kp + 1][0] == 1 and stubs[kp + 1][1] == 2
    jumps = [pc for pc in stubs if pc not in (kp, kp + 1)]
    assert len(jumps) == 2
    for pc in jumps:
        assert stubs[pc] == (2, 1, 2)
        assert img.insns[pc][0] & 0xFF == isa.OP_JMP and img.insns[pc][1] == kp
        assert img.insns[pc - 1][0] & 0xFF == isa.OP_WAIT_ABS
