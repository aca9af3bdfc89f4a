"""The class of every row of a snapshot's directory (csrc/prefix_clean.hpp
clean_classes), CPU only: a stand-alone program built with ASan +
UBSan classifies hand-made parked states (header rows of claimed slots only,
never slot 0; run entries of claimable positions only, tagged with their
killers, over a window that wraps its ring; the observer's position; the
arrays tw_reset fills with zero and non-zero nv_init, with and without
listen_init, bind_own / bind_rel at and away from their constants, tmo_done;
rows the directory lacks, operands out of range) and, for the token-ring image
at 4 and 40 nodes, a parked state laid out around the image's own kill stub
and sweep time as tests/prefix_clean_main.cpp lays it out."""
import os
import shutil
import subprocess

import pytest

from timewarp import scenarios
from timewarp.timeunits import sec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("rows") / "rows"
    # (the runtimes linked statically: the program then runs the same whatever
    # else the environment loads ahead of it)
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "prefix_rows_main.cpp")], check=True)
    return str(exe)


def test_hand_made_classes_under_sanitizers(rows_exe):
    r = subprocess.run([rows_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows ok" in r.stdout


@pytest.mark.parametrize("n_nodes", [4, 40])
def test_token_ring_image(rows_exe, tmp_path, n_nodes):
    scn = scenarios.token_ring(n_nodes=n_nodes, n_replicas=1, launch_duration=sec(20))
    img = scn.image
    path = tmp_path / "ring.txt"
    with open(path, "w") as f:
        f.write(f"{len(img.insns)} {len(img.consts)}\n")
        for w0, imm in img.insns.tolist():
            f.write(f"{w0} {imm - (1 << 32) if imm >= (1 << 31) else imm}\n")
        f.write("\n".join(str(int(k)) for k in img.consts) + "\n")
    r = subprocess.run([rows_exe, str(path), str(n_nodes)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(zip(r.stdout.split()[::2], (int(x) for x in r.stdout.split()[1::2])))
    k = n = n_nodes + 1
    # k kill wakes with two victims each and the observer's, which claims nothing;
    # of tw_reset's arrays: variables 1 - 3 and bind_rel of every node, two timeouts
    assert got == {"positions": k + 1, "claimable": k, "hdr": 3 * k, "body": 9 * k, "run": k,
                   "reset": 4 * n + 2, "reset_bytes": 28 * n + 2}
