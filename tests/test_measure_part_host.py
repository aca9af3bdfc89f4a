"""tw_measure's partition path, CPU only: the HIP-free half the host and the
kernels share (csrc/measure_part.hpp: the bijective id mixer, buckets(m), the
bucket of an id, the limits) in a stand-alone program built with ASan + UBSan,
and the Python mirror of the new limit against the header."""
import os
import re
import shutil
import subprocess

from timewarp import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_arithmetic_under_sanitizers(tmp_path):
    """buckets(m) at its edges, mix / unmix round trips, and for the id
    families the scenarios and the scripted tests produce (consecutive,
    C5's 1..256,000 at 512,000 keys, strided from 1 << 40, negative multiples,
    multiples of 2^20) at their buckets(m): no bucket gets more distinct ids
    than the LDS table has slots."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "part"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-o", str(exe),
                    os.path.join(ROOT, "tests", "measure_part_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "part ok" in r.stdout
    full = [int(m) for m in re.findall(r"fullest (\d+) of 2048 slots", r.stdout)]
    assert len(full) == 5 and 0 < min(full) and max(full) <= 2048


def test_limit_matches_the_header():
    text = open(os.path.join(ROOT, "include", "timewarp.h")).read()
    assert int(re.search(r"#define TW_MEASURE_MAX_KEYS_LARGE (\d+)u", text).group(1)) == abi.MEASURE_MAX_KEYS_LARGE
    assert abi.MEASURE_MAX_KEYS_LARGE == 4096 * 1024 > abi.MEASURE_MAX_KEYS
    assert re.search(r"int tw_set_measure_keys\(tw_ctx\* ctx, uint32_t max_keys\);", text)
