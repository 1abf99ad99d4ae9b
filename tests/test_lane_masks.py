"""The lane-range masks of the k = 2 flip kernel's lean instances (``csrc/fc_lane_mask.h``) on the
host: every form against its definition -- bit l set iff lo <= l < hi -- for every n in [0, 64] and
every pair 0 <= lo, hi <= 64 (``tests/native/lane_mask_check.cpp``).  The header is plain C++, so the
kernel's expressions are the ones that run here.  The program is built once plain and once with the
address and undefined-behaviour sanitizers (a shift by 64 would stop it) and run stand-alone.
CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


def _build(out, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-I", CSRC, "-o", out,
                    os.path.join(HERE, "native", "lane_mask_check.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    return _build(str(tmp_path_factory.mktemp("lane_mask") / "lane_mask_check"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    return _build(str(tmp_path_factory.mktemp("lane_mask_san") / "lane_mask_check_san"),
                  ("-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    last = res.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and last[2:] == ["bad", "0"], res.stdout
    # 2 * 65 + 4 * 64 single bounds, 65 * 65 + 2 * 64 * 65 + 2 * 64 * 64 ranges
    assert int(last[1]) == 2 * 65 + 4 * 64 + 65 * 65 + 2 * 64 * 65 + 2 * 64 * 64
    return int(last[1])


def test_masks_match_their_definition(exe):
    print(f"lane masks: {_run(exe)} checks")


def test_sanitized_stand_alone_program(exe_san):
    _run(exe_san)
