"""``log_cr`` (fc_philox.h): the correctly rounded logarithm a kernel takes where a geometric wait's
quotient ``log(1 - U) / log(1 - p)`` lies within the device log's one-ulp error of an integer, so
that its ceiling is the host's (the oracle's, numpy's).  Compiled as host code
(``tests/native/log_cr_check.cpp``) and compared with correctly rounded values on inputs within
10^-4 ulp of a rounding tie, and with the host's ``log`` on two million inputs: the two may differ
only where the host's own log is misrounded (glibc: below 0.1 % of inputs), and then by one ulp.
CPU only; the device side is pinned by the 8 x 8, k = 8 cases of test_flip_edges_gpu.py."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


def test_log_cr_is_correctly_rounded(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    exe = str(tmp_path / "log_cr_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe, os.path.join(HERE, "native", "log_cr_check.cpp")],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.search(r"vectors (\d+) bad (\d+); random (\d+) differ (\d+) far (\d+)$", res.stdout.strip())
    assert m, res.stdout
    vectors, bad, n, differ, far = (int(x) for x in m.groups())
    assert vectors >= 50 and bad == 0 and far == 0 and n > 1900000, res.stdout
    assert differ <= n // 1000, res.stdout
