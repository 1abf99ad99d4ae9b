"""``philox_round_keys`` followed by the keyed round function (``philox4x32_10_keys``, the form
the k = 2 flip kernel calls with its key-table argument) is the same function of (counter, seed)
as ``philox4x32_10``: 1,000 random pairs and two corners, compiled as host code
(``tests/native/philox_keys_check.cpp``).  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


def test_philox_round_keys(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    exe = str(tmp_path / "philox_keys_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "native", "philox_keys_check.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("pairs 1002 bad 0"), res.stdout
