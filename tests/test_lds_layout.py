"""The per-chain LDS layout of ``csrc/fc_lds.h`` (the ReCom and seed-plan kernels'), executed on the
CPU over a grid of shapes: ordering, alignment, totals against the closed forms the planner used
before and the room of the tree CSR; and ``frame_lds_bytes``, the frame-series kernel's staged
tables, at the shapes the series tests run (``tests/native/lds_layout_check.cpp``).  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


def test_lds_layout(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    exe = str(tmp_path / "lds_layout_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "native", "lds_layout_check.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    assert lines[-1].endswith("bad 0"), res.stdout
    # fc_bipartition.h's comment on its speculative child reads quotes these two
    assert "RMAX 8: speculative reads stay clear of par from npad - n >= 3" in res.stdout
    assert "RMAX 16: speculative reads stay clear of par from npad - n >= 5" in res.stdout
    # the frame-series kernel's staged tables: three shapes that fit, and the one that does not
    frames = [ln for ln in lines if ln.startswith("frame_lds_bytes ")]
    assert [ln.split(" = ")[1].split()[0] for ln in frames] == ["10496", "3264", "12800", "0"], res.stdout
    one = subprocess.run([exe, "frame", "256", "512", "14400", "152", "152", "1596"], capture_output=True, text=True,
                         timeout=120)
    assert one.returncode == 0
    assert one.stdout.splitlines() == ["frame_lds_bytes 256 512 14400 = 0", "frame_lds_bytes 152 152 1596 = 10496"]
