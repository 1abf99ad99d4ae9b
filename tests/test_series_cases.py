"""The series-kernel case table on the CPU: every case's oracle run reaches the branch the case is
for (``series_cases.CASES`` drives the device parity test, test_series_edges_gpu.py), the kernel
takes its frame tables from LDS or from global memory as the case says (``frame_lds_bytes`` of
``csrc/fc_lds.h``, asked of ``tests/native/lds_layout_check.cpp``), and the model's change points
and queue bookkeeping count what they say on key lists short enough to count by hand.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import series_cases as SC
import series_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "flipcomplexityempirical_amd", "csrc")


@pytest.mark.parametrize("name", list(SC.BY_NAME))
def test_case_reaches_its_branch(name):
    """A failure here means the case is wrong (graph, plans, frame, bases, seed or steps), not the kernel."""
    case = SC.BY_NAME[name]
    assert 1 <= case.n_chains <= 16 and case.steps <= 8200
    assert list(case.reads) == sorted(set(case.reads)) and case.reads[0] >= 0
    for parts, s in case.launches():
        assert all(p > 0 for p in parts) and len(parts) <= case.split
    assert sum(sum(p) for p, _ in case.launches()) == case.reads[-1]
    infos = [case.info(c) for c in range(case.n_chains)]
    for c, i in enumerate(infos):
        assert i["T"] == case.reads[-1] + 1 == len(i["x"]) and int(i["x"].max()) < 65536
        ev = i["events"]
        assert np.all(np.diff(ev[:, 0]) > 0) and (len(ev) == 0 or (case.t0 < ev[0, 0] and ev[-1, 0] <= case.steps))
    assert case.run_ok(case, infos), name
    if "cycle" in name:  # |cut| = 2 whatever the plan: every valid proposal is accepted
        for c, i in enumerate(infos):
            assert len(i["events"]) == case.reads[-1], (name, c)
            assert np.array_equal(i["events"][:, 0], case.t0 + 1 + np.arange(case.reads[-1]))
            assert set(i["x"].tolist()) == {2}


def test_table_holds_what_the_kernels_turn_on():
    names = set(SC.BY_NAME)
    assert {f"cycle256 prefix F={F}" for F in (0, 1, 2, 64, 65, 128, 129, 192, 193, 255, 256)} <= names
    for T in (1, 2, 4095, 4096, 4097, 8192, 8193):
        for split in (1, 3):
            case = SC.BY_NAME[f"lag T={T} launches={split}"]
            assert case.reads[-1] + 1 == T and len(case.launches()[0][0]) == min(split, T - 1)
    assert SC.BY_NAME["cycle65 ladder"].reads == (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1500)
    assert SC.BY_NAME["cycle65 ladder"].pre == 0  # the window is opened by series_reset()
    after = SC.BY_NAME["lag window after 1000"]
    assert after.pre == 1000 and after.reads == (0, 1, 4096)
    assert SC.lags_for(4097) == [0, 1, 2, 4095, 4096, 4097, 4098, 2 ** 31 - 1]
    assert SC.lags_for(1) == [0, 1, 2, 4095, 4096, 4097, 2 ** 31 - 1]
    fr = SC.BY_NAME["grid120x120 global tables"].frame_set()["disjoint 256"]
    assert len(fr.eu) == 256 and len(set(fr.eu.tolist()) | set(fr.ev.tolist())) == 512
    for name in ("grid12x12 dense",):
        for fr in SC.BY_NAME[name].frame_set().values():
            assert len(fr.eu) == 256


def test_frame_tables_in_lds_except_the_global_case(tmp_path):
    """Which kernel instance a case runs (tables staged in LDS, or read from global memory when
    they do not fit) by the kernel's own host-side rule."""
    if shutil.which("g++") is None:
        pytest.skip("no host C++ toolchain")
    exe = str(tmp_path / "lds_layout_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe,
                    os.path.join(HERE, "native", "lds_layout_check.cpp")], check=True)
    shapes = []
    for case in SC.CASES:
        for fname, fr in case.frame_set().items():
            rows = len(set(fr.eu.tolist()) | set(fr.ev.tolist()))
            shapes.append((case, fname, (len(fr.eu), rows, case.spec.n)))
    args = [str(x) for _, _, s in shapes for x in s]
    res = subprocess.run([exe, "frame"] + args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(shapes)
    seen_global = 0
    for (case, fname, s), ln in zip(shapes, lines):
        head, val = ln.split(" = ")
        assert head == "frame_lds_bytes %d %d %d" % s
        assert (int(val) == 0) == case.global_tables, (case.name, fname, ln)
        seen_global += case.global_tables
    assert seen_global == 1


def test_queue_profile_on_hand_made_keys():
    """130 events (3 chunks: wave 0 has none, wave 1 chunk 0, wave 2 chunk 1, wave 3 chunk 2 with
    two events).  Keys: the window start's 7; events 0-63 alternate 1, 2 (64 candidates: one flush,
    rest 0, tail 0); events 64-127 hold 2 except events 70 and 71 (3, then 2 again: candidates 70,
    71; event 64 equals event 63's 2: none): tail 2; events 128, 129: 2 and 5: tail 1."""
    keys = [7] + [1 + (i & 1) for i in range(64)] + [2] * 64 + [2, 5]
    keys[1 + 70] = 3
    assert M.queue_profile(keys) == ([0], [0, 0, 2, 1])
    # 8 chunks, two per wave, every other event a candidate (32 per chunk): each wave's queue
    # reaches 64 on its second chunk and flushes to rest 0, but for wave 0, which has one more
    # candidate: 65, rest 1, tail 1
    keys = [9] + [i // 2 % 2 for i in range(512)]
    keys[2] = 5  # event 1: one more candidate in chunk 0 (event 2 is one either way)
    assert M.queue_profile(keys) == ([1, 0, 0, 0], [1, 0, 0, 0])
    # two chunks of 64 candidates in one wave's range after 1 left over: rests stay 1
    keys = [0] + [1 + (i & 1) if i >= 63 else 0 for i in range(64 * 12)]
    rests, tails = M.queue_profile(keys)
    assert rests[:2] == [1, 1] and tails[0] == 1 and len(rests) == 11  # wave 0: 1, 1 + 64, 1 + 64; the others 3 x 64
    assert M.queue_profile([4]) == ([], [0, 0, 0, 0])
    assert M.queue_profile([4, 4]) == ([], [0, 0, 0, 0]) and M.queue_profile([4, 5]) == ([], [0, 0, 0, 1])


def test_frame_changes_on_a_hand_made_series():
    """Eight entries: the start; the same values; another slope; NaN, NaN (one change: NaN equals
    NaN); -0.0 after 0.0 in the angle (a change: other bits); the same again."""
    nan = math.nan
    dense = {"slope": np.asarray([1.0, 1.0, 2.0, nan, nan, 3.0, 3.0, 3.0]),
             "angle": np.asarray([0.5, 0.5, 0.5, nan, nan, 0.0, -0.0, -0.0])}
    ch = M.frame_changes(dense, 10, [11, 13, 14, 20, 21, 30, 31])
    assert ch["index"].tolist() == [0, 2, 3, 5, 6] and ch["t"].tolist() == [10, 13, 14, 21, 30]
    assert ch["slope"].tolist()[:2] == [1.0, 2.0] and math.isnan(ch["slope"][2]) and math.copysign(1, ch["angle"][4]) == -1


def test_frame_dense_on_a_hand_made_window():
    """A 6-cycle, frame = ring edges 0, 2, 3, 5 (in that order) with midpoints (0, 0), (1, 1),
    (1, 3), (3, 3) about the centre (1, 1).  District 1 = {1, 2}: ring edges 0 and 2 cut, frame
    edges 0 and 1 (slope 1; b is the centre: NaN angle).  Node 3 joins: ring edges 0 and 3, frame
    edges 0 and 2 (slope 3; vectors (-1, -1) and (0, 2): 3 pi / 4).  Node 0 joins: ring edges 3 and
    5, frame edges 2 and 3 (slope 0; vectors (0, 2) and (2, 2): pi / 4).  Node 1 leaves: ring edges
    0, 1, 3, 5 are cut, frame edges 0, 2, 3 (ring edge 1 is no frame edge): the first two again."""
    fu, fv = [0, 2, 3, 5], [1, 3, 4, 0]
    mid = [(0.0, 0.0), (1.0, 1.0), (1.0, 3.0), (3.0, 3.0)]
    a0 = [0, 1, 1, 0, 0, 0]
    events = np.asarray([(1, 3, 2, 4, 1), (2, 0, 2, 4, 1), (3, 1, 4, 6, 0)])
    d = M.frame_dense(a0, events, fu, fv, mid, (1.0, 1.0))
    assert d["n_cut"].tolist() == [2, 2, 2, 3]
    assert d["key"].tolist() == [0 | 1 << 16, 0 | 2 << 16, 2 | 3 << 16, 0 | 2 << 16]
    assert d["slope"].tolist() == [1.0, 3.0, 0.0, 3.0]
    assert math.isnan(d["angle"][0]) and d["angle"][1] == d["angle"][3] == pytest.approx(3 * math.pi / 4, abs=1e-15)
    assert d["angle"][2] == pytest.approx(math.pi / 4, abs=1e-15)
    x = M.cut_yields(2, events, 0, 5)
    assert x.tolist() == [2, 2, 2, 4, 4]
