"""bench.py --dump-outputs (bench.dump_outputs): the last launch's chain states and per-chain
statistics as float32 / float64 .npy files within the byte budget, identical from call to call; a
state beyond the budget is written for a fixed sample of chains."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Run:
    """Stands in for FlipRun: dump_outputs reads only state()."""

    def __init__(self, chains, n):
        self._s = (np.arange(chains * n, dtype=np.int64).reshape(chains, n) % 5 - 1).astype(np.int8)

    def state(self):
        return self._s.copy()


def _stats(chains):
    return {"steps": np.full(chains, 1000, dtype=np.int64), "sum_wait": np.arange(chains, dtype=np.int64) << 40,
            "cut": np.arange(chains, dtype=np.int32)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_state_and_stats(tmp_path):
    run, st = _Run(37, 101), _stats(37)
    rec = bench.dump_outputs(str(tmp_path / "a"), run, st)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == ["state", "state_chains", "stats_cut", "stats_steps", "stats_sum_wait"]
    assert got["state"].dtype == np.float32 and np.array_equal(got["state"], run.state())
    assert np.array_equal(got["state_chains"], np.arange(37)) and not rec["state_sampled"]
    for k, v in st.items():
        assert got["stats_" + k].dtype == np.float64 and np.array_equal(got["stats_" + k], v)
    assert rec["files"] == 5 and rec["bytes"] == sum(a.nbytes for a in got.values())


def test_dump_samples_a_state_beyond_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40000)
    run, st = _Run(200, 101), _stats(200)
    rec = bench.dump_outputs(str(tmp_path / "a"), run, st)
    bench.dump_outputs(str(tmp_path / "b"), run, st)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    size = sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a"))
    assert size <= 40000 and rec["state_sampled"]
    ids = a["state_chains"].astype(np.int64)
    assert 1 <= len(ids) < 200 and np.all(np.diff(ids) > 0) and ids.max() < 200
    assert np.array_equal(a["state"], run.state()[ids])
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the same sample every time
    assert len(a["stats_cut"]) == 200  # the statistics of every chain


def test_dump_ranks_write_their_own_files(tmp_path):
    bench.dump_outputs(str(tmp_path), _Run(4, 9), _stats(4), rank=1, world=2)
    assert "state_rank1.npy" in os.listdir(tmp_path) and "state.npy" not in os.listdir(tmp_path)
