"""The seed-plan case table shared by test_seed_cases.py (CPU: the model reaches the branch each
case is for, and its plans are valid by the definition) and test_seed_gpu.py (the device equals
the model on every plan of every case).

A case fixes the graph, k, the inclusive population bounds, the parameters and the plans of one
launch, and states the coverage condition ``ok(case, results)`` that the model's results (one
dict per plan, tests/seed_model.py) must meet.  A condition that fails means the case is wrong
(change the case, never the condition).  The shapes are the smallest at which the kernel can still
go wrong; the model's results are computed once per case and shared.
"""
import dataclasses
import functools
from typing import Callable, Optional, Tuple

import numpy as np

import recom_cases as RC
import seed_model
from flipcomplexityempirical_amd import graphs as G

SEED = 77


# ---- graphs -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def p3_141():
    """Path of three nodes with populations 1, 4, 1."""
    return dataclasses.replace(RC.path(3), pop=np.asarray([1, 4, 1], dtype=np.int32))


# ---- coverage conditions ----------------------------------------------------------------
def all_ok(case, res):
    return all(r["ok"] == 1 for r in res)


def re_rooted(case, res):
    return all_ok(case, res) and any(r["attempts"] > r["trees"] > case.k - 1 for r in res)


def restarted(case, res):
    return all_ok(case, res) and any(r["restarts"] > 0 for r in res)


def some_restart(case, res):
    return any(r["restarts"] > 0 for r in res)


def mixed(case, res):
    return any(r["ok"] == 1 for r in res) and any(r["ok"] == 0 for r in res)


def hopeless(case, res):
    return all(r["ok"] == 0 and r["attempts"] == 9 for r in res)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    graph: Callable                 # () -> GraphSpec
    k: int
    ok: Callable                    # (case, [model result per plan]) -> bool
    lohi: Optional[Tuple[int, int]] = None  # inclusive bounds ...
    pct: Optional[float] = None     # ... or within pct of ideal (graphs.population_bounds)
    node_repeats: int = 1
    max_attempts: int = 0           # 0: the default (256)
    max_restarts: int = 0           # 0: the default (16)
    n_plans: int = 5                # one full 4-wave block and a partial one at small n
    plan_id_offset: int = 0
    kernel: str = "fc::seed_kernel<8>"

    @property
    def spec(self):
        return self.graph()

    @property
    def bounds(self):
        if self.lohi is not None:
            return tuple(self.lohi)
        return G.population_bounds(int(self.spec.pop.astype(np.int64).sum()), self.k, self.pct)[1]

    @property
    def params(self):
        return {"node_repeats": self.node_repeats, "max_attempts": self.max_attempts, "max_restarts": self.max_restarts}

    def model(self):
        """The model's results, one per plan (computed once)."""
        return _model(self.name)


@functools.lru_cache(maxsize=None)
def _model(name):
    c = BY_NAME[name]
    lo, hi = c.bounds
    return tuple(seed_model.seed_plans(c.spec, c.k, lo, hi, SEED, c.n_plans, c.plan_id_offset, **c.params))


def _grid(gx, gy):
    return functools.partial(RC.grid, gx, gy)


CASES = [
    # sizes (n < 16: one 16-node pad)
    Case("size 2x2 k=2", _grid(2, 2), 2, all_ok, lohi=(1, 3)),
    Case("size 3x1 k=2", _grid(3, 1), 2, all_ok, lohi=(1, 2)),
    Case("size 3x4 k=3", _grid(3, 4), 3, all_ok, lohi=(3, 5)),
    Case("size 4x4 k=4", _grid(4, 4), 4, all_ok, lohi=(3, 5)),
    Case("size 7x9 k=3", _grid(7, 9), 3, all_ok, pct=0.1),
    Case("size 8x8 k=4", _grid(8, 8), 4, all_ok, lohi=(15, 17)),
    Case("size 13x5 k=4", _grid(13, 5), 4, all_ok, pct=0.2),
    Case("size 16x16 k=4", _grid(16, 16), 4, all_ok, pct=0.1),
    # trees of maximal depth
    Case("path P16 k=4", functools.partial(RC.path, 16), 4, all_ok, lohi=(3, 5)),
    Case("cycle C32 k=4", functools.partial(RC.cycle, 32), 4, all_ok, lohi=(7, 9)),
    # a second root on the same tree, then new trees
    Case("re-root 8x8 k=4", _grid(8, 8), 4, re_rooted, lohi=(16, 16), node_repeats=2),
    # a level without a cut in max_attempts: the plan starts again
    Case("restart 8x8 k=4", _grid(8, 8), 4, restarted, lohi=(16, 16), max_attempts=2, max_restarts=16),
    # plans that succeed and plans that fail side by side in one launch
    Case("mixed 8x8 k=4", _grid(8, 8), 4, mixed, lohi=(16, 16), max_attempts=1, max_restarts=1),
    # passes the host checks (3 * 2 = 6 = total) and cannot succeed: 3 attempts in each of 3 runs
    Case("hopeless P3 k=3", p3_141, 3, hopeless, lohi=(2, 2), max_attempts=3, max_restarts=2),
    # a two-node remainder has no inner node (the root rule of gerrychain 0.2): the restart covers it
    Case("no inner node 4x2 k=4", _grid(4, 2), 4, some_restart, lohi=(1, 3), max_attempts=20),
    # a real dead end: a legal first cut whose remainder cannot be split
    Case("dead end weights 9x7 k=3", RC.weighted_grid, 3, some_restart, pct=0.2, max_attempts=40, max_restarts=8),
    # population totals next to 2^31
    Case("top of range 4x4 k=2", RC.heavy_grid, 2, all_ok, pct=0.4),
    # degree-wide rows
    Case("delaunay200 k=6", RC.delaunay200, 6, all_ok, pct=0.1, kernel="fc::seed_kernel<16>"),
    # the largest k
    Case("k=32 16x16", _grid(16, 16), 32, all_ok, lohi=(4, 12)),
    # ten blocks of which the last holds one wave; plan ids from 1000
    Case("many blocks 8x8 k=2", _grid(8, 8), 2, all_ok, pct=0.1, n_plans=37, plan_id_offset=1000),
    # the LDS limit: one wave per block, tree offsets up to 2 (n - 1) = 15998
    Case("LDS limit 100x80 k=2", _grid(100, 80), 2, all_ok, pct=0.01, n_plans=2),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
