"""The ReCom case table shared by test_recom_cases.py (CPU: the oracle reaches the branch each
case is for, and its steps are ReCom moves by the definition) and test_recom_edges_gpu.py (the
device equals the oracle on every chain of every case).

A case fixes the graph, the start plans and bounds dealt round-robin to the chains, the
proposal's parameters and the launch geometry, and states the coverage condition its oracle
trace must meet: ``chain_ok`` for every chain on its own, ``run_ok`` for all chains together.
A condition that fails means the case is wrong (change the case, never the condition).
"""
import dataclasses
import functools
from typing import Callable, Optional, Sequence, Tuple

import networkx as nx
import numpy as np

from flipcomplexityempirical_amd import graphs as G
from oracle.flipref import recom_run

SEED = 99
TRACE_FIELDS = ("draw", "edge", "root", "child", "attempts", "flags", "cut")


# ---- graphs -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(nx_, ny):
    return G.grid_graph(nx_, ny)


@functools.lru_cache(maxsize=None)
def path(n):
    return G.from_networkx(nx.path_graph(n), pos={i: (float(i), 0.0) for i in range(n)})


@functools.lru_cache(maxsize=None)
def cycle(n):
    t = 2 * np.pi / n
    return G.from_networkx(nx.cycle_graph(n), pos={i: (float(np.cos(i * t)), float(np.sin(i * t))) for i in range(n)})


@functools.lru_cache(maxsize=None)
def weighted_grid():
    """9 x 7 grid, populations 1-59 with every tenth node 10^5-10^6."""
    spec = G.grid_graph(9, 7)
    rng = np.random.default_rng(5)
    pop = rng.integers(1, 60, spec.n)
    pop[::10] = rng.integers(10 ** 5, 10 ** 6 + 1, len(pop[::10]))
    return dataclasses.replace(spec, pop=pop.astype(np.int32))


@functools.lru_cache(maxsize=None)
def heavy_grid():
    """4 x 4 grid of 2^27 - 1 per node: total 2^31 - 16, the largest totals a ReCom run takes."""
    spec = G.grid_graph(4, 4)
    return dataclasses.replace(spec, pop=np.full(spec.n, 2 ** 27 - 1, dtype=np.int32))


def overweight_grid():
    """4 x 4 grid of 2^28 per node: total 2^32, more than a ReCom run takes."""
    spec = G.grid_graph(4, 4)
    return dataclasses.replace(spec, pop=np.full(spec.n, 2 ** 28, dtype=np.int32))


def create_run(spec, k=2):
    """``fc_run_create`` of a two-chain ReCom run from k strips with the widest bounds (its
    checks of the graph come before anything touches a device)."""
    from flipcomplexityempirical_amd import _lib
    from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
    total = int(spec.pop.astype(np.int64).sum())
    cfg = RunConfig(k=k, labels=tuple(range(k)), proposal=_lib.FC_PROPOSE_RECOM, seed=SEED, pop_lo=0, pop_hi=2 ** 62,
                    recom_pop_target=total / k, recom_epsilon=0.3, diag_mask=0)
    return FlipRun(FlipGraph(spec), np.stack(strips(spec, k) * 2), cfg)


@functools.lru_cache(maxsize=None)
def delaunay200():
    return G.delaunay_graph(200, seed=3)


# ---- start plans (district ids 0..k-1 in canonical node order) ------------------------------
def strips(spec, k):
    return [spec.assignment_array(G.strip_plan(spec, k), range(k))]


def bisect(spec, k):
    return [spec.assignment_array(G.bisection_plan(spec, k), range(k))]


def halves(spec, k):
    """Node ids cut into k runs (paths and cycles)."""
    return [(np.arange(spec.n) * k // spec.n).astype(np.int8)]


def both_strips(spec, k):
    """Strips along x and strips along y, alternating over the chains."""
    turned = dataclasses.replace(spec, pos=spec.pos[:, ::-1].copy())
    return strips(spec, k) + strips(turned, k)


# ---- coverage conditions ----------------------------------------------------------------
def all_steps(case, ref):
    s = ref["stats"]
    return s["steps"] == case.steps and s["stuck"] == 0


def some_flag(flag):
    def ok(case, ref):
        return all_steps(case, ref) and bool(np.any(ref["trace"]["flags"] == flag))
    return ok


def end_root(case, ref):
    n = case.spec.n
    return all_steps(case, ref) and bool(np.any(np.isin(ref["trace"]["root"], (1, n - 2))))


def re_rooted(case, ref):
    s = ref["stats"]
    return (all_steps(case, ref) and s["attempts"] > s["trees"] > s["proposals"]
            and bool(np.any(ref["trace"]["attempts"] > case.node_repeats)))


def re_drawn(case, ref):
    return all_steps(case, ref) and ref["stats"]["inv_pop"] > 0


def stuck_midway(case, ref):
    s = ref["stats"]
    return s["stuck"] == 1 and 0 < s["steps"] < case.steps


def no_cut(case, ref):
    s = ref["stats"]
    return (s["stuck"] == 1 and s["steps"] == 0 and s["attempts"] == 7 and s["trees"] == 4 and s["proposals"] == 1
            and len(ref["trace"]) == 0)


def draw_capped(case, ref):
    s = ref["stats"]
    return s["stuck"] == 1 and s["proposals"] == 50 and 0 < s["steps"] < 60


def accept_and_reject(case, ref):
    f = ref["trace"]["flags"]
    return all_steps(case, ref) and bool(np.any(f == 3)) and bool(np.any(f == 1))


def more_attempts(case, ref):
    s = ref["stats"]
    return all_steps(case, ref) and s["attempts"] > s["proposals"]


def past_cap(case, ref):
    return all_steps(case, ref) and ref["stats"]["proposals"] > case.trace_cap


def bounds_matter(case, refs):
    """The two bound sets give different ``inv_pop`` totals, under each start plan on its own.
    The sets do not hold the same number of chains (37 chains), so the totals are compared per
    chain: total_a * chains_b != total_b * chains_a.  Plans are dealt with period 2 and bounds
    with period 4, so every (plan, bounds) pair occurs and the bounds' effect is not the plan's."""
    sets = sorted(set(case.bounds()))
    assert len(sets) == 2
    for plan in range(case.n_plans):
        tot, cnt = [0, 0], [0, 0]
        for c, r in enumerate(refs):
            if c % case.n_plans == plan:
                b = sets.index(case.chain_bounds(c))
                tot[b] += r["stats"]["inv_pop"]
                cnt[b] += 1
        if not (cnt[0] and cnt[1] and tot[0] * cnt[1] != tot[1] * cnt[0]):
            return False
    return True


_PLANS = {}  # case name -> its start plans


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    graph: Callable                 # () -> GraphSpec
    k: int
    plans: Callable                 # (spec, k) -> [assignment], dealt round-robin to the chains
    epsilon: float
    pct: Sequence[float]            # population bounds within pct of ideal, dealt round-robin ...
    chain_ok: Callable              # (case, oracle result of one chain) -> bool
    steps: int = 40
    lohi: Optional[Tuple[int, int]] = None  # ... or one explicit inclusive pair
    node_repeats: int = 1
    max_attempts: int = 10000
    base: float = 1.0
    max_draws: int = 0              # > 0: one launch (the device cap is per launch, the oracle's per run)
    n_chains: int = 5               # one full 4-wave block and a partial one at small n
    chain_id_offset: int = 0
    trace_chains: Optional[int] = None  # default: every chain
    trace_cap: int = 0              # default: room for every record
    run_ok: Optional[Callable] = None   # (case, [oracle result per chain]) -> bool
    kernel: str = "fc::recom_kernel<8>"
    walk: bool = True               # step-by-step validity on the CPU (graphs of <= 256 nodes)

    @property
    def spec(self):
        return self.graph()

    @property
    def pop_target(self):
        return int(self.spec.pop.astype(np.int64).sum()) / self.k

    def bounds(self):
        if self.lohi is not None:
            return [tuple(self.lohi)]
        total = int(self.spec.pop.astype(np.int64).sum())
        return [G.population_bounds(total, self.k, p)[1] for p in self.pct]

    def _all_plans(self):
        if self.name not in _PLANS:
            _PLANS[self.name] = self.plans(self.spec, self.k)
        return _PLANS[self.name]

    @property
    def n_plans(self):
        return len(self._all_plans())

    def plan(self, c):
        pl = self._all_plans()
        return pl[c % len(pl)]

    def chain_bounds(self, c):
        b = self.bounds()
        return b[c % len(b)]

    @property
    def n_traced(self):
        return self.n_chains if self.trace_chains is None else self.trace_chains

    @property
    def room(self):
        """Records the oracle may keep (and the device, unless the case sets its own cap)."""
        return 64 * self.steps + 64

    def oracle(self, c, n_steps=None):
        """The oracle's run of chain c (its own plan, bounds and chain id)."""
        lo, hi = self.chain_bounds(c)
        return recom_run(self.spec, self.plan(c), k=self.k, pop_target=self.pop_target, epsilon=self.epsilon,
                         pop_lo=lo, pop_hi=hi, seed=SEED, chain_id=self.chain_id_offset + c,
                         n_steps=self.steps if n_steps is None else n_steps, node_repeats=self.node_repeats,
                         base=self.base, max_attempts=self.max_attempts, max_draws=self.max_draws,
                         trace_cap=self.room)


def _sizes():
    out = []
    for (gx, gy), k, eps, pct in (((2, 2), 2, 0.3, 0.5), ((3, 1), 2, 0.4, 0.5), ((3, 4), 2, 0.2, 0.2),
                                  ((3, 4), 3, 0.3, 0.3), ((4, 4), 3, 0.3, 0.3), ((7, 9), 3, 0.1, 0.1),
                                  ((8, 8), 4, 0.2, 0.2), ((13, 5), 4, 0.2, 0.2), ((16, 16), 4, 0.1, 0.1)):
        out.append(Case(f"size {gx}x{gy} k={k}", functools.partial(grid, gx, gy), k, strips, eps, (pct,), all_steps))
    return out


CASES = _sizes() + [
    # |M| = n = npad and trees of maximal depth: the BFS has npad - 1 levels when the root is next to an end
    Case("path P16", functools.partial(path, 16), 2, halves, 0.3, (0.4,), end_root, steps=60),
    Case("cycle C16", functools.partial(cycle, 16), 2, halves, 0.3, (0.4,), all_steps),
    Case("cycle C32", functools.partial(cycle, 32), 2, halves, 0.2, (0.3,), all_steps),
    # a second root on the same tree, then new trees
    Case("re-root 8x8 k=2", functools.partial(grid, 8, 8), 2, strips, 0.03, (0.1,), re_rooted, node_repeats=2, base=1.2),
    Case("re-root 7x9 k=3", functools.partial(grid, 7, 9), 3, strips, 0.02, (0.1,), re_rooted, node_repeats=3, base=1.2),
    Case("re-root 16x16 k=4", functools.partial(grid, 16, 16), 4, strips, 0.01, (0.1,), re_rooted, node_repeats=2,
         base=1.2),
    # epsilon * target = 4 exactly: a subtree of 28 or 36 is no cut (<, not <=)
    Case("strict bound 8x8 k=2", functools.partial(grid, 8, 8), 2, strips, 0.125, (0.2,), all_steps),
    # the Validator re-draw
    Case("re-draw 8x8 k=4", functools.partial(grid, 8, 8), 4, strips, 0.4, (0.1,), re_drawn),
    Case("re-draw 16x16 k=4", functools.partial(grid, 16, 16), 4, strips, 0.4, (0.1,), re_drawn),
    Case("reject 8x8 k=4", functools.partial(grid, 8, 8), 4, strips, 0.2, (0.2,), some_flag(1), base=2.0),
    # two-node strips drift to 1 + 1 pairs, whose tree has no inner node: stuck by max_attempts
    Case("no inner node 4x2 k=4", functools.partial(grid, 4, 2), 4, strips, 0.6, (), stuck_midway, lohi=(1, 8),
         max_attempts=20, steps=60),
    Case("no cut 8x8 k=2", functools.partial(grid, 8, 8), 2, strips, 0.0, (0.1,), no_cut, node_repeats=2,
         max_attempts=7),
    Case("draw cap 8x8 k=2", functools.partial(grid, 8, 8), 2, strips, 0.4, (0.1,), draw_capped, steps=60,
         max_draws=50),
    Case("k=32 16x16", functools.partial(grid, 16, 16), 32, strips, 0.3, (), all_steps, lohi=(4, 12)),
    Case("weights 9x7 k=2", weighted_grid, 2, bisect, 0.3, (0.35,), accept_and_reject, base=1.5),
    Case("weights 9x7 k=3", weighted_grid, 3, bisect, 0.3, (0.35,), accept_and_reject, base=1.5),
    Case("weights delaunay200 k=3", delaunay200, 3, bisect, 0.1, (0.2,), all_steps, kernel="fc::recom_kernel<16>"),
    Case("top of range 4x4 k=2", heavy_grid, 2, strips, 0.3, (0.4,), all_steps),
    # ten blocks of which the last holds one chain; chain ids from 1000; per-chain plans (alternating
    # chain by chain) and bounds (alternating pair by pair, so that each plan runs under both)
    Case("many blocks 8x8 k=2", functools.partial(grid, 8, 8), 2, both_strips, 0.4, (0.1, 0.1, 0.3, 0.3), all_steps,
         n_chains=37, chain_id_offset=1000, trace_chains=5, run_ok=bounds_matter),
    # one wave per block, tree offsets up to 2 (n - 1) = 15998
    Case("LDS limit 100x80 k=2", functools.partial(grid, 100, 80), 2, strips, 0.01, (0.05,), more_attempts, steps=6,
         n_chains=2, walk=False),
    Case("trace cap 8x8 k=4", functools.partial(grid, 8, 8), 4, strips, 0.4, (0.1,), past_cap, trace_cap=30),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
