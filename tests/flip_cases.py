"""The flip-kernel case table shared by test_flip_cases.py (CPU: the oracle's trace of every case
reaches the branch the case is for) and test_flip_edges_gpu.py (the device equals the oracle on
every chain of every case, under every commit path and launch shape).

A case fixes the graph and k, the start plans, population bounds and bases dealt round-robin to
the chains, the seed, the steps and how they split into launches, the draw cap, and states the
coverage condition its oracle run must meet: ``chain_ok`` for every chain on its own, ``run_ok``
for all chains together.  A condition that fails means the case is wrong (change the case, never
the condition).

Two conditions replay the oracle's trace in plain numpy: :func:`pop_verdict_flips` (a population
verdict that changes under an acceptance less than 64 proposals before it: what closes a segment
of flip2_kernel's segment-parallel commit early) and :func:`outer_face_moves` (a district losing
its last node on the outer face, and regaining one: what changes the sign tests on the kernel's
outer-face counts).  The outer-face node set is the built graph's own: the gamma flag (meta bit
9) of ``FlipGraph.rings()``, host data read without a device.
"""
import dataclasses
import functools
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from flipcomplexityempirical_amd import graphs as G
from oracle import flipref
from oracle.flipref import FLAG_ACCEPTED, FLAG_INV_CONTIG, FLAG_INV_POP, FLAG_VALID, STREAM_BAND, STREAM_NODE
from recom_cases import both_strips, bisect, cycle, grid, halves, heavy_grid, path, strips, weighted_grid

SEED = 77
TRACE_FIELDS = ("draw", "v", "flags", "cut", "nb", "wait")
STAT_KEYS = ("steps", "proposals", "draws", "accepted", "inv_contig", "inv_pop", "sum_cut", "sum_nb", "sum_wait",
             "cut", "nb", "stuck", "wait_cur")
WINDOW = 64  # slots of one batch of the flip kernels


# ---- graphs (further ones: recom_cases) -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_weights_grid():
    """9 x 7 grid, populations 1-59: bounds a few nodes wide bind on every other proposal."""
    spec = G.grid_graph(9, 7)
    pop = np.random.default_rng(5).integers(1, 60, spec.n)
    return dataclasses.replace(spec, pop=pop.astype(np.int32))


@functools.lru_cache(maxsize=None)
def gamma_nodes(graph):
    """Outer-face flags [n] (bool) of ``graph()`` as the native graph builder sets them."""
    from flipcomplexityempirical_amd.engine import FlipGraph
    fg = FlipGraph(graph())
    _, meta = fg.rings()
    fg.close()
    return ((meta >> np.uint64(9)) & np.uint64(1)).astype(bool)


# ---- population bounds (one inclusive pair per entry, dealt round-robin) ----------------------
def pct_bounds(*pcts):
    def f(case):
        total = int(case.spec.pop.astype(np.int64).sum())
        return [G.population_bounds(total, case.k, p)[1] for p in pcts]
    return f


def fixed_bounds(*pairs):
    return lambda case: [tuple(p) for p in pairs]


def around_start(slack):
    """One pair per start plan (the same period as the plans, so chain c's bounds are its own
    plan's): the plan's smallest district population - slack .. its largest + slack."""
    def f(case):
        out = []
        for pl in case.all_plans():
            pops = np.bincount(pl, weights=case.spec.pop, minlength=case.k).astype(np.int64)
            out.append((int(pops.min()) - slack, int(pops.max()) + slack))
        return out
    return f


# ---- replay of an oracle trace in numpy ------------------------------------------------------
def replay(pop, k, init, trace):
    """Per proposal j of ``trace``: the district of its node before it (``A``), its target
    (``T``), the district populations before it (``pops`` [P, k]); and the assignments at every
    yield's start (``states`` [accepted + 1, n], one per accepted flip after the initial one)."""
    a = np.asarray(init, dtype=np.int8).copy()
    pops = np.bincount(a, weights=pop, minlength=k).astype(np.int64)
    P = len(trace)
    A = np.zeros(P, dtype=np.int64)
    T = (trace["flags"].astype(np.int64) >> 8) & 0xff
    before = np.zeros((P, k), dtype=np.int64)
    states = [a.copy()]
    for j in range(P):
        v = int(trace["v"][j])
        A[j] = a[v]
        before[j] = pops
        if trace["flags"][j] & FLAG_ACCEPTED:
            pops[A[j]] -= pop[v]
            pops[T[j]] += pop[v]
            a[v] = T[j]
            states.append(a.copy())
    return {"A": A, "T": T, "pops": before, "states": np.stack(states)}


def pop_verdict_flips(pop, k, init, trace, lo, hi, window=WINDOW):
    """Proposals j, valid or flagged FLAG_INV_POP, whose population verdict is the opposite when
    taken against the populations before an accepted proposal i with j - window < i < j."""
    pop = np.asarray(pop, dtype=np.int64)
    r = replay(pop, k, init, trace)
    P = len(trace)
    flags = trace["flags"].astype(np.int64)
    judged = (flags & (FLAG_VALID | FLAG_INV_POP)) != 0
    actual = (flags & FLAG_VALID) != 0
    accepted = (flags & FLAG_ACCEPTED) != 0
    pv = pop[trace["v"]]
    j = np.arange(P)
    flipped = np.zeros(P, dtype=bool)
    for d in range(1, window):
        i = j - d
        ok = (i >= 0) & judged
        ok[ok] &= accepted[i[ok]]
        q = r["pops"][np.maximum(i, 0)].copy()
        q[j, r["A"]] -= pv
        q[j, r["T"]] += pv
        verdict = ((q >= lo) & (q <= hi)).all(axis=1)
        flipped |= ok & (verdict != actual)
    return int(flipped.sum())


def outer_face_moves(gamma, k, init, trace):
    """(leaves, regains): accepted flips after which the flipped node's old district has no node
    on the outer face any more, and those that give a district without one its first."""
    a = np.asarray(init, dtype=np.int8).copy()
    ng = np.bincount(a[gamma], minlength=k)
    leaves = regains = 0
    for rec in trace[(trace["flags"] & FLAG_ACCEPTED) != 0]:
        v, t = int(rec["v"]), (int(rec["flags"]) >> 8) & 0xff
        if gamma[v]:
            ng[a[v]] -= 1
            leaves += ng[a[v]] == 0
            regains += ng[t] == 0
            ng[t] += 1
        a[v] = t
    return int(leaves), int(regains)


def boundary_nodes(spec, state):
    e = spec.edges()
    cut = state[e[:, 0]] != state[e[:, 1]]
    out = np.zeros(spec.n, dtype=bool)
    out[e[cut, 0]] = True
    out[e[cut, 1]] = True
    return out


# ---- coverage conditions: (case, chain, oracle result) -> bool ---------------------------------
def share(ref, key):
    return ref["stats"][key] / max(1, ref["stats"]["proposals"])


def all_steps(case, c, ref):
    s = ref["stats"]
    return s["steps"] == case.steps and s["stuck"] == 0 and 0 < s["draws"] < case.max_draws


def both_invalid_kinds(case, c, ref):
    return all_steps(case, c, ref) and share(ref, "inv_pop") >= 0.1 and share(ref, "inv_contig") >= 0.1


def verdict_flips(times):
    def ok(case, c, ref):
        lo, hi = case.chain_bounds(c)
        return all_steps(case, c, ref) and pop_verdict_flips(case.spec.pop, case.k, case.plan(c), ref["trace"],
                                                             lo, hi) >= times
    return ok


def every_node_on_boundary(case, c, ref):
    r = replay(case.spec.pop.astype(np.int64), case.k, case.plan(c), ref["trace"])
    seen = np.zeros(case.spec.n, dtype=bool)
    for st in r["states"]:
        seen |= boundary_nodes(case.spec, st)
    return all_steps(case, c, ref) and bool(seen.all())


def some_inv_pop(case, c, ref):
    return all_steps(case, c, ref) and ref["stats"]["inv_pop"] > 0


def cannot_move(case, c, ref):
    s = ref["stats"]
    return (s["stuck"] == 1 and s["steps"] == 0 and s["accepted"] == 0 and s["draws"] == case.max_draws
            and s["proposals"] == s["inv_contig"] > 0)


def always_accepts(case, c, ref):
    s = ref["stats"]
    return all_steps(case, c, ref) and s["accepted"] == s["steps"]


def inv_pop_share(least):
    def ok(case, c, ref):
        return all_steps(case, c, ref) and share(ref, "inv_pop") >= least
    return ok


def last_node_refused(case, c, ref):
    """Some district is down to one node and a proposal to flip that node is refused (by the
    contiguity rule: the node has no neighbour left in its district); no district is ever empty."""
    r = replay(case.spec.pop.astype(np.int64), case.k, case.plan(c), ref["trace"])
    if not all_steps(case, c, ref) or (r["pops"] <= 0).any():
        return False
    flags = ref["trace"]["flags"]
    sizes = r["pops"][np.arange(len(flags)), r["A"]]  # unit populations: a district's size
    return bool(np.any((sizes == 1) & ((flags & FLAG_INV_CONTIG) != 0))) and not np.any((sizes == 1) & ((flags & FLAG_VALID) != 0))


# ---- conditions on all chains of a run: (case, [oracle result per chain]) -> bool ---------------
def leaves_at_low_bases(case, refs):
    """Every chain whose base is at most 1 sees a district leave the outer face and return to it
    (a base above 1 keeps the districts compact: those chains are in the case for the verdicts
    that do not change)."""
    moves = [outer_face_moves(gamma_nodes(case.graph), case.k, case.plan(c), r["trace"]) for c, r in enumerate(refs)]
    return all(min(m) >= 1 for c, m in enumerate(moves) if case.base(c) <= 1.0)


def leaves_in_run(times):
    def ok(case, refs):
        moves = [outer_face_moves(gamma_nodes(case.graph), case.k, case.plan(c), r["trace"])
                 for c, r in enumerate(refs)]
        return sum(m[0] for m in moves) >= times and sum(m[1] for m in moves) >= 1
    return ok


def some_chain_rejects(case, refs):
    return any(r["stats"]["accepted"] < r["stats"]["steps"] for r in refs)


_PLANS = {}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    graph: Callable                  # () -> GraphSpec
    k: int
    plans: Callable                  # (spec, k) -> [assignment], dealt round-robin to the chains
    bounds: Callable                 # (case) -> [(pop_lo, pop_hi)], dealt round-robin
    chain_ok: Callable               # (case, chain, oracle result of that chain) -> bool
    bases: Sequence[float] = (1.0,)  # dealt round-robin
    steps: int = 3000
    launches: Sequence[int] = (1000,)  # steps of the first launches; the rest goes in a last one
    max_draws: int = 2000000         # per launch on the device, per run in the oracle: never reached
                                     # by a case that takes all its steps
    n_chains: int = 8
    seed: int = SEED
    run_ok: Optional[Callable] = None  # (case, [oracle result per chain]) -> bool
    pair: bool = False               # FC_PROPOSE_PAIR (k > 2 kernel) instead of BI_SIGN
    use_positions: bool = True
    band: bool = False               # k = 2: also run under the band stream
    trace_cap: int = 16384

    @property
    def spec(self):
        return self.graph()

    @property
    def labels(self):
        return (-1, 1) if self.k == 2 and not self.pair else tuple(range(self.k))

    def all_plans(self):
        if self.name not in _PLANS:
            _PLANS[self.name] = self.plans(self.spec, self.k)
        return _PLANS[self.name]

    def plan(self, c):
        pl = self.all_plans()
        return pl[c % len(pl)]

    def chain_bounds(self, c) -> Tuple[int, int]:
        b = self.bounds(self)
        return b[c % len(b)]

    def base(self, c):
        return float(self.bases[c % len(self.bases)])

    def launch_steps(self):
        first = [int(x) for x in self.launches if x > 0]
        first = first if sum(first) < self.steps else []
        return first + [self.steps - sum(first)]

    def oracle(self, c, stream=STREAM_NODE):
        """The oracle's run of chain c with every output (cached: the CPU and the device tests and
        every device variant share one run)."""
        return _oracle(self.name, c, stream)


@functools.lru_cache(maxsize=None)
def _cref():
    flipref.build_lib()
    return flipref.CRef()


@functools.lru_cache(maxsize=None)
def _oracle(name, c, stream):
    case = BY_NAME[name]
    spec = case.spec
    lo, hi = case.chain_bounds(c)
    ref = _cref().run(spec, case.plan(c), base=case.base(c), pop_lo=lo, pop_hi=hi, seed=case.seed, chain_id=c,
                      n_steps=case.steps, k=case.k, labels=list(case.labels), log1mp=G.log1mp_table(spec.n, case.k),
                      max_draws=case.max_draws, trace_cap=case.trace_cap, want_hist=True, want_edges=True,
                      want_flips=True, proposal=int(case.pair), stream=stream)
    for arr in ref.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return ref


def _lines():
    out = []
    for n in (3, 5, 17):
        cond = every_node_on_boundary if n <= 5 else all_steps
        out.append(Case(f"path{n}", functools.partial(path, n), 2, halves, pct_bounds(0.9), cond, bases=(1.0, 0.5, 2.0),
                        band=n == 17))
        out.append(Case(f"cycle{n}", functools.partial(cycle, n), 2, halves, pct_bounds(0.9), cond,
                        bases=(1.0, 0.5, 2.0), band=n == 17))
    for n in (64, 65):  # words == 1 full, and the first node of a second word
        out.append(Case(f"path{n}", functools.partial(path, n), 2, halves, pct_bounds(0.9), some_inv_pop,
                        bases=(1.0, 0.7)))
        out.append(Case(f"cycle{n}", functools.partial(cycle, n), 2, halves, pct_bounds(0.9), some_inv_pop,
                        bases=(1.0, 0.7)))
    return out


K2_CASES = [
    # every node a boundary node: every draw is a hit, the 64th closes every window
    Case("grid3x3", functools.partial(grid, 3, 3), 2, both_strips, pct_bounds(0.5), both_invalid_kinds,
         bases=(1.0, 0.5, 3.0)),
    # npad == n == 16; a district of the four inner nodes has left the outer face
    Case("grid4x4", functools.partial(grid, 4, 4), 2, both_strips, pct_bounds(0.5), all_steps,
         bases=(0.5, 1.0, 3.0), n_chains=12, band=True, run_ok=leaves_at_low_bases),
    Case("grid4x4_heavy", heavy_grid, 2, both_strips, pct_bounds(0.5), all_steps, bases=(0.5, 1.0, 3.0),
         n_chains=12, run_ok=leaves_at_low_bases),
    Case("grid9x7", functools.partial(grid, 9, 7), 2, both_strips, pct_bounds(0.5), all_steps,
         run_ok=leaves_in_run(3)),
    # weighted populations in the segment commit's prefix scan, bounds about two median nodes wide
    Case("grid9x7_weighted", small_weights_grid, 2, both_strips, around_start(40), verdict_flips(5),
         bases=(1.0, 0.7, 1.5), n_chains=12, band=True),
    Case("grid8x8", functools.partial(grid, 8, 8), 2, both_strips, pct_bounds(0.5), all_steps, bases=(1.0, 0.5, 3.0)),
] + _lines() + [
    # a chain that cannot move: one launch, ended by the draw cap inside a batch window
    Case("path2", functools.partial(path, 2), 2, halves, fixed_bounds((0, 2)), cannot_move, steps=100, launches=(),
         max_draws=4099),
    # the launch's last step among accepted slots of a segment
    Case("all_accept", functools.partial(cycle, 17), 2, halves, pct_bounds(0.9), always_accepts,
         launches=(1, 2, 63, 64, 65)),
]

PAIR_CASES = [
    Case("pair 6x5 k=3 tight", functools.partial(grid, 6, 5), 3, strips, fixed_bounds((6, 14)), inv_pop_share(0.05),
         bases=(1.0, 0.5, 2.0), pair=True),
    # (N^k = 2^48: waits around 10^12, whose ceiling turns on the last bit of log(1 - U); chain 1's
    # proposal 3155 is the draw the device's own log got one short: DESIGN.md "Large waits")
    Case("pair 8x8 k=8 lo=1", functools.partial(grid, 8, 8), 8, strips, fixed_bounds((1, 64)), last_node_refused,
         bases=(1.0, 0.5), pair=True),
    Case("pair 8x8 k=8 lo=0", functools.partial(grid, 8, 8), 8, strips, fixed_bounds((0, 64)), last_node_refused,
         bases=(1.0, 0.5), pair=True),
    Case("pair weights 9x7 k=3", weighted_grid, 3, bisect, pct_bounds(0.35), some_inv_pop, bases=(1.5, 1.0, 0.5),
         pair=True, run_ok=some_chain_rejects),
    # the district-graph rule (planar rings) and, without positions, the device search
    Case("pair 8x8 k=4 dgraph", functools.partial(grid, 8, 8), 4, strips, pct_bounds(0.5), some_inv_pop,
         bases=(1.0, 0.5, 2.0), pair=True),
    Case("pair 8x8 k=4 search", functools.partial(grid, 8, 8), 4, strips, pct_bounds(0.5), some_inv_pop,
         bases=(1.0, 0.5, 2.0), pair=True, use_positions=False),
]

CASES = K2_CASES + PAIR_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
