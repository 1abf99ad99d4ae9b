"""The series-kernel case table shared by test_series_cases.py (CPU: the oracle's run of every case
reaches the branch the case is for) and test_series_edges_gpu.py (the device equals the reference
of ``series_model`` on every chain of every case).

A case fixes the graph, the start plans, bounds and bases dealt round-robin to the chains, the
steps before the series window opens (``pre``: ``series_reset()`` after that many; None: the
window is the run's own, from yield 0), the cumulative window steps at which everything is read
(``reads``; each stretch between two reads is one launch, or ``split`` launches), the frames read,
and the coverage condition ``run_ok`` its oracle run must meet.  A condition that fails means the
case is wrong (change the case, never the condition).

The events are the C oracle's (``CRef.run`` and ``events_from_trace``, as ``flip_cases``); the
expected values are ``series_model``'s and ``oracle.flipref.acf_exact``'s.
"""
import dataclasses
import functools
import math
from typing import Callable, Optional, Sequence

import numpy as np

import series_model as M
from flip_cases import _cref
from flipcomplexityempirical_amd import graphs as G
from oracle.flipref import events_from_trace
from recom_cases import both_strips, cycle, grid, halves

SEED = 77
LAG_MAX = 2 ** 31 - 1
LADDER = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1500)
LAG_T = (1, 2, 4095, 4096, 4097, 8192, 8193)
PREFIX_F = (0, 1, 2, 64, 65, 128, 129, 192, 193, 255, 256)


def lags_for(T):
    """The lags read on a window of T yields: around 0, the 4096-yield tile and the window's end,
    and the largest a lag can be."""
    return sorted({L for L in (0, 1, 2, 4095, 4096, 4097, T - 1, T, T + 1, LAG_MAX) if L >= 0})


# ---- start plans ----------------------------------------------------------------------------
def arc(n, j0, j1):
    """District 1 is the arc of nodes j0 + 1 .. j1 of the n-cycle (mod n): ring edges j0 and j1 cut."""
    a = np.zeros(n, dtype=np.int8)
    a[(j0 + 1 + np.arange((j1 - j0) % n)) % n] = 1
    return a


def word_pair_arcs(spec, k=2):
    """Ten arcs of the 256-cycle whose two cut ring edges lie in 64-edge words (w0, w1), every
    w0 <= w1 once."""
    return [arc(spec.n, 64 * w0 + 10, 64 * w1 + 40) for w0 in range(4) for w1 in range(w0, 4)]


def prefix_arcs(F):
    """Arcs of the 256-cycle about the end of the frame of its first F ring edges: the last frame
    edge F - 1 cut with one 20 edges before it; edge F - 2 cut with one 40 before it; and an arc
    with one cut edge inside the frame and one outside, where the frame leaves an edge outside.
    (Both of F - 2 and F - 1 cut at once would be a one-node district, outside any bounds; every
    chain's cut edges walk a step at a time, so they pass over F - 2, F - 1 and F.)"""
    def f(spec, k=2):
        n = spec.n
        out = [arc(n, (F - 21) % n, (F - 1) % n), arc(n, (F - 42) % n, (F - 2) % n)]
        if F + 28 < n:
            out.append(arc(n, (F - 2) % n, F + 28))
        elif F < n:
            out.append(arc(n, F - 31, n - 1))
        return out
    return f


# ---- frames -----------------------------------------------------------------------------------
def ring_frame(spec, idx, mid=None, centre=(0.0, 0.0)):
    """Frame edge i is ring edge (idx[i], idx[i] + 1 mod n) of a cycle, with its midpoint."""
    idx = np.asarray(list(idx), dtype=np.int32)
    eu, ev = idx, ((idx + 1) % spec.n).astype(np.int32)
    if mid is None:
        mid = (spec.pos[eu] + spec.pos[ev]) / 2 if idx.size else np.zeros((0, 2))
    return G.SlopeFrame(eu=eu, ev=ev, mid=np.asarray(mid, dtype=np.float64).reshape(-1, 2), center=tuple(centre))


def edge_frame(spec, edges, centre):
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return G.SlopeFrame(eu=e[:, 0].copy(), ev=e[:, 1].copy(), mid=(spec.pos[e[:, 0]] + spec.pos[e[:, 1]]) / 2,
                        center=tuple(centre))


def cycle65_frames(case):
    n = case.spec.n
    return {"full": ring_frame(case.spec, range(n)),
            "three quarters": ring_frame(case.spec, [i for i in range(n) if i % 4]),
            "even": ring_frame(case.spec, range(0, n, 2))}


def full_ring(case):
    return {"full": ring_frame(case.spec, range(case.spec.n))}


def prefix_frame(F):
    return lambda case: {"prefix": ring_frame(case.spec, range(F))}


VALUE_CENTRE = (1.0, 2.0)
# midpoints relative to the centre: the first cut edge's (frame edges 0-31, in turn) and the
# second's (32-64, in turn).  With a = (1, 1): equal x (+inf); equal y with bx < ax (-0.0) and
# bx > ax (0.0); the centre between the two (pi) and both on one ray from it (0); the centre itself
# (NaN angle, finite slope).  Neighbouring frame edges share (1, 1) and (-2, -2): other keys, the
# same values.
VALUE_A = ((1.0, 1.0), (1.0, 1.0), (-2.0, 3.0), (2.0, 0.0))
VALUE_B = ((1.0, -4.0), (-3.0, 1.0), (5.0, 1.0), (-2.0, -2.0), (-2.0, -2.0), (3.0, 3.0), (0.0, 0.0))


def value_frame(case):
    n = case.spec.n
    rel = [VALUE_A[i % len(VALUE_A)] if i < 32 else VALUE_B[(i - 32) % len(VALUE_B)] for i in range(n)]
    mid = np.asarray(rel) + np.asarray(VALUE_CENTRE)
    return {"values": ring_frame(case.spec, range(n), mid=mid, centre=VALUE_CENTRE)}


# (no lattice line passes through it: no two midpoints are collinear with the centre)
DENSE_CENTRE = (4 * math.sqrt(2.0), 1.8 * math.pi)


def dense_frames(case):
    e = case.spec.edges()
    perm = np.random.default_rng(SEED).permutation(len(e))
    return {"first 256": edge_frame(case.spec, e[:256], DENSE_CENTRE),
            "permuted 256": edge_frame(case.spec, e[perm[:256]], DENSE_CENTRE)}


GLOBAL_CENTRE = (59.5 + math.sqrt(0.5), 59.5 - 1 / math.pi)


def global_frame(case):
    """256 pairwise disjoint edges of the 120 x 120 grid: the 120 edges the x-strips' start plan
    cuts (x = 59 | 60), ordered from the middle row outwards, then edges two and four columns off."""
    ix = case.spec.index
    rows = sorted(range(120), key=lambda y: (abs(2 * y - 119), y))
    e = [(ix[(59, y)], ix[(60, y)]) for y in rows] + [(ix[(57, y)], ix[(58, y)]) for y in rows] + \
        [(ix[(61, y)], ix[(62, y)]) for y in rows[:16]]
    return {"disjoint 256": edge_frame(case.spec, e, GLOBAL_CENTRE)}


def x_strips(spec, k=2):
    return both_strips(spec, k)[:1]


def no_frames(case):
    return {}


# ---- coverage conditions: (case, [chain info]) -> bool; info: Case.info ---------------------------
def _profiles(infos, frame):
    return [M.queue_profile(i[frame]["key"]) for i in infos]


def events_equal_steps(case, infos):
    return all(len(i["events"]) == case.reads[-1] for i in infos)


def full_frame_queues(case, infos):
    """Every event a candidate: each chunk fills the queue exactly (rest 0), and at 1500 events
    waves 0-2 end on a flush, wave 3 with the 28 events of the last chunk."""
    ok = events_equal_steps(case, infos)
    for rests, tails in _profiles(infos, "full"):
        ok = ok and len(rests) == 23 and not any(rests) and tails == [0, 0, 0, 28]
    return ok


def sparse_frame_queues(case, infos, frames):
    """Frames that leave edges out (n_cut takes 0, 1 and 2, ``frames``: name -> the NaN share's
    range): on every chain and frame a 64-flush leaves a rest; over the run there are 64-flushes
    with and without a rest, and waves that end with and without a queue."""
    good = True
    rests, tails = [], []
    for frame, (nan_lo, nan_hi) in frames.items():
        for i, (r, t) in zip(infos, _profiles(infos, frame)):
            good = good and any(x > 0 for x in r) and {0, 1, 2} <= set(i[frame]["n_cut"].tolist())
            rests += r
            tails += t
        nan = np.mean(np.concatenate([np.isnan(i[frame]["slope"]) for i in infos]))
        good = good and nan_lo <= nan <= nan_hi
    return (good and any(x > 0 for x in rests) and any(x == 0 for x in rests) and any(x > 0 for x in tails)
            and any(x == 0 for x in tails))


def ladder(case, infos):
    """The reads of the 65-cycle: 0 to 5 chunks and 24, a last chunk of 1, 63 and 64 events, empty
    wave ranges; the three frames' queue conditions."""
    nk = {(s + 63) // 64 for s in case.reads}
    return (tuple(case.reads) == LADDER and {0, 1, 2, 3, 4, 5, 24} <= nk and {0, 1, 63} <= {s % 64 for s in case.reads}
            and full_frame_queues(case, infos)
            and sparse_frame_queues(case, infos, {"three quarters": (0.4, 0.6), "even": (0.65, 0.85)}))


def word_pairs(case, infos):
    pairs = {((int(i["full"]["key"][0]) & 0xffff) >> 6, int(i["full"]["key"][0]) >> 22) for i in infos}
    return events_equal_steps(case, infos) and pairs == {(a, b) for a in range(4) for b in range(a, 4)}


def prefix_edges(F):
    def ok(case, infos):
        if not events_equal_steps(case, infos):
            return False
        d = [i["prefix"] for i in infos]
        if F < 2:  # never two cut frame edges: NaN throughout, the window start the only change point
            return all(np.isnan(x["slope"]).all() and np.isnan(x["angle"]).all() and x["n_cut"].max() <= F and
                       len(i["changes"]["prefix"]["t"]) == 1 for x, i in zip(d, infos))
        cnt = np.concatenate([x["n_cut"] for x in d])
        if F < 256 and not np.any(cnt == 1):
            return False
        if F == 2:  # edges 0 and 1 cut at once: a one-node district
            return cnt.max() == 1 and all(np.isnan(x["slope"]).all() for x in d)
        second = {int(k) >> 16 for x in d for k in x["key"] if k != M.NO_KEY}
        return np.any(cnt == 2) and {F - 2, F - 1} <= second  # bit 62 / 63 of a word, or 63 / 0 of the next
    return ok


def special_values(case, infos):
    s = np.concatenate([i["values"]["slope"] for i in infos])
    a = np.concatenate([i["values"]["angle"] for i in infos])
    zero = s == 0.0
    spare = 0  # candidates that are no change points
    for i in infos:
        k = i["values"]["key"]
        spare += int((k[1:] != k[:-1]).sum()) + 1 - len(i["changes"]["values"]["t"])
    return (events_equal_steps(case, infos) and np.any(np.isposinf(s)) and np.any(zero & np.signbit(s)) and
            np.any(zero & ~np.signbit(s)) and np.any(a == math.pi) and np.any(a == 0.0) and
            np.any(np.isnan(a) & np.isfinite(s)) and spare >= 1)


def dense_masks(case, infos):
    ok = True
    for name, fr in case.frame_set().items():
        many = all4 = False
        for i in infos:
            many = many or i[name]["n_cut"].max() >= 3
            all4 = all4 or bool(np.any(i[name]["words"] == 15))
        ok = ok and many and all4
    return ok


def global_keys(case, infos):
    keys = set()
    for i in infos:
        keys |= set(i["disjoint 256"]["key"].tolist())
        if len(i["changes"]["disjoint 256"]["t"]) < 2:
            return False
    return len(keys) >= 5


def varying_cut(case, infos):
    """The |cut| series of the last window varies on every chain (windows of 64 yields or more: a
    window of one or two yields may well be constant)."""
    return case.reads[-1] < 64 or all(len(set(i["x"].tolist())) > 1 for i in infos)


def constant_cut(case, infos):
    return all(set(i["x"].tolist()) == {2} for i in infos)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    graph: Callable                  # () -> GraphSpec
    plans: Callable                  # (spec, k) -> [assignment], dealt round-robin to the chains
    frames: Callable                 # (case) -> {name: SlopeFrame}
    run_ok: Callable                 # (case, [Case.info per chain]) -> bool
    pct: float = 0.9
    bases: Sequence[float] = (1.0, 0.5, 2.0)
    reads: Sequence[int] = (1500,)   # cumulative window steps at which everything is read
    split: int = 1                   # launches per stretch between two reads
    pre: Optional[int] = None        # steps before series_reset() opens the window (None: no reset)
    n_chains: int = 8
    seed: int = SEED
    global_tables: bool = False      # the frame tables do not fit the LDS

    @property
    def spec(self):
        return self.graph()

    @property
    def steps(self):
        return (self.pre or 0) + self.reads[-1]

    @property
    def t0(self):
        return self.pre or 0

    def plan(self, c):
        pl = _plans(self.name)
        return pl[c % len(pl)]

    def base(self, c):
        return float(self.bases[c % len(self.bases)])

    def bounds(self):
        return G.population_bounds(int(self.spec.pop.astype(np.int64).sum()), 2, self.pct)[1]

    def frame_set(self):
        return _frames(self.name)

    def launches(self):
        """[(steps of each launch of the stretch, cumulative window steps at its read)]"""
        out, at = [], 0
        for s in self.reads:
            d = s - at
            parts = [d // self.split + (j < d % self.split) for j in range(self.split)]
            out.append(([p for p in parts if p > 0], s))
            at = s
        return out

    def oracle(self, c):
        return _oracle(self.name, c)

    def window(self, c, s):
        """Chain c's window read after s window steps: the start state ``a0`` with its |cut| ``x0``,
        the window's ``events`` (t, v, cut, nb, target) and its yields ``T``."""
        o = self.oracle(c)
        ev = o["events"]
        a0, x0 = _start(self.name, c)
        return {"a0": a0, "x0": x0, "t0": self.t0, "T": s + 1,
                "events": ev[(ev[:, 0] > self.t0) & (ev[:, 0] <= self.t0 + s)]}

    def info(self, c):
        """Chain c at the last read: the window, per frame the model's dense series (with
        ``words``, the 64-edge words holding a cut frame edge as a bit set, per entry) and its
        change points, and the per-yield |cut| list ``x``."""
        return _info(self.name, c)

    def dense(self, c, frame, s):
        """The model's dense series of chain c at the read after s window steps: a prefix of the
        last read's (the entries are per event)."""
        n = len(self.window(c, s)["events"]) + 1
        return {k: v[:n] for k, v in self.info(c)[frame].items()}


@functools.lru_cache(maxsize=None)
def _plans(name):
    case = BY_NAME[name]
    return case.plans(case.spec, 2)


@functools.lru_cache(maxsize=None)
def _frames(name):
    case = BY_NAME[name]
    return case.frames(case)


@functools.lru_cache(maxsize=None)
def _log1mp(n):
    return G.log1mp_table(n, 2)


@functools.lru_cache(maxsize=None)
def _oracle(name, c):
    case = BY_NAME[name]
    spec = case.spec
    lo, hi = case.bounds()
    cap = 8 * case.steps + 4096
    ref = _cref().run(spec, case.plan(c), base=case.base(c), pop_lo=lo, pop_hi=hi, seed=case.seed, chain_id=c,
                      n_steps=case.steps, k=2, labels=[-1, 1], log1mp=_log1mp(spec.n), max_draws=0, trace_cap=cap)
    assert ref["stats"]["steps"] == case.steps and len(ref["trace"]) == ref["stats"]["proposals"] < cap, (name, c)
    out = {"stats": ref["stats"], "final": ref["final"], "events": events_from_trace(ref["trace"])}
    for arr in out.values():
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _start(name, c):
    case = BY_NAME[name]
    a = np.array(case.plan(c), dtype=np.int8)
    for ev in case.oracle(c)["events"]:
        if ev[0] > case.t0:
            break
        a[ev[1]] = ev[4]
    e = case.spec.edges()
    a.setflags(write=False)
    return a, int((a[e[:, 0]] != a[e[:, 1]]).sum())


@functools.lru_cache(maxsize=None)
def _info(name, c):
    case = BY_NAME[name]
    w = case.window(c, case.reads[-1])
    out = dict(w)
    out["changes"] = {}
    for fname, fr in case.frame_set().items():
        d = M.frame_dense(w["a0"], w["events"], fr.eu, fr.ev, fr.mid, fr.center)
        d["words"] = _words(w["a0"], w["events"], fr)
        out[fname] = d
        out["changes"][fname] = M.frame_changes(d, w["t0"], w["events"][:, 0])
    out["x"] = M.cut_yields(w["x0"], w["events"], w["t0"], w["T"])
    return out


def _words(a0, events, fr):
    a = np.array(a0)
    out = np.zeros(len(events) + 1, dtype=np.int64)
    word = np.arange(len(fr.eu)) >> 6
    for i in range(len(events) + 1):
        if i:
            a[events[i - 1][1]] = events[i - 1][4]
        for q in set(word[a[fr.eu] != a[fr.ev]].tolist()):
            out[i] |= 1 << q
    return out


def _lag_cases():
    g97 = functools.partial(grid, 9, 7)
    out = []
    for T in LAG_T:
        for split in (1, 3):
            out.append(Case(f"lag T={T} launches={split}", g97, both_strips, no_frames, varying_cut, pct=0.5,
                            reads=(T - 1,), split=split, n_chains=4))
    # a window that starts mid-run, read with 1, 2 and 4097 yields
    out.append(Case("lag window after 1000", g97, both_strips, no_frames, varying_cut, pct=0.5, pre=1000,
                    reads=(0, 1, 4096), n_chains=4))
    out.append(Case("lag constant T=4097", functools.partial(cycle, 65), halves, no_frames, constant_cut,
                    reads=(1, 4096), n_chains=4))
    return out


CASES = [
    Case("cycle65 ladder", functools.partial(cycle, 65), halves, cycle65_frames, ladder, pre=0, reads=LADDER,
         n_chains=10),
    Case("cycle256 word pairs", functools.partial(cycle, 256), word_pair_arcs, full_ring, word_pairs, reads=(257,),
         n_chains=10),
] + [
    Case(f"cycle256 prefix F={F}", functools.partial(cycle, 256), prefix_arcs(F), prefix_frame(F), prefix_edges(F),
         reads=(257,), n_chains=6) for F in PREFIX_F
] + [
    Case("cycle65 values", functools.partial(cycle, 65), halves, value_frame, special_values, n_chains=10),
    Case("grid12x12 dense", functools.partial(grid, 12, 12), both_strips, dense_frames, dense_masks, pct=0.5,
         bases=(0.3, 1.0, 3.0, 0.6), reads=(1200,)),
    Case("grid120x120 global tables", functools.partial(grid, 120, 120), x_strips, global_frame, global_keys, pct=0.5,
         bases=(1.0, 0.5, 0.8, 0.3), reads=(1200,), global_tables=True),
] + _lag_cases()

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
