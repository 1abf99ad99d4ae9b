"""Host model of replica exchange (DESIGN.md "Replica exchange"): a helper, not a test.

Everything runs on the CPU.  Per round, every ladder chain advances by one oracle segment
(``cref.run`` from the chain's current state at the base of the rung it holds, on the canonical
stream replayed from the chain's draw counter: the oracle has no resume, a replay from a start draw
is how a segment is stated); then the swap rule is applied with ``fc_ladder_swap_threshold`` (the
one definition of the decision's bits) and the oracle's Philox.

A segment redraws its initial state's geometric wait, so ``sum_wait`` of a segment is not the
device's; the model leaves it out (tests/test_tempering_gpu.py checks it through equal bases).
"""
import numpy as np

from oracle import flipref

COUNTERS = ("steps", "proposals", "draws", "accepted", "inv_contig", "inv_pop")
SUMS = ("sum_cut", "sum_nb", "sum_cut2", "sum_nb2")
FIELDS = COUNTERS + SUMS


def mant53(a: int, b: int) -> int:
    return ((a >> 5) << 26) | (b >> 6)


class TemperingModel:
    def __init__(self, cref, spec, inits, bases, ladders, *, threshold, k=2, proposal=0, pop_lo, pop_hi,
                 seed, labels=(-1, 1), chain_id_offset=0, nb_pairs=False, want_hist=False):
        """``threshold(b_lo_rung, b_hi_rung, d) -> int`` is ``fc_ladder_swap_threshold``."""
        self.cref, self.spec, self.threshold = cref, spec, threshold
        self.k, self.proposal, self.pop_lo, self.pop_hi = k, proposal, pop_lo, pop_hi
        self.seed, self.labels, self.offset, self.nb_pairs = seed, list(labels), chain_id_offset, nb_pairs
        self.want_hist = want_hist
        self.C = int(np.asarray(inits).shape[0])
        self.assign = [np.array(a, dtype=np.int8) for a in inits]
        self.bases0 = np.asarray(bases, dtype=np.float64)
        self.ladders = [list(map(int, lad)) for lad in ladders]
        self.chain_at = [list(lad) for lad in self.ladders]            # per ladder, chain at each rung
        self.slot_bases = [[float(self.bases0[c]) for c in lad] for lad in self.ladders]
        self.rung_of = np.full(self.C, -1, dtype=np.int32)
        self.ladder_of = np.full(self.C, -1, dtype=np.int32)
        for l, lad in enumerate(self.ladders):
            for r, c in enumerate(lad):
                self.rung_of[c], self.ladder_of[c] = r, l
        self.round_no = 0
        self.decisions = []  # (round, ladder, rung, d, threshold, mant53, accepted)
        E, nbw = spec.n_edges, flipref.nb_width(spec, k, nb_pairs)
        # per chain: cumulative counters and sums as fc_chain_stats keeps them (sum_wait excepted)
        self.chain = [dict.fromkeys(FIELDS, 0) for _ in range(self.C)]
        self.rung = [[dict.fromkeys(FIELDS + ("swaps_tried", "swaps_accepted"), 0) for _ in lad] for lad in self.ladders]
        self.rung_cut_hist = [np.zeros((len(lad), E + 1), dtype=np.int64) for lad in self.ladders]
        self.rung_nb_hist = [np.zeros((len(lad), nbw), dtype=np.int64) for lad in self.ladders]
        for c in range(self.C):  # yield #0 enters every per-yield sum, for the initial rung
            st = self._segment(c, float(self.bases0[c]), 0)["stats"]
            ch = self.chain[c]
            ch.update(cut=st["cut"], nb=st["nb"], sum_cut=st["cut"], sum_nb=st["nb"], sum_cut2=st["cut"] ** 2,
                      sum_nb2=st["nb"] ** 2)
            if self.ladder_of[c] >= 0:
                l, r = self.ladder_of[c], self.rung_of[c]
                for f in SUMS:
                    self.rung[l][r][f] += ch[f]
                self.rung_cut_hist[l][r, st["cut"]] += 1
                self.rung_nb_hist[l][r, st["nb"]] += 1

    def base_now(self, c: int) -> float:
        l = self.ladder_of[c]
        return float(self.bases0[c]) if l < 0 else self.slot_bases[l][self.rung_of[c]]

    def bases_now(self) -> np.ndarray:
        return np.asarray([self.base_now(c) for c in range(self.C)])

    def _segment(self, c: int, base: float, steps: int):
        """``steps`` valid steps of chain c from its current state and draw counter."""
        gid, D = self.offset + c, self.chain[c]["draws"]
        enough = 64 * max(steps, 1)
        while True:
            tape = flipref.draw_tape(self.seed, gid, enough, start=D, k=self.k)
            out = self.cref.run(self.spec, self.assign[c], base=base, pop_lo=self.pop_lo, pop_hi=self.pop_hi,
                                seed=self.seed, chain_id=gid, n_steps=steps, k=self.k, labels=self.labels,
                                proposal=self.proposal, nb_pairs=self.nb_pairs, tape=tape, want_hist=self.want_hist)
            if not out["stats"]["stuck"]:
                return out
            enough *= 4  # the tape ran out: a longer one, from the same start draw

    def advance(self, c: int, steps: int):
        """One segment of chain c at the base it holds; returns the deltas attributed to its rung."""
        ch = self.chain[c]
        out = self._segment(c, self.base_now(c), steps)
        st = out["stats"]
        delta = {f: int(st[f]) for f in COUNTERS}
        # the segment's own initial yield is the previous segment's last: not counted again
        delta["sum_cut"] = int(st["sum_cut"]) - ch["cut"]
        delta["sum_nb"] = int(st["sum_nb"]) - ch["nb"]
        delta["sum_cut2"] = int(st["sum_cut2"]) - ch["cut"] ** 2
        delta["sum_nb2"] = int(st["sum_nb2"]) - ch["nb"] ** 2
        hists = None
        if self.want_hist:
            hists = (out["cut_hist"].copy(), out["nb_hist"].copy())
            hists[0][ch["cut"]] -= 1
            hists[1][ch["nb"]] -= 1
        for f in FIELDS:
            ch[f] += delta[f]
        ch["cut"], ch["nb"] = int(st["cut"]), int(st["nb"])
        self.assign[c] = out["final"].copy()
        return delta, hists

    def round(self, steps: int, parity: int = -1, free=False):
        """``steps`` valid steps of every ladder chain (and, with ``free``, of the others too),
        then one exchange round."""
        for c in range(self.C):
            l = self.ladder_of[c]
            if l < 0:
                if free:
                    self.advance(c, steps)
                continue
            r = self.rung_of[c]
            delta, hists = self.advance(c, steps)
            for f in FIELDS:
                self.rung[l][r][f] += delta[f]
            if hists is not None:
                self.rung_cut_hist[l][r] += hists[0]
                self.rung_nb_hist[l][r] += hists[1]
        par = (self.round_no & 1) if parity < 0 else parity
        k0, k1 = self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF
        for l, lad in enumerate(self.ladders):
            G = self.offset + lad[0]
            at = self.chain_at[l]
            for r in range(par, len(lad) - 1, 2):
                x, y = at[r], at[r + 1]
                d = self.chain[x]["cut"] - self.chain[y]["cut"]
                t = int(self.threshold(self.slot_bases[l][r], self.slot_bases[l][r + 1], d))
                w = self.cref.philox([self.round_no & 0xFFFFFFFF, r, G, 4], [k0, k1])
                u = mant53(int(w[0]), int(w[1]))
                acc = u < t
                self.rung[l][r]["swaps_tried"] += 1
                self.rung[l][r]["swaps_accepted"] += int(acc)
                self.decisions.append((self.round_no, l, r, d, t, u, acc))
                if acc:
                    at[r], at[r + 1] = y, x
                    self.rung_of[x], self.rung_of[y] = r + 1, r
        self.round_no += 1


# ---- the configuration tests/test_tempering.py (model alone) and tests/test_tempering_gpu.py share ----
# 12 rounds x 200 steps was the first choice.  With these bases (neighbours a factor 2.6 apart and
# more) the replicas' |cut| are tens of edges apart after 200 steps, and of the ~40 decisions whose
# threshold lies strictly between 0 and 2^53 at most 7 were accepted over 240 seeds tried (100 and
# 200 steps).  The model test needs at least 10 accepted and 10 rejected among them, so that the
# device test compares decisions that depend on the uniform: the members of a ladder start from one
# plan and a round is 12 steps, which keeps |cut| differences at a few edges (seed 6: 12 accepted,
# 38 rejected).  The device test runs 12 x 200 steps from the same starts as a second leg.
SEC11_SEED, SEC11_ROUNDS, SEC11_STEPS, SEC11_CHAINS = 6, 12, 12, 23


def sec11_case(spec):
    """sec11, k = 2, BI_SIGN, 23 chains: ladders of 5, 8, 2 and 1 rungs with interleaved members
    not in index order, and 7 chains in no ladder."""
    from flipcomplexityempirical_amd import graphs as G
    mu = G.SEC11_MU
    ladders = [[3, 17, 0, 9, 21], [1, 20, 5, 12, 7, 15, 2, 19], [22, 4], [11]]
    lad_bases = [[1, mu, 4, mu ** 2, 10], G.SEC11_BASES[2:], [.1, 10], [mu]]
    bases = np.asarray([G.SEC11_BASES[c % 10] for c in range(SEC11_CHAINS)], dtype=np.float64)
    for lad, bs in zip(ladders, lad_bases):
        assert len(lad) == len(bs)
        bases[lad] = bs
    plan_of = {c: l % 3 for l, lad in enumerate(ladders) for c in lad}  # one start plan per ladder
    plans = [spec.assignment_array(G.sec11_plan(a, spec.nodes), [-1, 1]) for a in range(3)]
    inits = np.stack([plans[plan_of.get(c, c % 3)] for c in range(SEC11_CHAINS)])
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), 2, 0.1)
    free = sorted(set(range(SEC11_CHAINS)) - {c for lad in ladders for c in lad})
    return dict(inits=inits, bases=bases, ladders=ladders, pop_lo=lo, pop_hi=hi, seed=SEC11_SEED, free=free)


_CACHE = {}


def sec11_reference(cref, spec, threshold, steps=SEC11_STEPS):
    """The model run of :func:`sec11_case` with histograms (``steps`` per round; 200, the first
    choice, is kept as a second leg of the device test for its longer segments), computed once
    per process: the model and, after every round, copies of what the device is compared with."""
    if steps not in _CACHE:
        case = sec11_case(spec)
        m = TemperingModel(cref, spec, case["inits"], case["bases"], case["ladders"], threshold=threshold,
                           pop_lo=case["pop_lo"], pop_hi=case["pop_hi"], seed=case["seed"], want_hist=True)
        snaps = []
        for _ in range(SEC11_ROUNDS):
            m.round(steps)
            snaps.append(dict(rung_of=m.rung_of.copy(), chain_at=[list(a) for a in m.chain_at], bases=m.bases_now(),
                              chain=[dict(ch) for ch in m.chain], assign=[a.copy() for a in m.assign]))
        _CACHE[steps] = (case, m, snaps)
    return _CACHE[steps]
