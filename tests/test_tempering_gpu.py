"""Replica exchange on the device (fc_run_set_ladders / fc_run_exchange; DESIGN.md "Replica
exchange") against the host model of tests/tempering_model.py, bit for bit: rung maps, bases,
every ladder chain's state and counters after every round, the per-rung sums, swap counters and
histograms; the equal-bases shuffle against the same run without ladders (sum_wait and wait_cur
included); other graph / kernel layouts; checkpoint / restore; and the argument errors."""
import ctypes
import struct

import numpy as np
import pytest

import tempering_model as TM
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
from flipcomplexityempirical_amd.tempering import TemperedRun, swap_threshold

pytestmark = pytest.mark.gpu

FULL = _lib.FC_DIAG_WAIT | _lib.FC_DIAG_HIST | _lib.FC_DIAG_EDGES | _lib.FC_DIAG_FLIPS
CHAIN_KEYS = TM.FIELDS + ("cut", "nb")
ALL_KEYS = ("steps", "proposals", "draws", "accepted", "inv_contig", "inv_pop", "sum_cut", "sum_nb", "sum_wait",
            "sum_cut2", "sum_nb2", "wait_cur", "cut", "nb", "last_flip")
RUNG_KEYS = [f for f, _ in _lib.RungStats._fields_]


def _check_maps(run, rung_of, chain_at, bases):
    ro, ca = run.rungs()
    assert np.array_equal(ro, rung_of)
    assert [list(x) for x in ca] == [list(x) for x in chain_at]
    assert np.array_equal(run.bases_now(), bases)  # the very doubles the run was created with


def _check_rung_stats(run, m, hist):
    rs = run.rung_stats()
    s = 0
    for l, lad in enumerate(m.ladders):
        for r in range(len(lad)):
            for f in TM.FIELDS + ("swaps_tried", "swaps_accepted"):
                assert int(rs[f][s]) == m.rung[l][r][f], (l, r, f)
            if hist:
                assert np.array_equal(rs["cut_hist"][s], m.rung_cut_hist[l][r]), (l, r)
                assert np.array_equal(rs["nb_hist"][s], m.rung_nb_hist[l][r]), (l, r)
            s += 1
    return rs


def _sec11_run(sec11, case, diag, hist, ladders=True):
    cfg = RunConfig(seed=case["seed"], pop_lo=case["pop_lo"], pop_hi=case["pop_hi"], diag_mask=diag)
    run = FlipRun(FlipGraph(sec11), case["inits"], cfg, bases=case["bases"])
    if ladders:
        run.set_ladders(case["ladders"], hist=hist)
    return run


_FREE = {}


def _free_refs(cref, sec11, steps):
    """The chains in no ladder: plain oracle runs from step 0, one per round's end."""
    if steps not in _FREE:
        case = TM.sec11_case(sec11)
        _FREE[steps] = {(c, i): cref.run(sec11, case["inits"][c], base=case["bases"][c], pop_lo=case["pop_lo"],
                                         pop_hi=case["pop_hi"], seed=case["seed"], chain_id=c, n_steps=(i + 1) * steps,
                                         log1mp=G.log1mp_table(sec11.n, 2))
                        for c in case["free"] for i in range(TM.SEC11_ROUNDS)}
    return _FREE[steps]


@pytest.mark.parametrize("diag,steps", [("lean", TM.SEC11_STEPS), ("full", TM.SEC11_STEPS), ("full", 200)])
def test_whole_run_against_model(gpu, cref, sec11, diag, steps):
    """lean: the FC_DIAG_WAIT instance, no histograms; full: every diagnostic, so the exchange
    follows tally log -> tally_reduce on the stream and attributes the histogram rows.  Rounds of
    TM.SEC11_STEPS steps are the case whose swap decisions go both ways (tempering_model.py); rounds
    of 200 steps add longer segments between mostly one-sided decisions."""
    case, m, snaps = TM.sec11_reference(cref, sec11, swap_threshold, steps)
    free_refs = _free_refs(cref, sec11, steps)
    hist = diag == "full"
    run = _sec11_run(sec11, case, FULL if hist else _lib.FC_DIAG_WAIT, hist)
    in_ladder = [c for lad in case["ladders"] for c in lad]
    for i, snap in enumerate(snaps):
        run.steps(steps)
        run.exchange()
        _check_maps(run, snap["rung_of"], snap["chain_at"], snap["bases"])
        st, fin = run.stats(), run.state()
        for c in in_ladder:
            assert np.array_equal(fin[c], snap["assign"][c]), (i, c)
            for f in CHAIN_KEYS:
                assert int(st[f][c]) == snap["chain"][c][f], (i, c, f)
        for c in case["free"]:
            ref = free_refs[(c, i)]
            assert np.array_equal(fin[c], ref["final"]), (i, c)
            for f in ("steps", "proposals", "draws", "accepted", "inv_contig", "inv_pop", "sum_cut", "sum_nb",
                      "sum_wait", "wait_cur", "cut", "nb"):
                assert int(st[f][c]) == int(ref["stats"][f]), (i, c, f)
    rs = _check_rung_stats(run, m, hist)
    # sum_wait is not the model's (a segment redraws its first wait): the slots of a ladder share
    # out exactly what its chains accumulated
    off, st = rs["ladder_off"], run.stats()
    for l, lad in enumerate(case["ladders"]):
        assert rs["sum_wait"][off[l]:off[l + 1]].sum() == st["sum_wait"][lad].sum()
    if hist:
        ch, nh = run.hist()
        for l, lad in enumerate(case["ladders"]):
            assert np.array_equal(rs["cut_hist"][off[l]:off[l + 1]].sum(axis=0), ch[lad].sum(axis=0))
            assert np.array_equal(rs["nb_hist"][off[l]:off[l + 1]].sum(axis=0), nh[lad].sum(axis=0))
    run.close()


def test_equal_bases_is_a_shuffle(gpu, sec11):
    """Every rung at base mu: every swap is accepted, the rung map is the even / odd shuffle, and
    since equal temperatures change nothing, every chain equals the same run without ladders in
    state and in all statistics (sum_wait, wait_cur, histograms); the rung sums add up to them."""
    C, R, S = 14, 7, 150
    ladders = [[4, 0, 5, 2, 1, 3], [10, 7, 6, 9, 8]]
    inits = np.stack([sec11.assignment_array(G.sec11_plan(c % 3, sec11.nodes), [-1, 1]) for c in range(C)])
    bases = np.full(C, G.SEC11_MU)
    bases[11:] = [0.8, 1.0, 4.0]
    _, (lo, hi) = G.population_bounds(int(sec11.pop.sum()), 2, 0.1)
    cfg = RunConfig(seed=99, pop_lo=lo, pop_hi=hi, diag_mask=_lib.FC_DIAG_WAIT | _lib.FC_DIAG_HIST)
    fg = FlipGraph(sec11)
    a = FlipRun(fg, inits, cfg, bases=bases).set_ladders(ladders, hist=True)
    b = FlipRun(fg, inits, cfg, bases=bases)
    at = [list(lad) for lad in ladders]
    for t in range(R):  # no read-out, so no host synchronisation, between the launches
        a.steps(S)
        a.exchange()
        b.steps(S)
        for x in at:
            for r in range(t & 1, len(x) - 1, 2):
                x[r], x[r + 1] = x[r + 1], x[r]
    rung_of = np.full(C, -1, dtype=np.int32)
    for x in at:
        for r, c in enumerate(x):
            rung_of[c] = r
    _check_maps(a, rung_of, at, bases)
    sa, sb = a.stats(), b.stats()
    for f in ALL_KEYS:
        assert np.array_equal(sa[f], sb[f]), f
    assert np.array_equal(a.state(), b.state())
    for x, y in zip(a.hist(), b.hist()):
        assert np.array_equal(x, y)
    rs = a.rung_stats()
    off = rs["ladder_off"]
    for l, lad in enumerate(ladders):
        sl = slice(off[l], off[l + 1])
        for f in RUNG_KEYS[:11]:
            assert rs[f][sl].sum() == sb[f][lad].sum(), (l, f)
        assert np.array_equal(rs["steps"][sl], np.full(len(lad), R * S))
        tried = [sum(1 for t in range(R) if (t & 1) == (r & 1)) if r + 1 < len(lad) else 0 for r in range(len(lad))]
        assert list(rs["swaps_tried"][sl]) == tried and list(rs["swaps_accepted"][sl]) == tried
        for key, full in (("cut_hist", b.hist()[0]), ("nb_hist", b.hist()[1])):
            assert np.array_equal(rs[key][sl].sum(axis=0), full[lad].sum(axis=0))
    # a second read-out attributes nothing twice
    rs2 = a.rung_stats()
    for f in RUNG_KEYS:
        assert np.array_equal(rs[f], rs2[f]), f
    a.close()
    b.close()


def _layout_case(name, sec11, frank):
    if name == "frank":  # n = 800 (no multiple of 64), histogram rows of odd width
        spec, k, labels, prop, flags, pct = frank, 2, (-1, 1), _lib.FC_PROPOSE_BI_SIGN, 0, 0.05
        inits = np.stack([spec.assignment_array(G.frank_plan(c % 3, spec.nodes), [-1, 1]) for c in range(7)])
        ladders, lad_bases = [[5, 0, 3], [1, 6, 2]], [.3, 1.0, 1 / .3]
        bases = np.ones(7)
    else:                # the k = 4 PAIR shape of test_chain_k4_gpu.py
        spec, k, labels, prop, flags, pct = sec11, 4, (0, 1, 2, 3), _lib.FC_PROPOSE_PAIR, _lib.FC_FLAG_NB_PAIRS, 0.05
        inits = np.stack([spec.assignment_array(G.quadrant_plan(spec.nodes), list(range(4)))] * 5)
        ladders, lad_bases = [[2, 4, 0, 3]], [0.5, 1.0, G.SEC11_MU, 4.0]
        bases = np.ones(5)
    for lad in ladders:
        bases[lad] = lad_bases
    _, (lo, hi) = G.population_bounds(int(spec.pop.sum()), k, pct)
    return spec, k, labels, prop, flags, inits, ladders, bases, lo, hi


@pytest.mark.parametrize("name", ["frank", "k4_pair"])
def test_other_layouts(gpu, cref, sec11, frank, name):
    spec, k, labels, prop, flags, inits, ladders, bases, lo, hi = _layout_case(name, sec11, frank)
    hist = name == "frank"
    m = TM.TemperingModel(cref, spec, inits, bases, ladders, threshold=swap_threshold, k=k, proposal=int(prop),
                          pop_lo=lo, pop_hi=hi, seed=41, labels=labels, nb_pairs=bool(flags), want_hist=hist)
    cfg = RunConfig(k=k, labels=labels, proposal=prop, flags=flags, seed=41, pop_lo=lo, pop_hi=hi,
                    diag_mask=_lib.FC_DIAG_WAIT | (_lib.FC_DIAG_HIST if hist else 0))
    run = FlipRun(FlipGraph(spec), inits, cfg, bases=bases).set_ladders(ladders, hist=hist)
    for _ in range(6):
        run.steps(100)
        run.exchange()
        m.round(100)
        _check_maps(run, m.rung_of, m.chain_at, m.bases_now())
    if hist:
        assert (spec.n_edges + 1) % 2 == 1 or (spec.n + 1) % 2 == 1  # a padded row is exercised
    _check_rung_stats(run, m, hist)
    run.close()


def test_checkpoint_restore_with_ladders(gpu, cref, sec11):
    case, m, snaps = TM.sec11_reference(cref, sec11, swap_threshold)
    a = _sec11_run(sec11, case, FULL, True)
    for _ in range(5):
        a.steps(TM.SEC11_STEPS).exchange()
    blob = a.checkpoint()
    for _ in range(TM.SEC11_ROUNDS - 5):
        a.steps(TM.SEC11_STEPS).exchange()
    b = _sec11_run(sec11, case, FULL, True)
    b.steps(11).exchange()  # diverge first: the restore must overwrite everything that matters
    b.restore(blob)
    for _ in range(TM.SEC11_ROUNDS - 5):
        b.steps(TM.SEC11_STEPS).exchange()
    last = snaps[-1]
    for run in (a, b):  # both are the uninterrupted run the model describes
        _check_maps(run, last["rung_of"], last["chain_at"], last["bases"])
    sa, sb = a.stats(), b.stats()
    for f in ALL_KEYS:
        assert np.array_equal(sa[f], sb[f]), f
    assert np.array_equal(a.state(), b.state())
    ra, rb = a.rung_stats(), _check_rung_stats(b, m, True)
    for f in RUNG_KEYS + ["cut_hist", "nb_hist"]:
        assert np.array_equal(ra[f], rb[f]), f
    # the header carries the ladder layout: no restore into a run without ladders or with others
    assert struct.unpack_from("<I", blob, 12)[0] != 0
    plain = _sec11_run(sec11, case, FULL, False, ladders=False)
    with pytest.raises(ValueError, match="ladders"):
        plain.restore(blob)
    other = _sec11_run(sec11, case, FULL, False, ladders=False)
    other.set_ladders([case["ladders"][0][::-1]] + case["ladders"][1:], hist=True)
    with pytest.raises(ValueError, match="ladders"):
        other.restore(blob)
    # a run without ladders writes the blob it always wrote: same length, reserved word 0
    pb = plain.checkpoint()
    C, npad, R, E, n = TM.SEC11_CHAINS, 1600, 8, sec11.n_edges, sec11.n
    magic, ver, reserved = struct.unpack_from("<8sII", pb, 0)
    payload = struct.unpack_from("<q", pb, 64)[0]
    assert (magic, ver, reserved) == (b"FCCKPT03", 3, 0)
    sections = C * (2 * npad + 192 + 32 * 4 + (2 * R + 1) * 8)   # assign, fcnt, ChainScalars, popk, thresholds
    sections += C * 8 * ((E + 1) + (n + 1) + E + 3 * n)           # histograms, cut_times, flips
    assert payload == sections and len(pb) == 88 + payload
    assert len(blob) > len(pb)
    for run in (a, b, plain, other):
        run.close()


def test_argument_errors(gpu, sec11):
    L = _lib.load()
    C = 6
    inits = np.stack([sec11.assignment_array(G.sec11_plan(0, sec11.nodes), [-1, 1])] * C)
    _, (lo, hi) = G.population_bounds(int(sec11.pop.sum()), 2, 0.1)
    fg = FlipGraph(sec11)

    def rc(run, ladders, flags=0):
        off = np.zeros(len(ladders) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(x) for x in ladders])
        mem = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32) for x in ladders]), dtype=np.int32)
        return L.fc_run_set_ladders(run.handle, len(ladders), off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    mem.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), flags)

    cfg = RunConfig(seed=3, pop_lo=lo, pop_hi=hi)
    run = FlipRun(fg, inits, cfg, bases=np.linspace(1, 2, C))
    assert L.fc_run_exchange(run.handle, -1, None) == _lib.FC_ERR_ARG          # before set_ladders
    assert rc(run, [[0, 1, 2], [2, 3]]) == _lib.FC_ERR_ARG                      # overlapping ladders
    assert rc(run, [[0, 1], [4, C]]) == _lib.FC_ERR_ARG                         # index out of range
    assert rc(run, [[0, -1]]) == _lib.FC_ERR_ARG
    assert rc(run, [[0, 1]], _lib.FC_LADDER_HIST) == _lib.FC_ERR_ARG            # no FC_DIAG_HIST
    assert rc(run, [[0, 1]], 0x80) == _lib.FC_ERR_ARG                           # unknown flag
    assert rc(run, [[0, 1], [3, 2]]) == _lib.FC_OK                              # nothing above stuck
    assert rc(run, [[4, 5]]) == _lib.FC_ERR_ARG                                 # callable once
    assert L.fc_run_exchange(run.handle, 2, None) == _lib.FC_ERR_ARG
    assert L.fc_run_exchange(run.handle, 1, None) == _lib.FC_OK
    run.close()
    bounds = np.tile([lo, hi], (C, 1))
    bounds[3] = [lo - 1, hi + 1]
    run = FlipRun(fg, inits, cfg, bases=np.linspace(1, 2, C), pop_bounds=bounds)
    assert rc(run, [[0, 1], [2, 3]]) == _lib.FC_ERR_ARG                         # unequal population bounds
    assert rc(run, [[0, 1, 2], [4, 5]]) == _lib.FC_OK
    run.close()
    anneal = FlipRun(fg, inits, RunConfig(seed=3, pop_lo=lo, pop_hi=hi, accept=_lib.FC_ACCEPT_ANNEAL, beta=5.0, base=2.0))
    assert rc(anneal, [[0, 1]]) == _lib.FC_ERR_UNSUPPORTED
    anneal.close()
    recom = FlipRun(fg, inits, RunConfig(proposal=_lib.FC_PROPOSE_RECOM, seed=5, pop_lo=lo, pop_hi=hi, base=1.0,
                                         recom_pop_target=sec11.n / 2, recom_epsilon=0.1))
    assert rc(recom, [[0, 1]]) == _lib.FC_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        recom.set_ladders([[0, 1]])
    recom.close()


def test_tempered_run_driver(gpu, sec11):
    """tempering.TemperedRun: L ladders x m rungs from plans; per-rung read-outs are consistent."""
    plans = np.stack([sec11.assignment_array(G.sec11_plan(a, sec11.nodes), [-1, 1]) for a in range(3)])
    _, (lo, hi) = G.population_bounds(int(sec11.pop.sum()), 2, 0.1)
    bases = [1.0, 1.3, 1.7, 2.2]
    tr = TemperedRun(FlipGraph(sec11), plans, bases, RunConfig(seed=8, pop_lo=lo, pop_hi=hi), hist=True)
    res = tr.advance(6, 100).results()
    assert np.array_equal(res["yields"], np.full(4, 3 * 601))
    assert np.array_equal(res["cut_hist"].sum(axis=1), res["yields"])
    assert np.array_equal((res["cut_hist"] * np.arange(res["cut_hist"].shape[1])).sum(axis=1), res["sum_cut"])
    assert np.array_equal(res["swaps_tried"], [9, 9, 9]) and (res["swaps_accepted"] <= res["swaps_tried"]).all()
    assert res["swaps_accepted"].sum() > 0  # neighbouring bases this close do trade places
    assert sorted(tr.run.bases_now()) == sorted(bases * 3)
    tr.close()
