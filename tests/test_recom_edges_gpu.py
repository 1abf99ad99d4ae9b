"""GPU parity of the ReCom kernel with the C oracle at small shapes and on every proposal branch.

Every case of ``recom_cases.CASES`` (what each is for, and that the oracle reaches it:
test_recom_cases.py) runs on the device and is compared with ``oracle/recomref.c`` for every
chain: trace records, final assignment, counters and ``stuck``, all bit for bit.  The oracle
gets the chain's own start plan, its own bounds and ``chain_id = chain_id_offset + c``.
"""
import ctypes

import numpy as np
import pytest

import recom_cases as RC
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import RECOM_RECORD_DTYPE, FlipGraph, FlipRun, RunConfig

pytestmark = pytest.mark.gpu

COUNTERS = (("steps", "steps"), ("proposals", "proposals"), ("accepted", "accepted"), ("inv_pop", "inv_pop"),
            ("sum_cut", "sum_cut"), ("sum_nb", "sum_nb"), ("cut", "cut"), ("nb", "nb"), ("bfs_calls", "attempts"),
            ("bfs_levels", "trees"), ("stuck", "stuck"))


def _run(case, spec=None, **cfg_over):
    spec = case.spec if spec is None else spec
    nc = case.n_chains
    lohi = np.asarray([case.chain_bounds(c) for c in range(nc)], dtype=np.int64)
    cfg = dict(k=case.k, labels=tuple(range(case.k)), proposal=_lib.FC_PROPOSE_RECOM, seed=RC.SEED,
               pop_lo=int(lohi[0, 0]), pop_hi=int(lohi[0, 1]), base=case.base, chain_id_offset=case.chain_id_offset,
               recom_pop_target=case.pop_target, recom_epsilon=case.epsilon, recom_node_repeats=case.node_repeats,
               recom_max_attempts=case.max_attempts, trace_chains=case.n_traced,
               trace_cap=case.trace_cap or case.room, diag_mask=0)
    cfg.update(cfg_over)
    # per-chain bounds go through chain_pop_bounds only where the case has more than one pair
    return FlipRun(FlipGraph(spec), np.stack([case.plan(c) for c in range(nc)]), RunConfig(**cfg),
                   pop_bounds=lohi if len(case.bounds()) > 1 else None)


def _read_trace(run, c, cap):
    """The first ``cap`` records of chain c and the number the chain produced (no OverflowError)."""
    out = np.zeros(cap, dtype=RECOM_RECORD_DTYPE)
    n = ctypes.c_int64(0)
    rc = _lib.load().fc_run_read_recom_trace(run.handle, c, ctypes.cast(out.ctypes.data, ctypes.POINTER(_lib.RecomRecord)),
                                             cap, ctypes.byref(n))
    assert rc == 0
    return out[:min(cap, n.value)], int(n.value)


def _consistent(case, cref, run, c, st, fin):
    """Chain c's state is a plan of k contiguous districts inside its bounds, and its counters
    describe that state."""
    lo, hi = case.chain_bounds(c)
    cut, nb, pops = G.cut_and_boundary(case.spec, fin[c])
    assert (cut, nb) == (int(st["cut"][c]), int(st["nb"][c])), (case.name, c)
    assert len(pops) == case.k and lo <= pops.min() and pops.max() <= hi, (case.name, c)
    assert cref.districts_contiguous(case.spec, fin[c], case.k), (case.name, c)


@pytest.mark.parametrize("name", list(RC.BY_NAME))
def test_recom_case_matches_oracle(gpu, cref, name):
    case = RC.BY_NAME[name]
    refs = [case.oracle(c) for c in range(case.n_chains)]
    for c, ref in enumerate(refs):
        assert case.chain_ok(case, ref), (name, c)
    run = _run(case)
    if case.max_draws:
        run.steps(case.steps, max_draws=case.max_draws)  # the device cap is per launch, the oracle's per run
    else:
        # across launches; a chain that gets stuck must do so in the last (the oracle stops there)
        first = min(case.steps // 2, min(r["stats"]["steps"] for r in refs))
        if first:
            run.steps(first)
        run.steps(case.steps - first)
    st, fin = run.stats(), run.state()
    assert run.kernel_name() == case.kernel
    for c, ref in enumerate(refs):
        rs, rt = ref["stats"], ref["trace"]
        for kd, kr in COUNTERS:
            assert int(st[kd][c]) == int(rs[kr]), (name, c, kd)
        assert np.array_equal(fin[c], ref["final"]), (name, c)
        _consistent(case, cref, run, c, st, fin)
        if c >= case.n_traced:  # traced chains only
            continue
        if case.trace_cap:
            assert len(rt) > case.trace_cap
            with pytest.raises(OverflowError):
                run.recom_trace(c)
            tr, n_rec = _read_trace(run, c, case.trace_cap)
            assert n_rec == len(rt) and len(tr) == case.trace_cap
            rt = rt[:case.trace_cap]
        else:
            tr = run.recom_trace(c)
        assert len(tr) == len(rt), (name, c)
        for f in RC.TRACE_FIELDS:
            assert np.array_equal(tr[f], rt[f]), (name, c, f)
    if case.n_traced < case.n_chains:
        with pytest.raises(ValueError, match="not traced"):
            run.recom_trace(case.n_traced)
    if any(r["stats"]["stuck"] for r in refs):
        # a stuck chain's next launch goes on from the next draw: the run stays consistent
        run.steps(3)
        st2, fin2 = run.stats(), run.state()
        for c in range(case.n_chains):
            _consistent(case, cref, run, c, st2, fin2)
            assert int(st2["proposals"][c]) > int(st["proposals"][c]), (name, c)
            assert int(st["steps"][c]) <= int(st2["steps"][c]) <= int(st["steps"][c]) + 3, (name, c)
            assert int(st2["steps"][c]) == int(st["steps"][c]) + 3 or int(st2["stuck"][c]) == 1, (name, c)
            assert int(st2["accepted"][c]) - int(st["accepted"][c]) <= int(st2["steps"][c]) - int(st["steps"][c])
            if int(st2["steps"][c]) == int(st["steps"][c]):
                assert np.array_equal(fin2[c], fin[c]), (name, c)


def test_recom_refuses_population_totals_past_int32(gpu):
    """Subtree populations are int32 with bit 31 as the subset mark: a total of 2^32 is refused
    (FC_ERR_UNSUPPORTED, naming the limit), the largest legal totals run (the top-of-range case)."""
    with pytest.raises(NotImplementedError, match="INT32_MAX = 2147483647"):  # FC_ERR_UNSUPPORTED
        RC.create_run(RC.overweight_grid())
    run = _run(RC.BY_NAME["top of range 4x4 k=2"]).steps(1)
    assert np.array_equal(run.stats()["steps"], np.ones(run.n_chains))


def test_recom_refuses_more_than_8000_nodes(gpu):
    with pytest.raises(NotImplementedError, match="n <= 8000"):
        RC.create_run(RC.grid(127, 63))  # n = 8001
