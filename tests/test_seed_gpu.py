"""GPU parity of the seed-plan kernel (fc_seed.hip, ``fc_graph_seed_plans``) with the Python
model of the definition (tests/seed_model.py), and the seed plans' way into runs.

Every case of ``seed_cases.CASES`` (what each is for, and that the model reaches it:
test_seed_cases.py) runs on the device and is compared bit for bit, plan by plan: the row and
``attempts``, ``trees``, ``restarts``, ``ok``; ``cut`` / ``nb`` against ``graphs.cut_and_boundary``.
Contiguity and bounds are also checked without the model (the C oracle's ``districts_contiguous``).
"""
import functools

import networkx as nx
import numpy as np
import pytest

import recom_cases as RC
import seed_cases as SC
import test_pair_gpu as TP
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd import chain as C
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig
from oracle.flipref import recom_run

pytestmark = pytest.mark.gpu

FIELDS = ("attempts", "trees", "restarts", "ok")


def _seed(case, n_plans=None, offset=None, fg=None, **kw):
    fg = FlipGraph(case.spec) if fg is None else fg
    return fg.seed_plans(case.k, case.n_plans if n_plans is None else n_plans, pop_bounds=case.bounds, seed=SC.SEED,
                         plan_id_offset=case.plan_id_offset if offset is None else offset, strict=False,
                         **case.params, **kw)


@pytest.mark.parametrize("name", list(SC.BY_NAME))
def test_seed_case_matches_model(gpu, cref, name):
    case = SC.BY_NAME[name]
    ref = case.model()
    assert case.ok(case, ref), name
    fg = FlipGraph(case.spec)
    if case.kernel.endswith("<16>"):
        assert fg.info["ring_max"] == 16
    plans, st = _seed(case, fg=fg)
    assert st["kernel"] == case.kernel
    assert plans.shape == (case.n_plans, case.spec.n) and plans.dtype == np.int8
    lo, hi = case.bounds
    for i, r in enumerate(ref):
        for f in FIELDS:
            assert int(st[f][i]) == int(r[f]), (name, i, f)
        assert np.array_equal(plans[i], r["assign"]), (name, i)
        if not r["ok"]:
            assert np.all(plans[i] == -1) and (int(st["cut"][i]), int(st["nb"][i])) == (0, 0), (name, i)
            continue
        # independent of the model: counters, bounds and contiguity from the row
        cut, nb, pops = G.cut_and_boundary(case.spec, plans[i])
        assert (cut, nb) == (int(st["cut"][i]), int(st["nb"][i])), (name, i)
        assert len(pops) == case.k and lo <= pops.min() and pops.max() <= hi, (name, i)
        assert cref.districts_contiguous(case.spec, plans[i], case.k), (name, i)


def test_plans_do_not_depend_on_the_sharding(gpu):
    """Plans 1000..1036 in one call, in two calls, and one call per plan."""
    case = SC.BY_NAME["many blocks 8x8 k=2"]
    fg = FlipGraph(case.spec)
    whole, st = _seed(case, fg=fg)
    a, sa = _seed(case, 20, 1000, fg=fg)
    b, sb = _seed(case, 17, 1020, fg=fg)
    assert np.array_equal(whole, np.concatenate([a, b]))
    for f in FIELDS + ("cut", "nb"):
        assert np.array_equal(st[f], np.concatenate([sa[f], sb[f]])), f
    for i in (0, 19, 36):
        one, so = _seed(case, 1, 1000 + i, fg=fg)
        assert np.array_equal(one[0], whole[i]) and all(int(so[f][0]) == int(st[f][i]) for f in FIELDS + ("cut", "nb"))
    assert len({p.tobytes() for p in whole}) > 18  # and they are not one plan 37 times


def test_seeds_start_pair_and_recom_runs(gpu, cref):
    """The 8x8 k = 4 seeds, one per chain: fc_run_create accepts every plan (its own validation:
    contiguity and bounds); after 40 steps the ReCom run equals the oracle started from the same
    plan, and the PAIR run equals the C oracle as test_pair_gpu.py compares."""
    case = SC.BY_NAME["size 8x8 k=4"]
    spec, k = case.spec, case.k
    lo, hi = case.bounds
    pct = 0.0625  # (15, 17) through population_bounds
    assert G.population_bounds(int(spec.pop.sum()), k, pct)[1] == (lo, hi)
    plans, st = _seed(case, 8)
    assert np.all(st["ok"] == 1) and len({p.tobytes() for p in plans}) > 1
    # ReCom
    target = int(spec.pop.sum()) / k
    cfg = RunConfig(k=k, labels=tuple(range(k)), proposal=_lib.FC_PROPOSE_RECOM, seed=5, pop_lo=lo, pop_hi=hi,
                    recom_pop_target=target, recom_epsilon=0.1, diag_mask=0)
    run = FlipRun(FlipGraph(spec), plans, cfg).steps(40)
    rs, fin = run.stats(), run.state()
    for c in range(len(plans)):
        ref = recom_run(spec, plans[c], k=k, pop_target=target, epsilon=0.1, pop_lo=lo, pop_hi=hi, seed=5, chain_id=c,
                        n_steps=40, max_attempts=10000)
        for kd, kr in (("steps", "steps"), ("proposals", "proposals"), ("accepted", "accepted"), ("inv_pop", "inv_pop"),
                       ("sum_cut", "sum_cut"), ("sum_nb", "sum_nb"), ("cut", "cut"), ("nb", "nb"),
                       ("bfs_calls", "attempts"), ("bfs_levels", "trees"), ("stuck", "stuck")):
            assert int(rs[kd][c]) == int(ref["stats"][kr]), (c, kd)
        assert np.array_equal(fin[c], ref["final"]), c
    run.close()
    # PAIR
    bases = np.asarray([[0.5, 1.0, 2.0, 4.0][c % 4] for c in range(len(plans))])
    prun = TP._run_pair(spec, plans, bases, k, steps=40, pct=pct)
    TP._check(cref, spec, prun, k, plans, bases, steps=40, pct=pct)
    prun.close()


def test_strict_names_the_failed_plans(gpu):
    case = SC.BY_NAME["mixed 8x8 k=4"]
    ref = case.model()
    failed = [case.plan_id_offset + i for i, r in enumerate(ref) if not r["ok"]]
    assert failed and len(failed) < case.n_plans
    fg = FlipGraph(case.spec)
    with pytest.raises(RuntimeError, match="plan ids " + ", ".join(map(str, failed)) + r"\)"):
        fg.seed_plans(case.k, case.n_plans, pop_bounds=case.bounds, seed=SC.SEED, **case.params)
    plans, st = fg.seed_plans(case.k, case.n_plans, pop_bounds=case.bounds, seed=SC.SEED, strict=False, **case.params)
    assert np.array_equal(st["ok"], [r["ok"] for r in ref])
    assert np.array_equal(np.all(plans == -1, axis=1), st["ok"] == 0)
    # percent goes through graphs.population_bounds
    spec = RC.grid(8, 8)
    p1, _ = FlipGraph(spec).seed_plans(2, 3, percent=0.1, seed=SC.SEED)
    p2, _ = FlipGraph(spec).seed_plans(2, 3, pop_bounds=G.population_bounds(64, 2, 0.1)[1], seed=SC.SEED)
    assert np.array_equal(p1, p2)


def test_recursive_tree_part_through_the_chain_api(gpu):
    g = nx.grid_2d_graph(8, 8)
    for nd in g.nodes:
        g.nodes[nd]["population"] = 1
    parts = [5, 6, 7, 8]
    plan = C.recursive_tree_part(g, parts, 16, "population", 0.07, seed=11, plan_id=3)
    assert set(plan) == set(g.nodes) and set(plan.values()) == set(parts)
    assert plan == C.recursive_tree_part(g, parts, 16, "population", 0.07, seed=11, plan_id=3)
    assert plan != C.recursive_tree_part(g, parts, 16, "population", 0.07, seed=11, plan_id=4)
    ups = {"population": C.Tally("population"), "cut_edges": C.cut_edges, "base": lambda p: 1.0}
    part = C.Partition(g, plan, ups)
    assert C.contiguous(part) and all(15 <= v <= 17 for v in part["population"].values())  # |s - 16| <= 1.12
    tree = functools.partial(C.recom, pop_col="population", pop_target=16, epsilon=0.07, node_repeats=1)
    pb = C.within_percent_of_ideal_population(part, 0.07)
    res = C.MarkovChain(tree, C.Validator([pb]), accept=C.always_accept, initial_state=part, total_steps=11, seed=2).run()
    assert res.steps == 10
    # the device plan is the model's plan 3 under the integer bounds (15, 17)
    spec = RC.grid(8, 8)
    import seed_model
    ref = seed_model.seed_plan(spec, 4, 15, 17, 11, 3)
    assert ref["ok"] == 1
    assert [plan[nd] for nd in spec.nodes] == [parts[d] for d in ref["assign"]]


def test_kernel_time_is_reported_and_changes_nothing(gpu):
    case = SC.BY_NAME["size 16x16 k=4"]
    fg = FlipGraph(case.spec)
    plain, st0 = _seed(case, fg=fg)
    timed, st1 = _seed(case, fg=fg, timing=True)
    assert "kernel_ms" not in st0 and st1["kernel_ms"] > 0.0
    assert np.array_equal(plain, timed)
    for f in FIELDS + ("cut", "nb"):
        assert np.array_equal(st0[f], st1[f]), f
