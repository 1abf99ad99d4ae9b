"""GPU parity of the k = 2 tallies with the C oracle on every pass plan, under log overflow and at
the field edges of the log entry.

Every case of ``tally_cases.CASES`` (what each is for, and that its oracle run and its plan reach
it: test_tally_cases.py) runs on the device under each of its variants, and every chain is compared
with ``oracle/flipref.c`` bit for bit on the scalars, the final state and populations, both
histograms, ``cut_times``, the quirk tallies and the corrected ones -- only what the variant's
diagnostics keep; the readers of what it does not keep must refuse.  Two invariants hold without
the oracle: every histogram row sums to steps + 1, and ``flip_count`` sums to ``accepted``.

Each variant asserts its kernel instance by name and, through ``FlipRun.tally_plan()``, the pass
plan the reduce launched: the plan of ``csrc/fc_tally_plan.h`` (asked of the native program) at
the limit the device reported.  The cases of the hand-written table need that limit to be 163,840
bytes and fail, naming the limit, on a device that reports another; a pass demoted to global
atomics because the device refused its LDS shows as a plan that differs.
"""
import time

import numpy as np
import pytest

import flip_cases as FC
import tally_cases as TC
from flipcomplexityempirical_amd import _lib
from flipcomplexityempirical_amd.engine import FlipGraph, FlipRun, RunConfig


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = TC.build_plan_check(tmp_path_factory.mktemp("tally_plan"))
    assert out is not None, "no host C++ toolchain: the expected plans come from tests/native/tally_plan_check.cpp"
    return out


def _run(case, diag, flags, tune):
    nc = case.n_chains
    fg = FlipGraph(case.spec)
    lohi = np.asarray([case.chain_bounds(c) for c in range(nc)], dtype=np.int64)
    cfg = RunConfig(k=2, labels=case.labels, proposal=_lib.FC_PROPOSE_BI_SIGN, seed=case.seed, pop_lo=int(lohi[0, 0]),
                    pop_hi=int(lohi[0, 1]), diag_mask=diag, flags=flags, tune=dict(tune))
    run = FlipRun(fg, np.stack([case.plan(c) for c in range(nc)]), cfg, bases=[case.base(c) for c in range(nc)],
                  pop_bounds=lohi)
    t = time.perf_counter()
    for n in case.launch_steps():
        run.steps(n)
    run.sync()
    return fg, run, time.perf_counter() - t


def _check(case, run, diag):
    """Every chain of the run against the oracle's run of the same chain, on what `diag` keeps."""
    st, fin, pops = run.stats(), run.state(), run.pops()
    kept = {}
    for bit, reader, keys in ((TC.HIST, run.hist, ("cut_hist", "nb_hist")), (TC.EDGES, run.cut_times, ("cut_times",)),
                              (TC.FLIPS, run.flips, ("num_flips", "part_sum", "last_flipped")),
                              (TC.EXACT, run.flips_exact, ("flip_count", "occupancy", "last_accept"))):
        if diag & bit:
            got = reader()
            kept.update(zip(keys, got if isinstance(got, tuple) else (got,)))
        else:
            with pytest.raises(ValueError, match="not enabled"):
                reader()
    for c in range(case.n_chains):
        ref = case.oracle(c)
        who = (case.name, c)
        for key in FC.STAT_KEYS:
            assert int(st[key][c]) == int(ref["stats"][key]), f"{who} stat {key}: {st[key][c]} vs {ref['stats'][key]}"
        assert np.array_equal(fin[c], ref["final"]), who
        want = np.bincount(ref["final"], weights=case.spec.pop, minlength=2).astype(np.int64)
        assert np.array_equal(pops[c], want), who
        for key, arr in kept.items():
            bad = np.nonzero(arr[c] != ref[key])[0]
            assert bad.size == 0, f"{who} {key}: {bad.size} entries differ, first at {bad[:3]}: {arr[c][bad[:3]]} vs {ref[key][bad[:3]]}"
        if diag & TC.HIST:
            assert int(kept["cut_hist"][c].sum()) == int(kept["nb_hist"][c].sum()) == case.steps + 1, who
        if diag & TC.EXACT:
            assert int(kept["flip_count"][c].sum()) == int(st["accepted"][c]), who


PARAMS = [pytest.param(c.name, v[0], marks=[pytest.mark.slow] if c.slow else [], id=f"{c.name}-{v[0]}")
          for c in TC.CASES for v in c.variants]


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", PARAMS)
def test_tallies_match_oracle(gpu, exe, name, variant):
    case = TC.BY_NAME[name]
    _, diag, flags, tune = next(v for v in case.variants if v[0] == variant)
    fg, run, secs = _run(case, diag, flags, tune)
    print(f"\n{name} [{variant}]: {case.steps} steps x {case.n_chains} chains on the device in {secs:.2f} s, "
          f"last call {run.last_ms():.1f} ms")
    search = fg.info["n_exact"] != fg.n
    assert not search
    assert run.kernel_name() == "fc::flip2_kernel<%d, 4, true, false, false, false>" % fg.info["ring_max"]
    if case.group == "ring16" or name == "ovf delaunay_wide":
        assert fg.info["ring_max"] == 16  # tally_reduce_kernel<16> / tally_apply<16>
    # the pass plan the reduce launched
    plan = run.tally_plan()
    if name in TC.HAND_PLANS:
        assert plan["limit"] == TC.LIMIT, f"the device reports an LDS limit of {plan['limit']} B, the plan table is for {TC.LIMIT}"
    spec = case.spec
    assert plan == TC.native_plan(exe, diag, spec.n, spec.n_edges, plan["limit"]), (name, variant, plan)
    if name in TC.HAND_PLANS and diag == TC.ALL:
        assert (plan["passes"], plan["global_mask"]) == TC.HAND_PLANS[name]
    if case.group == "ring16":
        assert plan["global_mask"] & TC.EDGE and plan["global_mask"] & TC.CUT
    # the log: granted in full, or the 64 entries of the overflow variants
    paths = run.diag_paths()
    if flags & TC.SMALL:
        assert paths["tally_log_cap"] == paths["tally_log_wanted"] == 64
    else:
        assert paths["tally_log_cap"] >= paths["tally_log_wanted"] > 64
    if case.group == "edge":
        assert paths["tally_log_wanted"] == 2 ** 23 + 2 ** 20 + 256
    _check(case, run, diag)
    run.close()
    fg.close()
