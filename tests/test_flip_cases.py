"""The flip-kernel case table on the CPU: every case's oracle run reaches the branch the case is
for (``flip_cases.CASES`` drives the device parity test, test_flip_edges_gpu.py), and the two
trace-replay conditions count what they say on traces small enough to count by hand.
"""
import numpy as np
import pytest

import flip_cases as FC
from oracle.flipref import FLAG_ACCEPTED, FLAG_INV_CONTIG, FLAG_INV_POP, FLAG_VALID, RECORD_DTYPE, STREAM_BAND


@pytest.mark.parametrize("name", list(FC.BY_NAME))
def test_case_reaches_its_branch(name):
    """A failure here means the case is wrong (graph, bounds, bases, seed or steps), not the kernel."""
    case = FC.BY_NAME[name]
    assert 8 <= case.n_chains <= 16 and case.steps <= 3000 and case.spec.n <= 65 and case.max_draws > 0
    assert sum(case.launch_steps()) == case.steps and min(case.launch_steps()) > 0
    refs = [case.oracle(c) for c in range(case.n_chains)]
    for c, ref in enumerate(refs):
        assert case.chain_ok(case, c, ref), (name, c, ref["stats"])
        assert len(ref["trace"]) == ref["stats"]["proposals"] < case.trace_cap, (name, c)
    if case.run_ok is not None:
        assert case.run_ok(case, refs), name
    if case.band:  # the band stream's run is another trajectory: it has to end as well
        for c in range(case.n_chains):
            ref = case.oracle(c, STREAM_BAND)
            assert FC.all_steps(case, c, ref) and len(ref["trace"]) == ref["stats"]["proposals"] < case.trace_cap


def test_layout_edges_are_in_the_table():
    """The shapes the k = 2 kernel's LDS layout turns on: n < 16, n == npad == 16, n no multiple of
    16, one full 64-bit word and the first node of a second one, a graph that cannot move."""
    sizes = {c.spec.n for c in FC.K2_CASES}
    assert {2, 3, 5, 9, 16, 17, 63, 64, 65} <= sizes
    assert all(c.k == 2 and not c.pair for c in FC.K2_CASES) and all(c.k > 2 and c.pair for c in FC.PAIR_CASES)
    assert FC.BY_NAME["all_accept"].launch_steps()[:5] == [1, 2, 63, 64, 65]
    heavy = FC.BY_NAME["grid4x4_heavy"].spec.pop.astype(np.int64)
    assert int(heavy.sum()) == 2 ** 31 - 16 and FC.BY_NAME["grid4x4_heavy"].chain_bounds(0)[1] < 2 ** 31
    assert len(set(FC.BY_NAME["grid9x7_weighted"].spec.pop.tolist())) > 20


def test_outer_face_is_the_grid_hull():
    """The graph builder's outer-face flags on a grid are its hull, so a district leaves the outer
    face exactly when it holds inner nodes only."""
    for gx, gy in ((3, 3), (4, 4), (9, 7)):
        spec = FC.grid(gx, gy)
        mx, my = (max(nd[i] for nd in spec.nodes) for i in (0, 1))
        hull = np.asarray([x in (0, mx) or y in (0, my) for x, y in spec.nodes])
        assert 0 < (~hull).sum() == (gx - 2) * (gy - 2)
        assert np.array_equal(FC.gamma_nodes(FC.BY_NAME["grid%dx%d" % (gx, gy)].graph), hull)


def _trace(rows):
    tr = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for j, (v, target, flags) in enumerate(rows):
        tr[j]["v"] = v
        tr[j]["flags"] = flags | (target << 8)
    return tr


VA = FLAG_VALID | FLAG_ACCEPTED


def test_pop_verdict_flips_on_a_hand_made_trace():
    """Four nodes of populations 1, 2, 3, 4, districts {0, 1} | {2, 3} (populations 3 | 7), bounds
    1 .. 9.  Proposal 0 moves node 1 (accepted: 1 | 9).  Proposal 1 moves node 0: 0 | 10 is out of
    bounds, but against the populations before proposal 0 it is 2 | 8: a flipped verdict.
    Proposal 2 (node 2 back, valid either way) and 3 (flagged for contiguity: not judged) do not
    count.  Proposal 4 moves node 1 back (accepted: 3 | 7); proposal 5 moves node 0, valid at
    2 | 8, out of bounds against the populations before proposal 4: the second flipped verdict."""
    pop, init = [1, 2, 3, 4], [0, 0, 1, 1]
    tr = _trace([(1, 1, VA), (0, 1, FLAG_INV_POP), (2, 0, FLAG_VALID), (3, 0, FLAG_INV_CONTIG), (1, 0, VA),
                 (0, 1, FLAG_VALID)])
    r = FC.replay(np.asarray(pop), 2, init, tr)
    assert r["pops"].tolist() == [[3, 7], [1, 9], [1, 9], [1, 9], [1, 9], [3, 7]]
    assert r["A"].tolist() == [0, 0, 1, 1, 1, 0] and r["states"].tolist() == [[0, 0, 1, 1], [0, 1, 1, 1], [0, 0, 1, 1]]
    assert FC.pop_verdict_flips(pop, 2, init, tr, 1, 9) == 2
    assert FC.pop_verdict_flips(pop, 2, init, tr, 1, 9, window=2) == 2  # both one proposal after their flip
    assert FC.pop_verdict_flips(pop, 2, init, tr, 1, 9, window=1) == 0  # j - 1 < i < j: no i
    # proposal 4 not accepted: proposal 5 is then out of bounds (0 | 10), and only proposal 0, five
    # proposals back, gives the other verdict: inside a window of 6, outside one of 5
    tr2 = _trace([(1, 1, VA), (0, 1, FLAG_INV_POP), (2, 0, FLAG_VALID), (3, 0, FLAG_INV_CONTIG), (1, 0, FLAG_VALID),
                  (0, 1, FLAG_INV_POP)])
    assert FC.pop_verdict_flips(pop, 2, init, tr2, 1, 9, window=6) == 2
    assert FC.pop_verdict_flips(pop, 2, init, tr2, 1, 9, window=5) == 1


def test_outer_face_moves_on_a_hand_made_trace():
    """Nodes 0 and 3 on the outer face, districts {0, 1} | {2, 3}.  Proposal 0 moves node 0: district
    0 = {1} has left the outer face (1 leave).  Proposals 1 (not accepted) and 2 (node 2, inner)
    change no count.  Proposal 3 moves node 3 to district 0: it is back (1 regain).  Proposal 4 is
    invalid.  Proposal 5 moves node 0 to district 0: district 1 = {} has left (2 leaves)."""
    gamma = np.asarray([True, False, False, True])
    tr = _trace([(0, 1, VA), (2, 0, FLAG_VALID), (2, 0, VA), (3, 0, VA), (0, 0, FLAG_INV_CONTIG), (0, 0, VA)])
    assert FC.outer_face_moves(gamma, 2, [0, 0, 1, 1], tr) == (2, 1)
    assert FC.outer_face_moves(gamma, 2, [0, 0, 1, 1], tr[:3]) == (1, 0)
    assert FC.outer_face_moves(~gamma, 2, [0, 0, 1, 1], tr) == (1, 0)  # nodes 1, 2: proposal 2 empties district 1's
