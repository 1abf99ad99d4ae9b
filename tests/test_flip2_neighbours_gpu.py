"""k = 2 flips on nodes with more (and fewer) than four neighbours, against the C oracle.

On a graph without a node of more than four neighbours flip2_kernel's segment-parallel commit
walks, for each slot, a list of the node's neighbours (their ring positions come with the graph
record: meta bits 48-63); on any other graph it walks the ring's cells, and the choice is made per
launch from the records.  The grids of test_flip_edges_gpu.py have at most four neighbours per
node (the list, padded where a node has two or three); the graphs here have two to nine, so these
cases hold the other side of that choice: k = 2 flips at nodes of five and more neighbours, next
to nodes of two and three, in 8-cell and 16-cell rings.

Every case runs on the device under the instances and commit paths a launch can take (lean / tally
/ full diagnostics; the segment pass for every acceptance, from three on, never; the band stream)
and every chain is compared with ``oracle/flipref.c`` bit for bit, on what
``test_flip_edges_gpu._check`` compares.  The CPU tests state, from the oracle's trace alone, that
each case reaches what it is for, and check the record's neighbour positions against its
neighbour bits.
"""
import functools

import networkx as nx
import numpy as np
import pytest

import flip_cases as FC
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.engine import FlipGraph
from oracle.flipref import FLAG_ACCEPTED, STREAM_BAND, STREAM_NODE
from recom_cases import strips
from test_flip_edges_gpu import FULL, LEAN, TALLY, _check, _flag, _run

LOW, HIGH = 4, 4  # degrees below LOW / above HIGH: a padded list / neighbours past the list


# ---- graphs --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def triangular():
    return G.triangular_graph(4, 6)


@functools.lru_cache(maxsize=None)
def mixed_grid():
    """5 x 6 square grid with one diagonal in every cell of the columns x < 2: degrees 2-4 on the
    plain side, up to 6 on the other, so the candidates of one wave sometimes do and sometimes do
    not exceed four neighbours."""
    g = nx.grid_graph([6, 5])  # nodes (x, y), x < 5, y < 6
    for x in range(2):
        for y in range(5):
            g.add_edge((x, y), (x + 1, y + 1))
    for nd in g.nodes():
        g.nodes[nd]["population"] = 1
    return G.from_networkx(g, pos={nd: (float(nd[0]), float(nd[1])) for nd in g.nodes()})


@functools.lru_cache(maxsize=None)
def delaunay40():
    return G.delaunay_graph(40, seed=0)


@functools.lru_cache(maxsize=None)
def delaunay_wide():
    """A Delaunay graph whose longest ring needs the 16-cell record."""
    return G.delaunay_graph(WIDE_POINTS, seed=WIDE_SEED)


WIDE_POINTS, WIDE_SEED = 60, 3

# (graph, ring_max, lowest and highest degree, needs flips at degrees below LOW)
SHAPES = {
    "triangular4x6": (triangular, 8, 2, 6, True),
    "mixed5x6": (mixed_grid, 8, 2, 6, True),
    "delaunay40": (delaunay40, 8, 3, 8, False),
    "delaunay_wide": (delaunay_wide, 16, 3, 9, False),
}


def _case(name):
    return FC.Case(name, SHAPES[name][0], 2, strips, FC.pct_bounds(0.9), FC.all_steps, bases=(1.0, 0.5, 2.0, 1.0),
                   steps=3000, launches=(1000,), n_chains=8, band=True)


CASES = [_case(n) for n in SHAPES]
for _c in CASES:  # the oracle cache of flip_cases looks its cases up by name
    assert FC.BY_NAME.setdefault(_c.name, _c) is _c

VARIANTS = {  # (diagnostics, tune, band stream)
    "lean par_min=1": (LEAN, {"par_min": 1}, False),
    "lean par_min=3": (LEAN, {"par_min": 3}, False),
    "lean par_min=65": (LEAN, {"par_min": 65}, False),
    "lean par_min=1 nsub=1": (LEAN, {"par_min": 1, "nsub": 1}, False),
    "tally par_min=1": (TALLY, {"par_min": 1}, False),
    "full par_min=1": (FULL, {"par_min": 1}, False),
    "full par_min=3": (FULL, {"par_min": 3}, False),
    "full par_min=65": (FULL, {"par_min": 65}, False),
    "band lean par_min=1": (LEAN, {"par_min": 1}, True),
    "band full par_min=3": (FULL, {"par_min": 3}, True),
}


# ---- CPU: the graphs, the record's neighbour positions, the oracle's coverage ------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_graph_shape(name):
    graph, ring_max, dlo, dhi, _ = SHAPES[name]
    spec = graph()
    fg = FlipGraph(spec)
    deg = spec.degree()
    assert fg.info["ring_max"] == ring_max
    assert fg.info["n_exact"] == spec.n  # the run rule decides every proposal: no SEARCH instance
    assert (int(deg.min()), int(deg.max())) == (dlo, dhi)
    fg.close()


def _positions_match(spec):
    fg = FlipGraph(spec)
    ring, meta = fg.rings()
    fg.close()
    for v in range(spec.n):
        m = int(meta[v])
        nbr, pos = (m >> 16) & 0xFFFF, (m >> 48) & 0xFFFF
        want = [i for i in range(16) if nbr >> i & 1]
        assert len(want) == len(spec.neighbors(v))
        assert sorted(int(ring[v][i]) for i in want) == sorted(int(u) for u in spec.neighbors(v))
        got = [(pos >> 4 * i) & 15 for i in range(4)]
        assert got == (want + [15] * 4)[:4], (v, got, want)


@pytest.mark.parametrize("name", list(SHAPES) + ["sec11"])
def test_neighbour_positions_match_neighbour_bits(name):
    _positions_match(G.sec11_graph() if name == "sec11" else SHAPES[name][0]())


def _shared_neighbour_window(spec, trace):
    """Two accepted proposals less than 64 proposals apart whose nodes have a common neighbour."""
    acc = np.nonzero((trace["flags"] & FLAG_ACCEPTED) != 0)[0]
    nb = [set(int(u) for u in spec.neighbors(v)) for v in range(spec.n)]
    for a, i in enumerate(acc):
        for j in acc[a + 1:]:
            if j - i >= FC.WINDOW:
                break
            if nb[int(trace["v"][i])] & nb[int(trace["v"][j])]:
                return True
    return False


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_reaches_the_case(case):
    spec = case.spec
    deg = spec.degree()
    for stream in (STREAM_NODE, STREAM_BAND):
        high = low = 0
        shared = False
        for c in range(case.n_chains):
            ref = case.oracle(c, stream)
            assert case.chain_ok(case, c, ref), (case.name, c)
            tr = ref["trace"]
            assert len(tr) < case.trace_cap
            d = deg[tr["v"][(tr["flags"] & FLAG_ACCEPTED) != 0]]
            high += int((d > HIGH).sum())
            low += int((d < LOW).sum())
            shared = shared or _shared_neighbour_window(spec, tr)
        assert high >= 20, (case.name, high)
        if SHAPES[case.name][4]:
            assert low >= 20, (case.name, low)
        assert shared, case.name


# ---- GPU -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", [(c.name, v) for c in CASES for v in VARIANTS])
def test_case_matches_oracle(gpu, name, variant):
    case = FC.BY_NAME[name]
    diag, tune, band = VARIANTS[variant]
    fg, run = _run(case, diag, tune, band=band)
    want = "fc::flip2_kernel<%d, %d, %s, false, %s, %s>" % (SHAPES[name][1], tune.get("nsub", 4), _flag(diag != LEAN),
                                                           _flag(diag == FULL), _flag(band))
    assert run.kernel_name() == want
    _check(case, run, diag, STREAM_BAND if band else STREAM_NODE)
    run.close()
    fg.close()
