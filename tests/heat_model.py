"""Host model of the heat-map series (include/flipchain.h ``fc_run_heat_series``),
computed from the **list of per-yield states** and nothing else: no event, no lazy sum.  Every
output is evaluated by its definition at every yield of the window, one yield after the other, in
Python integers -- the style of tests/recom_log_model.py, whose ``states`` and ``cut_nb`` feed it.

tests/test_heat.py checks this model against the C oracle's fused tallies on flip trajectories and
by hand on a burst; tests/test_heat_gpu.py checks the device against it.
"""
import numpy as np

KEYS = ("cut_hist", "nb_hist", "cut_times", "moves", "last_move", "dwell")


def heat(S, t0, edges_uv, k, cut, nb, nb_width):
    """fc_run_heat_series of one chain whose window's yields t0, t0 + 1, ... have the states S
    (``cut`` / ``nb``: |cut| and |B| per state; ``edges_uv`` the canonical edge list)."""
    uv = np.asarray(edges_uv, dtype=np.int64).reshape(-1, 2)
    n, E = S[0].size, uv.shape[0]
    cut_hist, nb_hist = [0] * (E + 1), [0] * nb_width
    cut_times, moves, last_move = [0] * E, [0] * n, [0] * n
    dwell = [[0] * k for _ in range(n)]
    for i, a in enumerate(S):
        cut_hist[int(cut[i])] += 1
        nb_hist[int(nb[i])] += 1
        for e in range(E):
            if a[uv[e, 0]] != a[uv[e, 1]]:
                cut_times[e] += 1
        for u in range(n):
            dwell[u][int(a[u])] += 1
            if i > 0 and a[u] != S[i - 1][u]:
                moves[u] += 1
                last_move[u] = t0 + i
    i64 = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    return {"yields": len(S), "cut_hist": i64(cut_hist), "nb_hist": i64(nb_hist), "cut_times": i64(cut_times),
            "moves": i64(moves), "last_move": i64(last_move), "dwell": i64(dwell).reshape(n, k)}


def occupancy(dwell, labels):
    """sum_d labels[d] dwell[u][d]: the time integral of every node's label."""
    return np.asarray(dwell, dtype=np.int64) @ np.asarray(labels, dtype=np.int64)


def assert_matches(got, i, want, keys=KEYS):
    """Chain ``i`` of a ``FlipRun.heat_series`` result against a model, bit for bit."""
    for key in keys:
        assert got[key][i].dtype == np.int64 and got[key][i].shape == want[key].shape, (i, key)
        assert np.array_equal(got[key][i], want[key]), (i, key)
    assert int(got["yields"][i]) == want["yields"], i


def moved_edge_ends(S, edges_uv):
    """Yields at which both ends of some edge changed district."""
    uv = np.asarray(edges_uv, dtype=np.int64).reshape(-1, 2)
    out = 0
    for i in range(1, len(S)):
        ch = S[i] != S[i - 1]
        out += int((ch[uv[:, 0]] & ch[uv[:, 1]]).any())
    return out


def flipped_back(S):
    """Nodes that leave a district and are back in it at a later yield."""
    A = np.asarray(S)
    out = 0
    for u in range(A.shape[1]):
        col = A[:, u]
        runs = col[np.r_[True, col[1:] != col[:-1]]]  # the districts u is in, one entry per stay
        out += int(len(set(runs.tolist())) < runs.size)
    return out
