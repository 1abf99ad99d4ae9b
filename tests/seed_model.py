"""Plain Python restatement of the seed-plan definition (include/flipchain.h fc_graph_seed_plans,
DESIGN.md §5i): the reference of test_seed_cases.py (CPU) and test_seed_gpu.py (the device equals
it bit for bit).  Kruskal, DFS subtree sums and linear scans; no code shared with the product.
``bipartition`` is the ReCom oracle's bipartition_tree (oracle/recomref.c) with the cut test as an
argument, which test_seed_cases.py holds against the oracle's trace.
"""
import numpy as np

from oracle.flipref import philox4x32_10

M64 = (1 << 64) - 1
DEFAULTS = {"node_repeats": 1, "max_attempts": 256, "max_restarts": 16}


def _splitmix64(x):
    """splitmix64 of a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _words(d, gid, purpose, seed):
    w = philox4x32_10(d & 0xFFFFFFFF, d >> 32, gid, purpose, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [int(x) for x in w]


def _mulhi64(r, n):
    return (r * n) >> 64


def edge_list(spec):
    """Canonical edges (u < v, CSR order), as recomref.c builds them."""
    e = spec.edges()
    return e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)


def bipartition(spec, in_M, d, gid, seed, node_repeats, max_attempts, is_cut, edges=None):
    """bipartition_tree on the node subset ``in_M`` (bool [n]) with draw index ``d``, chain word
    ``gid`` and key ``seed``; ``is_cut(s)`` is the cut test of a subtree population.  Returns
    ``attempts``, ``trees``, ``root``, ``child`` (-1: no cut within ``max_attempts``), the
    subtree's population ``pop`` and its nodes ``subset`` (bool [n])."""
    n = spec.n
    eu, ev = edge_list(spec) if edges is None else edges
    pop = spec.pop.astype(np.int64)
    inside = np.nonzero(in_M[eu] & in_M[ev])[0]
    tree = -1
    trees = attempts = 0
    root = child = -1
    adj = None
    while attempts < max_attempts:
        t = attempts
        attempts += 1
        if t // node_repeats != tree:  # a new maximum spanning tree of random weights (Kruskal)
            tree = t // node_repeats
            trees += 1
            kw = _words(d, gid, 0x80000000 | tree, seed)
            key = ((kw[1] << 32) | kw[0]) & M64
            with np.errstate(over="ignore"):
                wts = _splitmix64(np.uint64(key) + inside.astype(np.uint64)) >> np.uint64(32)
            order = inside[np.lexsort((inside, -wts.astype(np.int64)))]  # weight descending, edge id ascending
            uf = list(range(n))

            def find(x):
                while uf[x] != x:
                    uf[x] = uf[uf[x]]
                    x = uf[x]
                return x
            adj = [[] for _ in range(n)]
            for e in order:
                u, v = int(eu[e]), int(ev[e])
                x, y = find(u), find(v)
                if x == y:
                    continue
                uf[x] = y
                adj[u].append(v)
                adj[v].append(u)
        cw = _words(d, gid, 0x40000000 | t, seed)
        inner = [x for x in range(n) if in_M[x] and len(adj[x]) > 1]
        if not inner:
            continue
        root = inner[_mulhi64((cw[1] << 32) | cw[0], len(inner))]
        # subtree populations: DFS order from the root, children before parents
        parent = {root: -1}
        order, stack = [], [root]
        while stack:
            x = stack.pop()
            order.append(x)
            for y in adj[x]:
                if y != parent[x]:
                    parent[y] = x
                    stack.append(y)
        spop = {x: int(pop[x]) for x in order}
        for x in reversed(order[1:]):
            spop[parent[x]] += spop[x]
        cuts = [x for x in range(n) if in_M[x] and x != root and x in spop and is_cut(spop[x])]
        if not cuts:
            continue
        child = cuts[_mulhi64((cw[3] << 32) | cw[2], len(cuts))]
        subset = np.zeros(n, dtype=bool)
        stack = [child]
        subset[child] = True
        while stack:
            x = stack.pop()
            for y in adj[x]:
                if y != parent[x] and not subset[y]:
                    subset[y] = True
                    stack.append(y)
        return {"attempts": attempts, "trees": trees, "root": root, "child": child, "pop": spop[child],
                "subset": subset}
    return {"attempts": attempts, "trees": trees, "root": root, "child": -1, "pop": 0, "subset": None}


def seed_plan(spec, k, lo, hi, seed, G, node_repeats=0, max_attempts=0, max_restarts=0, edges=None):
    """Plan ``G``: ``assign`` (int8 [n]; -1 everywhere when it failed) and the per-plan record
    ``attempts``, ``trees``, ``restarts``, ``ok``, ``cut``, ``nb``."""
    node_repeats = node_repeats or DEFAULTS["node_repeats"]
    max_attempts = max_attempts or DEFAULTS["max_attempts"]
    max_restarts = max_restarts or DEFAULTS["max_restarts"]
    n = spec.n
    edges = edge_list(spec) if edges is None else edges
    pop = spec.pop.astype(np.int64)
    attempts = trees = 0
    for r in range(max_restarts + 1):
        a = np.full(n, k - 1, dtype=np.int8)
        pop_m = int(pop.sum())
        done = True
        for i in range(k - 1):
            m = k - 1 - i
            in_m = a == k - 1

            def is_cut(s, m=m, pop_m=pop_m):
                return lo <= s <= hi and m * lo <= pop_m - s <= m * hi
            b = bipartition(spec, in_m, 0xFFFFFFFF00000000 | (r << 8) | i, G, seed, node_repeats, max_attempts,
                            is_cut, edges)
            attempts += b["attempts"]
            trees += b["trees"]
            if b["child"] < 0:
                done = False
                break
            a[b["subset"]] = i
            pop_m -= b["pop"]
        if done:
            eu, ev = edges
            cut_mask = a[eu] != a[ev]
            on_cut = np.zeros(n, dtype=bool)
            on_cut[eu[cut_mask]] = True
            on_cut[ev[cut_mask]] = True
            return {"assign": a, "attempts": attempts, "trees": trees, "restarts": r, "ok": 1,
                    "cut": int(cut_mask.sum()), "nb": int(on_cut.sum())}
    return {"assign": np.full(n, -1, dtype=np.int8), "attempts": attempts, "trees": trees, "restarts": max_restarts,
            "ok": 0, "cut": 0, "nb": 0}


def seed_plans(spec, k, lo, hi, seed, n_plans, plan_id_offset=0, **kw):
    edges = edge_list(spec)
    return [seed_plan(spec, k, lo, hi, seed, plan_id_offset + i, edges=edges, **kw) for i in range(n_plans)]
