"""Replica exchange, the parts that need no GPU (DESIGN.md "Replica exchange"): the swap
threshold ``fc_ladder_swap_threshold`` (the one definition of a decision's bits, the code the
device runs) against ``math.pow``; the host model on the GPU test's configuration; and the sharding
of ladders over ranks."""
import itertools
import math

import numpy as np

import tempering_model as TM
from flipcomplexityempirical_amd import graphs as G
from flipcomplexityempirical_amd.distributed import shard_ladders
from flipcomplexityempirical_amd.tempering import geometric_ladder, swap_threshold

TWO53 = 1 << 53
BASES = sorted(set(G.SEC11_BASES + G.FRANK_BASES))
D_MAX = 3120  # sec11's edge count: every |cut| difference the GPU tests can meet


def test_swap_threshold_against_pow():
    """|t - p 2^53| <= 1 + 64 ulp: at most 17 factors pow(qq, 2^j) of <= 1 ulp each, at most 16
    roundings of the products (1/2 ulp each), the reference's own ulp, with margin; the 1 is the
    ceil.  The reference is math.pow(qq, |d|) of the same double qq = min(b) / max(b)."""
    for b0, b1 in itertools.permutations(BASES, 2):
        qq = min(b0, b1) / max(b0, b1)
        unfav = 1 if b0 < b1 else -1
        prev = TWO53
        for a in range(1, D_MAX + 1):
            t = swap_threshold(b0, b1, unfav * a)
            ref = math.pow(qq, a) * TWO53
            assert abs(t - ref) <= 1 + 64 * 2.0 ** -53 * ref, (b0, b1, a, t, ref)
            assert t <= prev, (b0, b1, a)  # non-increasing in |d| on the unfavourable side
            prev = t
            assert swap_threshold(b0, b1, -unfav * a) == TWO53  # favourable: always swaps
        assert swap_threshold(b0, b1, 0) == TWO53


def test_swap_threshold_equal_bases_and_limits():
    for b in BASES:
        for d in (-D_MAX, -7, -1, 0, 1, 7, D_MAX):
            assert swap_threshold(b, b, d) == TWO53
    # the product is cut to 0 once below 2^-64 (no denormal is formed); |d| < 2^17
    assert swap_threshold(.1, 10, 40) == 0
    assert swap_threshold(10, .1, -(2 ** 17 - 1)) == 0
    for bad in ((0.0, 1.0, 1), (1.0, -2.0, 1), (1.0, float("inf"), 1), (1.0, 2.0, 2 ** 17)):
        try:
            swap_threshold(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_geometric_ladder():
    lad = geometric_ladder(1.0, 10.0, 5)
    assert lad[0] == 1.0 and lad[-1] == 10.0 and np.allclose(lad[1:] / lad[:-1], 10 ** .25)
    assert list(geometric_ladder(2.0, 3.0, 1)) == [2.0]


def test_model_alone_on_the_gpu_configuration(cref, sec11):
    """The model of tests/test_tempering_gpu.py's whole-run case: rung maps stay permutations, and
    the swap decisions that depend on the uniform (0 < t < 2^53) go both ways at least 10 times,
    so the device test compares real decisions."""
    case, m, snaps = TM.sec11_reference(cref, sec11, swap_threshold)
    assert len(snaps) == TM.SEC11_ROUNDS
    for snap in snaps:
        for lad, at in zip(case["ladders"], snap["chain_at"]):
            assert sorted(at) == sorted(lad)
            for r, c in enumerate(at):
                assert snap["rung_of"][c] == r
        assert all(snap["rung_of"][c] == -1 for c in case["free"])
    open_dec = [d for d in m.decisions if 0 < d[4] < TWO53]
    acc = sum(1 for d in open_dec if d[6])
    assert acc >= 10 and len(open_dec) - acc >= 10, (acc, len(open_dec))
    # every slot's steps: rounds x steps, whoever held it
    for l, lad in enumerate(case["ladders"]):
        for r in range(len(lad)):
            assert m.rung[l][r]["steps"] == TM.SEC11_ROUNDS * TM.SEC11_STEPS
            assert m.rung_cut_hist[l][r].sum() == TM.SEC11_ROUNDS * TM.SEC11_STEPS + 1
    # the sums of a ladder's slots are the sums of its chains
    for l, lad in enumerate(case["ladders"]):
        for f in TM.FIELDS:
            assert sum(rg[f] for rg in m.rung[l]) == sum(m.chain[c][f] for c in lad), f


def test_shard_ladders():
    sizes = [5, 8, 2, 1, 4, 4, 4, 7, 3]
    start = np.concatenate([[0], np.cumsum(sizes)])
    for world in (1, 2, 3, 4, 9, 16):
        seen, nxt = [], 0
        for rank in range(world):
            lo, cnt, off, nch = shard_ladders(sizes, world, rank)
            assert lo == nxt and off == start[lo] and nch == start[lo + cnt] - start[lo]  # whole ladders, contiguous
            seen += list(range(lo, lo + cnt))
            nxt = lo + cnt
        assert seen == list(range(len(sizes)))  # every ladder once, for any world size
    for bad in ((sizes, 0, 0), (sizes, 2, 2), ([], 1, 0), ([3, 0], 1, 0)):
        try:
            shard_ladders(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)
