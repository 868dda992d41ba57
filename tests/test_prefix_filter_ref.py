"""The prefix-row filter on the oracle's full matrices (no GPU): the lemma itself — every cell that holds the
maximum B crosses row P within W columns and above B - smax (m - P) —, its sharpness, and the two locate rounds of the host emulated
with the sampled prefix values of tests/row_sampled_fold.py: the evaluated sub-chunks hold every cell that holds B.  The offender
counts that tests/test_gpu_prefix_filter.py asserts on the device come from the same emulation (tests/prefix_filter.py)."""
import numpy as np
import pytest

from oracle import binding as ob
from prefix_filter import LANES, bound, covers, emulate, geometry
from row_sampled_fold import SUB, slack

R = 19
P = LANES * R                                                        # 38 rows
SCORINGS = [(3.0, -3.0, 2.0), (2.0, -3.0, 5.0), (5.0, -4.0, 1.0)]
CAP = 64 + 1024 // 8                                                 # query_flag_cap of a batch of eight reads


def _dna(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def _mutate(rng, x, lo, hi, k):
    """k substitutions at distinct places of x[lo:hi]."""
    x = bytearray(x)
    for at in rng.choice(np.arange(lo, hi), k, replace=False):
        x[at] = b"ACGT"[(b"ACGT".index(x[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(x)


def _cases(rng, m, n):
    """(name, read, reference): planted copies in a random reference of n columns."""
    y = _dna(rng, n)
    at = 5 * SUB + 100
    copy = y[at:at + m]
    out = [("exact", copy, y),
           ("errors", _mutate(rng, copy, 0, m, max(1, m // 20)), y),
           ("prefix_errors", _mutate(rng, copy, 0, P, 6), y),          # a low prefix value at the true locus
           ("first_columns", y[:m], y),
           ("last_columns", y[n - m:], y)]
    # the prefix rows end in sub-chunk c, the end cell behind a long insertion of the reference in c + 1
    c_end = 4 * SUB - 2
    ins = _dna(rng, 24)
    y2 = y[:c_end] + ins + y[c_end:]
    out.append(("insertion", y[c_end - P - 4:c_end] + y[c_end:c_end + m - P - 4], y2))
    # two equal copies (the first wins), and a third one score unit lower is impossible at these scorings' steps: one mismatch lower
    y3 = bytearray(y)
    y3[9 * SUB + 7:9 * SUB + 7 + m] = copy
    out.append(("two_copies", copy, bytes(y3)))
    out.append(("random", _dna(rng, m), y))
    return out


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "%g_%g_%g" % s)
@pytest.mark.parametrize("m", [60, 150])
def test_lemma_and_rounds(m, scoring):
    match, mismatch, gap = scoring
    rng = np.random.default_rng(190 + m + int(10 * match))
    n = int(rng.integers(2600, 4000))
    _, W, D = geometry(m, R, match, gap)
    certified = 0
    for name, x, y in _cases(rng, m, n):
        H = ob.fill(x, y, ob.F32, match, mismatch, gap).astype(np.float64)
        assert np.array_equal(ob.fill(x[:P], y, ob.F32, match, mismatch, gap), H[:P + 1].astype(np.float32)), "the first P rows are the prefix's matrix"
        B = float(H.max())
        cells = np.argwhere(H == B)
        if B > match * (m - P):
            for i, j in cells:
                if i <= P:
                    continue                                         # a cell of the prefix matrix itself
                lo = max(0, j - W)
                assert H[P, lo:j + 1].max() >= B - match * (i - P), (name, m, scoring, int(i), int(j))
        e = emulate(x, y, R, match, mismatch, gap, CAP)
        assert e["B0"] <= B
        if name == "random" and scoring == SCORINGS[0] and m == 150:
            assert e["offender"], (m, scoring)                       # (cheap gaps let a random read score above the bound: then it certifies)
        if e["offender"]:
            assert e["B0"] <= bound(m, R, match, gap) or e["why"] == "over the cap", (name, e["why"])
            continue
        certified += 1
        for i, j in cells:
            assert covers(e["evaluated"], int(j) - 1), (name, m, scoring, int(i), int(j), e["evaluated"])
        first = min((int(j), int(i)) for i, j in cells)
        assert e["result"] == (B, first[1], first[0]), (name, m, scoring, e["result"], B, first)
    # the planted copies certify wherever the rule can certify at all
    if match * m > bound(m, R, match, gap):
        assert certified >= 5, (m, scoring, certified)


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "%g_%g_%g" % s)
def test_bound_is_sharp(scoring):
    """A copy whose first P rows are letters the reference does not hold scores exactly smax (m - P): an offender by the rule, and one
    more matching row certifies nothing either (the slack); with random letters instead the copy still cannot certify."""
    match, mismatch, gap = scoring
    m = 150
    rng = np.random.default_rng(77 + int(match))
    y = _dna(rng, 3000)
    at = 1500
    x = b"N" * P + y[at + P:at + m]
    H = ob.fill(x, y, ob.F32, match, mismatch, gap)
    assert float(H.max()) == match * (m - P)
    assert emulate(x, y, R, match, mismatch, gap, CAP)["offender"]
    x = _dna(rng, P) + y[at + P:at + m]
    e = emulate(x, y, R, match, mismatch, gap, CAP)
    B = float(ob.fill(x, y, ob.F32, match, mismatch, gap).max())
    assert e["offender"] or all(covers(e["evaluated"], int(j) - 1) for j in np.flatnonzero(ob.fill(x, y, ob.F32, match, mismatch, gap).max(axis=0) == B))
    assert slack(R, gap) == 7 * gap


def test_end_cell_in_the_second_right_neighbour():
    """5 / -4 / 1, m = 150: the prefix rows end in the last columns of sub-chunk c and the other rows follow 150 inserted columns, so
    the end cell lies in c + 2 and B = 750 - 150 = 600 is above the bound 567: the read certifies, and only the second right
    neighbour of its prefix sub-chunk holds the maximum.  (Reference over A / C, read over G / T: the threshold 33 flags nothing else.)"""
    match, mismatch, gap = 5.0, -4.0, 1.0
    m, c = 150, 4
    rng = np.random.default_rng(5)
    n = 12 * SUB + 40
    y = bytearray(rng.choice(list(b"AC"), n).astype(np.uint8))
    x = bytes(rng.choice(list(b"GT"), m).astype(np.uint8))
    cut = (c + 1) * SUB - 3
    y[cut - (P + 2):cut] = x[:P + 2]
    y[cut + 150:cut + 150 + m - P - 2] = x[P + 2:]
    y = bytes(y)
    H = ob.fill(x, y, ob.F32, match, mismatch, gap)
    B = float(H.max())
    cells = np.argwhere(H == B)
    assert B == 600 and B > bound(m, R, match, gap) == 567
    assert {(int(j) - 1) // SUB for _, j in cells} == {c + 2}
    _, W, D = geometry(m, R, match, gap)
    assert D >= 2
    for i, j in cells:
        assert H[P, max(0, j - W):j + 1].max() >= B - match * (i - P)
    e = emulate(x, y, R, match, mismatch, gap, CAP)
    assert not e["offender"] and int(np.flatnonzero(e["values"] == e["values"].max())[0]) == c
    assert c + 2 in e["evaluated"] and e["result"] == (B, int(cells[0][0]), int(cells[0][1])), e
