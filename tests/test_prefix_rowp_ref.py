"""The row-P variant of the prefix filter on the oracle's full matrices (no GPU), for the prefix heights R = 13, 16
and 19 (P = 26, 32, 38): with the tiles folding row P alone the threshold loses the row term of the slack, B0 - smax (m - P) - (MK - 1) g,
and a read must also score above smax P.  The two locate rounds are emulated on the row-P values (tests/prefix_rowp.py); the
references are 200 k columns, as in tests/test_gpu_prefix_filter.py."""
import numpy as np
import pytest

from oracle import binding as ob
from prefix_filter import covers
from prefix_rowp import LANES, bound, emulate, geometry, rowp_values, slack
from row_sampled_fold import MK, SUB

HEIGHTS = [13, 16, 19]
M = 150
N = 200_000 + 77
SCORING = (3.0, -3.0, 2.0)
CAP = 64 + 1024 // 8


def _dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(list(letters), n).astype(np.uint8))


def _mutate(rng, x, lo, hi, k):
    x = bytearray(x)
    for at in rng.choice(np.arange(lo, hi), k, replace=False):
        x[at] = b"ACGT"[(b"ACGT".index(x[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(x)


def _truth(x, y, scoring):
    """(B, cells holding B as (i, j), 1-based) of the oracle's full matrix."""
    H = ob.fill(x, y, ob.F32, *scoring)
    B = float(H.max())
    return B, [(int(i), int(j)) for i, j in np.argwhere(H == B)], H


@pytest.fixture(scope="module")
def main_case():
    rng = np.random.default_rng(3107)
    y = bytearray(_dna(rng, N))
    copy = lambda o, m=M: bytes(y[o:o + m])
    two = copy(700 * SUB + 5)
    y[90 * SUB + 99:90 * SUB + 99 + M] = two                             # an equal copy further left: it wins
    reads = dict(exact=copy(40 * SUB + 17),
                 errors=_mutate(rng, copy(333 * SUB + 200), 0, M, 5),
                 prefix_errors=_mutate(rng, copy(500 * SUB + 60), 0, LANES * HEIGHTS[0], 4),   # confined to the first P rows of every height
                 first_columns=copy(0), last_columns=copy(N - M), two_copies=two, random=_dna(rng, M))
    y = bytes(y)
    truth = {}
    for name, x in reads.items():
        B, cells, H = _truth(x, y, SCORING)
        truth[name] = (B, cells, {R: H[LANES * R].astype(np.float64) for R in HEIGHTS})
    return reads, y, truth


@pytest.mark.parametrize("R", HEIGHTS)
def test_lemma_and_rounds(main_case, R):
    reads, y, truth = main_case
    match, mismatch, gap = SCORING
    P, W, D = geometry(M, R, match, gap)
    assert slack(gap) == (MK - 1) * gap == 6 and bound(M, R, match, gap) == match * (M - P) + 6
    for name, x in reads.items():
        B, cells, rows = truth[name]
        val = rowp_values(x, y, R, match, mismatch, gap)
        if B > bound(M, R, match, gap):
            for i, j in cells:
                # the lemma: row P holds >= B - smax (i - P) within W columns left of the end cell, and the fold sees it within the slack
                assert i > P and rows[R][max(0, j - W):j + 1].max() >= B - match * (i - P), (name, R, i, j)
                c = max(0, j - W) + int(np.argmax(rows[R][max(0, j - W):j + 1]))          # 1-based column of such a crossing
                s = (c - 1) // SUB
                assert val[s:s + 2].max() >= B - match * (M - P) - slack(gap), (name, R, i, j, c)
        e = emulate(x, y, R, match, mismatch, gap, CAP)
        assert e["B0"] <= B
        print("R=%d %-14s B=%g offender=%d %s evaluated=%s" % (R, name, B, e["offender"], e["why"], e["evaluated"][:6]))
        assert e["offender"] == (name == "random"), (name, R, e["why"], e["B0"])
        if e["offender"]:
            assert e["B0"] <= bound(M, R, match, gap)
            continue
        for i, j in cells:
            assert covers(e["evaluated"], j - 1), (name, R, i, j, e["evaluated"])
        first = min((j, i) for i, j in cells)
        assert e["result"] == (B, first[1], first[0]), (name, R, e["result"], B, first)


@pytest.fixture(scope="module")
def two_letter_case():
    """Reference over A / C, reads over G / T (prefix values are zero away from the planted copies): per height one read whose copy
    scores bound + 1 (one inserted column below row P: 3 k - 2) and one that scores the bound exactly (3 k)."""
    rng = np.random.default_rng(4211)
    y = bytearray(_dna(rng, N, b"AC"))
    reads = {}
    for h, R in enumerate(HEIGHTS):
        b = int(bound(M, R, 3.0, 2.0))
        assert b % 3 == 0
        k = (b + 3) // 3                                                 # 3 k - 2 = bound + 1
        above = _dna(rng, k, b"GT")
        at = (100 + 80 * h) * SUB + 9
        y[at:at + k + 1] = above[:70] + b"A" + above[70:]
        equal = _dna(rng, b // 3, b"GT")
        at = (130 + 80 * h) * SUB + 40
        y[at:at + len(equal)] = equal
        reads[R] = (above + b"N" * (M - k), equal + b"N" * (M - len(equal)))
    return reads, bytes(y)


@pytest.mark.parametrize("R", HEIGHTS)
def test_reads_at_the_bound(two_letter_case, R):
    reads, y = two_letter_case
    b = bound(M, R, 3.0, 2.0)
    above, equal = reads[R]
    B, cells, _ = _truth(above, y, SCORING)
    assert B == b + 1
    e = emulate(above, y, R, *SCORING, CAP)
    assert not e["offender"] and e["result"][0] == B and all(covers(e["evaluated"], j - 1) for _, j in cells), e
    B, _, _ = _truth(equal, y, SCORING)
    assert B == b
    e = emulate(equal, y, R, *SCORING, CAP)
    assert e["offender"] and e["why"] == "B0 cannot certify" and e["B0"] == b, e


@pytest.mark.parametrize("R", HEIGHTS)
def test_end_cell_right_of_the_crossing(R):
    """5 / -4 / 1: the first P + 2 rows end in the last columns of sub-chunk c, the other rows follow an insertion as long as the bound
    lets the read certify (at most 150 columns): the end cell lies that far right of its crossing of row P, within W — in sub-chunk
    c + 2 at P = 32 and 38; at P = 26 the bound leaves no read of this length an insertion that long, and it is c + 1."""
    scoring = (5.0, -4.0, 1.0)
    match, mismatch, gap = scoring
    P, W, D = geometry(M, R, match, gap)
    c = 300
    rng = np.random.default_rng(99 + R)
    y = bytearray(_dna(rng, N, b"AC"))
    x = _dna(rng, M, b"GT")
    ins = int(min(150, match * M - bound(M, R, match, gap) - 1))
    cut = (c + 1) * SUB - 3
    y[cut - (P + 2):cut] = x[:P + 2]
    y[cut + ins:cut + ins + M - P - 2] = x[P + 2:]
    y = bytes(y)
    B, cells, H = _truth(x, y, scoring)
    assert B == match * M - ins > bound(M, R, match, gap) and len(cells) == 1
    i, j = cells[0]
    crossing = cut - 2                                                   # (1-based) the path's cell in row P: P matches so far
    assert H[P, crossing] == match * P >= B - match * (M - P) and j - crossing == M - P + ins
    assert (crossing - 1) // SUB == c and 0 < j - crossing <= W and D >= 2
    assert (j - 1) // SUB == (c + 2 if R > 13 else c + 1)
    e = emulate(x, y, R, match, mismatch, gap, CAP)
    assert not e["offender"] and int(np.flatnonzero(e["values"] == e["values"].max())[0]) in (c, c + 1), e["why"]
    assert (j - 1) // SUB in e["evaluated"] and e["result"] == (B, i, j), e


@pytest.mark.parametrize("R", HEIGHTS)
def test_short_read_that_ends_in_the_prefix(R):
    """P < m < 2 P: the bound is smax P.  A read whose best alignment ends above row P (its first P - 2 letters are a copy, the rest
    matches nothing) shows nothing in row P that the rule could trust: B <= smax P makes it an offender, never a wrong result.  The
    whole copy of the same length ends below row P and certifies."""
    match, mismatch, gap = SCORING
    P = LANES * R
    m = P + 10
    assert P < m < 2 * P and bound(m, R, match, gap) == match * P > match * (m - P) + slack(gap)
    rng = np.random.default_rng(7 + R)
    y = _dna(rng, N)
    at = 410 * SUB + 33
    x = y[at:at + P - 2] + b"N" * (m - P + 2)
    B, cells, _ = _truth(x, y, SCORING)
    assert B == match * (P - 2) and all(i < P for i, _ in cells)
    e = emulate(x, y, R, match, mismatch, gap, CAP)
    assert e["offender"] and e["why"] in ("B0 cannot certify", "no prefix value"), e
    x = y[at:at + m]
    B, cells, _ = _truth(x, y, SCORING)
    e = emulate(x, y, R, match, mismatch, gap, CAP)
    assert B == match * m and not e["offender"] and e["result"] == (B, cells[0][0], cells[0][1]), e
