"""The prefix filter with row P folded at every step (DESIGN.md §3.3 L19, row-P variant with MK = 1: no slack) on the oracle's full
matrices (no GPU), for P = 26, 32 and 38, and the rule by which a chained bucket picks its start height and sends offenders to ONE
taller pass (tests/prefix_cascade.py emulate_chain) on counted examples."""
import numpy as np
import pytest

from oracle import binding as ob
from prefix_cascade import LANES, PROBE, Read, bound, emulate_chain, geometry, slack, start_height
from prefix_filter import covers
from row_sampled_fold import SUB

HEIGHTS = [13, 16, 19]
M = 150
N = 60_000 + 77
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
    """(B, cells holding B as (i, j), 1-based, matrix) of the oracle's full matrix."""
    H = ob.fill(x, y, ob.F32, *scoring)
    B = float(H.max())
    return B, [(int(i), int(j)) for i, j in np.argwhere(H == B)], H


@pytest.fixture(scope="module")
def main_case():
    rng = np.random.default_rng(5107)
    y = bytearray(_dna(rng, N))
    copy = lambda o, m=M: bytes(y[o:o + m])
    two = copy(170 * SUB + 5)
    y[90 * SUB + 99:90 * SUB + 99 + M] = two                             # an equal copy further left: it wins
    reads = dict(exact=copy(40 * SUB + 17), errors=_mutate(rng, copy(133 * SUB + 200), 0, M, 5),
                 late_errors=_mutate(rng, copy(200 * SUB + 60), 40, M, 11),   # deficit about 66: a threshold the background reaches too often at the lower heights
                 first_columns=copy(0), last_columns=copy(N - M), two_copies=two, random=_dna(rng, M))
    y = bytes(y)
    out = {}
    for name, x in reads.items():
        B, cells, H = _truth(x, y, SCORING)
        out[name] = (Read(x, y, SCORING, HEIGHTS), B, cells, {R: H[LANES * R].astype(np.float64) for R in HEIGHTS})
    return out


@pytest.mark.parametrize("R", HEIGHTS)
def test_lemma_and_rounds_without_slack(main_case, R):
    match, mismatch, gap = SCORING
    P, W, D = geometry(M, R, match, gap)
    assert slack(gap) == 0 and bound(M, R, match, gap) == max(match * (M - P), match * P) == match * (M - P)
    for name, (read, B, cells, rows) in main_case.items():
        val = read.val[R, 1]
        if B > bound(M, R, match, gap):
            for i, j in cells:
                # every cell that holds B lies at most W columns right of a row-P cell of value >= B - smax (m - P) ...
                seg = rows[R][max(0, j - W):j + 1]
                assert i > P and seg.max() >= B - match * (i - P) >= B - match * (M - P), (name, R, i, j)
                # ... which the fold sees as it is, in its own sub-chunk or (the one column of lane lag) the next
                c = max(0, j - W) + int(np.argmax(seg))
                s = (c - 1) // SUB
                assert val[s:s + 2].max() >= B - match * (M - P), (name, R, i, j, c)
        e = read.emulate(R, CAP)
        assert e["B0"] <= B
        print("R=%d %-14s B=%g offender=%d %s evaluated=%s" % (R, name, B, e["offender"], e["why"], e["evaluated"][:6]))
        if name == "late_errors" and e["offender"]:
            # above the bound, but its threshold B - smax (m - P) is what row P reaches against the background in more sub-chunks than
            # the cap: the cap's offender (at 60 k columns only a four-letter background this low does that)
            assert e["why"] == "over the cap" and e["B0"] == B > bound(M, R, match, gap) and R < HEIGHTS[-1], (R, e["why"], e["B0"])
            continue
        assert e["offender"] == (name == "random"), (name, R, e["why"], e["B0"])
        if e["offender"]:
            assert e["B0"] <= bound(M, R, match, gap)
            continue
        for i, j in cells:
            assert covers(e["evaluated"], j - 1), (name, R, i, j, e["evaluated"])
        first = min((j, i) for i, j in cells)
        assert e["result"] == (B, first[1], first[0]), (name, R, e["result"], B, first)


def test_values_are_row_maxima(main_case):
    """With the fold at every step a sub-chunk value is the maximum of row P over the columns lane 1 visits during the sub-chunk's
    steps: columns s E .. (s + 1) E - 1 (1-based), the range's last sub-chunk to its end."""
    for name, (read, B, cells, rows) in main_case.items():
        for R in HEIGHTS:
            row, val = rows[R], read.val[R, 1]
            for s in range(len(val)):
                lo, hi = max(1, s * SUB), (s + 1) * SUB if s + 1 < len(val) else len(row)
                assert val[s] == row[lo:hi].max(), (name, R, s)


@pytest.fixture(scope="module")
def two_letter_case():
    """Reference over A / C, reads over G / T (prefix values are zero away from the planted copies): per height one read whose copy
    scores bound + 1 (one inserted column below row P: 3 k - 2) and one that scores the bound exactly (3 k).  The oracle says so."""
    rng = np.random.default_rng(6211)
    y = bytearray(_dna(rng, N, b"AC"))
    reads = {}
    for h, R in enumerate(HEIGHTS):
        b = int(bound(M, R, 3.0, 2.0))
        assert b % 3 == 0
        k = (b + 3) // 3                                                 # 3 k - 2 = bound + 1
        above = _dna(rng, k, b"GT")
        at = (20 + 60 * h) * SUB + 9
        y[at:at + k + 1] = above[:70] + b"A" + above[70:]
        equal = _dna(rng, b // 3, b"GT")
        at = (40 + 60 * h) * SUB + 40
        y[at:at + len(equal)] = equal
        reads[R] = (above + b"N" * (M - k), equal + b"N" * (M - len(equal)))
    return reads, bytes(y)


@pytest.mark.parametrize("R", HEIGHTS)
def test_reads_at_the_bound(two_letter_case, R):
    reads, y = two_letter_case
    b = bound(M, R, 3.0, 2.0)
    assert b == {13: 372, 16: 354, 19: 336}[R]
    above, equal = reads[R]
    B, cells, _ = _truth(above, y, SCORING)
    assert B == b + 1
    e = Read(above, y, SCORING, HEIGHTS).emulate(R, CAP)
    assert not e["offender"] and e["result"][0] == B and all(covers(e["evaluated"], j - 1) for _, j in cells), e
    B, _, _ = _truth(equal, y, SCORING)
    assert B == b
    e = Read(equal, y, SCORING, HEIGHTS).emulate(R, CAP)
    assert e["offender"] and e["why"] == "B0 cannot certify" and e["B0"] == b, e
    # the read at this height's bound is what the next height up certifies: its second pass
    if R < HEIGHTS[-1]:
        e = Read(equal, y, SCORING, HEIGHTS).emulate(HEIGHTS[HEIGHTS.index(R) + 1], CAP)
        assert not e["offender"] and e["result"][0] == b, e


def test_start_height_rule():
    P = [26, 32, 38]
    assert start_height(P, [10, 0, 0]) == 0 and start_height(P, [11, 0, 0]) == 1             # (o + 2) 32 <= 64 * 6: o <= 10
    assert start_height(P, [11, 8, 0]) == 1 and start_height(P, [11, 9, 0]) == 2             # (o + 2) 38 <= 64 * 6: o <= 8
    assert start_height(P, [64, 40, 32]) == 2 and start_height(P, [64, 40, 33]) == -1        # the last height: more than half hopeless
    assert start_height([38], [32]) == 0 and start_height([38], [33]) == -1
    assert start_height([32, 38], [8, 64]) == 0 and start_height([32, 38], [9, 20]) == 1


class _Scripted:
    """A read whose passes are scripted: certified from height `ok` on (None: never), over the cap below it when `cap_below`, else
    short of the bound there (B0 = 3 * 118 = 354 means: not above the bound of P = 32 either)."""

    def __init__(self, ok, B0=444.0, cap_below=False):
        self.x, self.scoring, self.ok, self.B0, self.cap_below = b"A" * M, SCORING, ok, B0, cap_below

    def emulate(self, R, cap, mk=1, vote_Rs=()):
        good = lambda r: self.ok is not None and r >= self.ok
        why = "" if good(R) else ("over the cap" if self.cap_below else "B0 cannot certify")
        return dict(offender=not good(R), why=why, B0=self.B0, votes={r: good(r) for r in vote_Rs})


def test_chain_on_counted_examples():
    n = 1040
    # ten probe offenders: the start stays at R = 13; those R = 16 certifies take the second pass with the rest's offenders whose B0
    # is above 354, a cap offender among them; B0 = 354 skips it; the second pass's own offender goes to the sweep
    reads = [_Scripted(13) for _ in range(n)]
    for k in range(8):
        reads[3 * k] = _Scripted(16, 366.0)
    reads[40], reads[41] = _Scripted(None, 0.0), _Scripted(19, 350.0)
    reads[100], reads[200], reads[300], reads[400] = _Scripted(16, 372.0), _Scripted(16, 420.0, True), _Scripted(19, 354.0), _Scripted(19, 360.0)
    emu = emulate_chain(reads, 19, 64)
    assert emu["o"] == [10, 2, 1] and emu["start"] == 13 and emu["riders"] == []
    assert emu["launches"] == [(13, PROBE), (13, n - PROBE), (16, 11)] and emu["second"] == sorted([3 * k for k in range(8)] + [100, 200, 400])
    assert emu["offenders"] == {40, 41, 300, 400}
    # an eleventh: the start moves to R = 16 with nine riders; the probe's other offenders wait for R = 19 or go to the sweep
    reads[50] = _Scripted(16, 366.0)
    emu = emulate_chain(reads, 19, 64)
    assert emu["o"] == [11, 2, 1] and emu["start"] == 16 and emu["riders"] == [3 * k for k in range(8)] + [50]
    assert emu["launches"] == [(13, PROBE), (16, n - PROBE + 9), (19, 3)] and emu["second"] == [41, 300, 400] and emu["offenders"] == {40}
    # most of the probe hopeless at every height: the probe fails, nothing else is launched
    for k in range(33):
        reads[k] = _Scripted(None, 0.0)
    emu = emulate_chain(reads, 19, 64)
    assert emu["outcome"] == "probe_failed" and emu["launches"] == [(13, PROBE)] and emu["o"][2] == 34   # (read 40 as well)
    # a rest that mostly offends gives up: nobody takes a second pass
    reads = [_Scripted(13) for _ in range(PROBE)] + [_Scripted(16, 366.0) for _ in range(n - PROBE)]
    emu = emulate_chain(reads, 19, 64)
    assert emu["start"] == 13 and emu["second"] == [] and emu["offenders"] == set(range(PROBE, n)) and len(emu["launches"]) == 2
