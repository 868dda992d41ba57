"""Pins the checker of the z-drop stop rule (tests/affine_zdrop_ref.py; no GPU, no project code): its two statements of the rule agree,
the results are those of the banded extension on the first rows_done letters (the definition by truncation), zdrop = inf is the banded
extension itself, a stop can change the best extension, and every branch of the rule on matrices written by hand."""
import numpy as np
import pytest

from tests import affine_extend_band_ref as B
from tests import affine_zdrop_ref as Z

NINF = Z.NINF
INF = float("inf")
SCORINGS = (dict(match=1.0, mismatch=-4.0, gap_open=7.0, gap_extend=1.0), dict(match=2.0, mismatch=-6.0, gap_open=10.0, gap_extend=2.0),
            dict(match=3.0, mismatch=-9.0, gap_open=12.0, gap_extend=2.0), dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0))


def _cases(seed, count, mmax=14, nmax=18):
    rng = np.random.default_rng(seed)
    for k in range(count):
        m, n = int(rng.integers(0, mmax + 1)), int(rng.integers(0, nmax + 1))
        y = bytes(rng.choice(list(b"ACGT"), n).tolist())
        x = bytes((y + y)[:m]) if n else bytes(rng.choice(list(b"ACGT"), m).tolist())
        cut = int(rng.integers(0, m + 1))                              # a tail of junk from a random point
        x = x[:cut] + bytes(rng.choice(list(b"ACGT"), m - cut).tolist())
        lo, hi = -int(rng.integers(0, 7)), int(rng.integers(0, 7))
        yield x, y, lo, hi, float(rng.integers(0, 25)), bool(k & 1), SCORINGS[k % len(SCORINGS)]


def test_loops_equal_vectors():
    stopped = 0
    for x, y, lo, hi, z, back, sc in _cases(1, 600):
        a = Z.rows_done(x, y, lo, hi, z, back, mats=B.matrices_loops, rule=Z.stop_row_loops, **sc)
        b = Z.rows_done(x, y, lo, hi, z, back, **sc)
        assert a == b, (x, y, lo, hi, z, back)
        assert (0 if not x else 1) <= a <= len(x)
        stopped += a < len(x)
        if x:
            H = B.matrices(x[::-1] if back else x, y[::-1] if back else y, lo, hi, **sc)[0]
            r0, c0 = Z.row_maxima_loops(H)
            r1, c1 = Z.row_maxima(H)
            assert np.array_equal(r0, r1) and np.array_equal(c0[r0 > NINF], c1[r1 > NINF])
    assert 100 < stopped < 500                                          # both branches


def test_results_are_the_banded_extension_on_the_first_rows_done_letters():
    for x, y, lo, hi, z, back, sc in _cases(2, 300):
        got = Z.locate(x, y, lo, hi, z, back, **sc)
        s, m = got["rows_done"], len(x)
        cut = x[m - s:] if back else x[:s]
        want = B.locate(cut, y, lo, hi, backward=back, **sc)
        if s < m:
            assert (got["to_end_score"], got["to_end_y"]) == (NINF, -1)
            want["to_end_score"], want["to_end_y"] = NINF, -1
            assert got["end_x"] < s or got["score"] == 0                # row s cannot hold the best: r_s < B
        assert {k: got[k] for k in want} == want
        for te in (False, True):
            t = Z.trace(x, y, lo, hi, z, back, te, **sc)
            assert t["rows_done"] == s
            if s < m and te:
                assert (t["score"], t["end_x"], t["end_y"], t["cons_x"], t["cons_y"], t["cigar"]) == (NINF, 0, 0, "", "", "")
                continue
            w = B.trace(cut, y, lo, hi, backward=back, to_end=te, **sc)
            assert all(t[k] == w[k] for k in ("score", "end_x", "end_y", "pos", "cons_x", "cons_y", "cigar"))
            assert t["end_x"] <= s
            if t["score"] > NINF and t["cons_x"]:
                assert B.rescore(t["cons_x"], t["cons_y"], **sc) == t["score"]


def test_an_infinite_zdrop_is_the_banded_extension():
    for x, y, lo, hi, z, back, sc in _cases(3, 200):
        got = Z.locate(x, y, lo, hi, INF, back, **sc)
        assert got.pop("rows_done") == len(x)
        assert got == B.locate(x, y, lo, hi, backward=back, **sc)


def test_a_stop_changes_the_best_extension():
    """30 matching letters, 15 that mismatch, 100 matching letters: the full matrix's best jumps the junk, the stopped one does not."""
    rng = np.random.default_rng(7)
    y = bytes(rng.choice(list(b"ACGT"), 160).tolist())
    junk = bytes({65: 67, 67: 71, 71: 84, 84: 65}[c] for c in y[30:45])
    x = y[:30] + junk + y[45:145]
    sc = SCORINGS[0]
    full = B.locate(x, y, -16, 16, **sc)
    cut = Z.locate(x, y, -16, 16, 20.0, **sc)
    assert full["score"] > 60 and full["end_x"] == 145
    assert 30 < cut["rows_done"] < 60 and (cut["score"], cut["end_x"], cut["end_y"]) == (30.0, 30, 30)
    assert (cut["to_end_score"], cut["to_end_y"]) == (NINF, -1)


def _H(rows):
    return np.array(rows, dtype=np.float64)


@pytest.mark.parametrize("rule", (Z.stop_row_loops, Z.stop_row))
def test_the_rule_branch_by_branch(rule):
    n = NINF
    # rows 0 and 1 of every case: the anchor, then B = 5 at (1, 1)
    top = [[0, -1, -2, -3], [-1, 5, 1, 0]]
    # the drop without a diagonal offset: r_2 = 1 at (2, 2), d = 0, B - r = 4; strictly greater than zdrop stops
    H = _H(top + [[n, 0, 1, 0], [n, n, 9, 9]])
    assert rule(H, 1.0, 3.0) == 2 and rule(H, 1.0, 4.0) == 3 and rule(H, 1.0, 3.5) == 2
    # the diagonal term, c_i right of the best's diagonal: r_2 = 1 at (2, 3), d = |1 - 2| = 1: 4 - e
    H = _H(top + [[n, 0, 0, 1], [n, n, 9, 9]])
    assert rule(H, 1.0, 3.0) == 3 and rule(H, 1.0, 2.0) == 2 and rule(H, 0.0, 3.0) == 2 and rule(H, 2.0, 2.0) == 3
    # ... and left of it: r_2 = 1 at (2, 0), d = |1 - (-1)| = 2: 4 - 2 e
    H = _H(top + [[1, 0, 0, 0], [n, n, 9, 9]])
    assert rule(H, 1.0, 2.0) == 3 and rule(H, 1.0, 1.0) == 2 and rule(H, 0.0, 3.0) == 2
    # the smallest column of a repeated row maximum: 1 at columns 1 and 3 — c_2 = 1, d = 1
    H = _H(top + [[n, 1, 0, 1], [n, n, 9, 9]])
    assert rule(H, 1.0, 2.0) == 2 and rule(H, 1.0, 3.0) == 3
    # an equal r_i does not move (bi, bj): row 2 holds 5 again, at (2, 3), one diagonal to the right; row 3's 1 at (3, 3) lies on the
    # diagonal of (1, 1): d = 0 and the drop is 4 (from (2, 3) it would be d = 1 and 3)
    H = _H(top + [[n, 0, 0, 5], [n, n, 0, 1], [n, n, n, 9]])
    assert rule(H, 1.0, 3.0) == 3 and rule(H, 1.0, 4.0) == 4
    # a greater r_i moves it: B = 6 at (2, 3), then 2 at (3, 3): d = 1, 4 - e
    H = _H(top + [[n, 0, 0, 6], [n, n, 0, 2], [n, n, n, 9]])
    assert rule(H, 1.0, 3.0) == 4 and rule(H, 1.0, 2.0) == 3
    # a row without an in-band real column stops for every finite zdrop, and never for an infinite one
    H = _H(top + [[n, n, n, n], [n, n, n, n]])
    assert rule(H, 1.0, 1e30) == 2 and rule(H, 1.0, INF) == 3
    # row m is never tested: the drop of the last row leaves rows_done = m
    H = _H(top + [[n, 4, 4, 4], [n, n, -50, -60]])
    assert rule(H, 1.0, 3.0) == 3
    # the anchor is the first best: B = 0 at (0, 0); r_1 = -4 at (1, 1) drops by 4, the border cell (1, 0) = -4 by 4 - e
    assert rule(_H([[0, -7], [-7, -4], [n, 0]]), 1.0, 3.0) == 1 and rule(_H([[0, -7], [-7, -4], [n, 0]]), 1.0, 4.0) == 2
    assert rule(_H([[0, -7], [-4, -9], [n, 0]]), 1.0, 2.0) == 1 and rule(_H([[0, -7], [-4, -9], [n, 0]]), 1.0, 3.0) == 2
    # fewer than two rows: nothing is tested
    assert rule(_H([[0, -7]]), 1.0, 0.0) == 0 and rule(_H([[0, -7], [-99, -99]]), 1.0, 0.0) == 1


def test_an_empty_window_is_the_rule_on_the_border_column():
    # H(i, 0) = -(o + (i-1) e), B = 0 at the anchor and d = i: the drop is o - e in every in-band row; the first row below the band stops
    sc = dict(match=1.0, mismatch=-4.0, gap_open=7.0, gap_extend=1.0)
    assert Z.locate(b"ACGTACGT", b"", -8, 3, 6.0, **sc)["rows_done"] == 8
    assert Z.locate(b"ACGTACGT", b"", -8, 3, 5.0, **sc)["rows_done"] == 1
    assert Z.locate(b"ACGTACGT", b"", -3, 3, 6.0, **sc)["rows_done"] == 4
    got = Z.locate(b"ACGTACGT", b"", -3, 3, 6.0, **sc)
    assert (got["score"], got["end_x"], got["end_y"], got["to_end_score"], got["to_end_y"]) == (0.0, 0, 0, NINF, -1)
    assert Z.locate(b"", b"ACGT", -3, 3, 6.0, **sc)["rows_done"] == 0
