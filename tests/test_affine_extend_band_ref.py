"""Pins the checker of the banded anchored extension (tests/affine_extend_band_ref.py; no GPU, no project code): its two statements
of the model agree, a band that covers the matrix is the unbanded model of tests/affine_extend_ref.py field for field, widening a band
never lowers a score, the read's end is unreachable exactly when band_lo > n - m, the window clip changes nothing, every emitted cell
of a walk lies in the band and the strings rescore to the score, and a case worked by hand."""
import numpy as np
import pytest

from tests import affine_extend_band_ref as B
from tests import affine_extend_ref as X

SCORINGS = (dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0), dict(match=2.0, mismatch=-4.0, gap_open=2.0, gap_extend=2.0),
            dict(match=1.0, mismatch=-1.0, gap_open=6.0, gap_extend=1.0), dict(match=5.0, mismatch=-2.0, gap_open=1.0, gap_extend=1.0))


def _cases(seed, count, mmax=9, nmax=12):
    rng = np.random.default_rng(seed)
    for k in range(count):
        m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(0, nmax + 1))
        x = bytes(rng.choice(list(b"ACGT"), m).tolist())
        y = bytes(rng.choice(list(b"ACGT"), n).tolist())
        if n and rng.random() < 0.6:                                  # related strings: alignments worth extending
            y = bytes((x * 3)[:n])
            y = bytes(c if rng.random() > 0.15 else int(rng.choice(list(b"ACGT"))) for c in y)
        lo, hi = -int(rng.integers(0, mmax + 3)), int(rng.integers(0, nmax + 3))
        yield x, y, lo, hi, SCORINGS[k % len(SCORINGS)]


def test_loops_equal_vectors():
    for x, y, lo, hi, sc in _cases(1, 400):
        a, b = B.matrices_loops(x, y, lo, hi, **sc), B.matrices(x, y, lo, hi, **sc)
        for u, v in zip(a, b):
            assert np.array_equal(u, v), (x, y, lo, hi)
        H = a[0]
        i, j = np.indices(H.shape)
        inside = (j - i >= lo) & (j - i <= hi)
        assert np.isfinite(H[inside]).all() and (H[~inside] == B.NINF).all()      # every in-band cell is finite, and no other


def test_a_covering_band_is_the_unbanded_model():
    for x, y, lo, hi, sc in _cases(2, 200):
        m, n = len(x), len(y)
        for blo, bhi in ((-m, n), (-m - 3, n + 5)):
            for back in (False, True):
                assert B.locate(x, y, blo, bhi, backward=back, **sc) == X.locate(x, y, backward=back, **sc)
                for te in (False, True):
                    assert B.trace(x, y, blo, bhi, backward=back, to_end=te, **sc) == X.trace(x, y, backward=back, to_end=te, **sc)


def test_widening_a_band_never_lowers_a_score():
    for x, y, lo, hi, sc in _cases(3, 300):
        a = B.locate(x, y, lo, hi, **sc)
        b = B.locate(x, y, lo - 1, hi + 2, **sc)
        assert b["score"] >= a["score"] >= 0 and b["to_end_score"] >= a["to_end_score"]
        if a["score"] == 0:
            assert (a["end_x"], a["end_y"]) == (0, 0)


def test_unreachable_exactly_when_the_band_misses_row_m():
    seen = set()
    for x, y, lo, hi, sc in _cases(4, 400):
        m, n = len(x), len(y)
        r = B.locate(x, y, lo, hi, **sc)
        assert B.reachable(m, n, lo) == (lo <= n - m)
        assert (r["to_end_y"] == -1) == (r["to_end_score"] == B.NINF) == (lo > n - m)
        seen.add(lo > n - m)
        t = B.trace(x, y, lo, hi, to_end=True, **sc)
        if lo > n - m:
            assert (t["score"], t["end_x"], t["end_y"], t["pos"], t["cons_x"], t["cons_y"]) == (B.NINF, 0, 0, 0, "", "")
    assert seen == {False, True}
    # n = 0: today's host-filled answer when band_lo <= -m, unreachable otherwise
    assert B.locate(b"ACG", b"", -3, 0) == dict(score=0.0, end_x=0, end_y=0, to_end_score=-7.0, to_end_y=0)
    assert B.locate(b"ACG", b"", -2, 0) == dict(score=0.0, end_x=0, end_y=0, to_end_score=B.NINF, to_end_y=-1)


def test_the_window_clip_changes_nothing():
    for x, y, lo, hi, sc in _cases(5, 300, nmax=20):
        nc = B.clip(len(x), len(y), hi)
        assert nc <= len(y)
        for back in (False, True):                                    # a backward pair keeps the columns next to ITS anchor: the last nc
            cut = y[len(y) - nc:] if back else y[:nc]
            assert B.locate(x, y, lo, hi, backward=back, **sc) == B.locate(x, cut, lo, hi, backward=back, **sc)
            for te in (False, True):
                assert B.trace(x, y, lo, hi, backward=back, to_end=te, **sc) == B.trace(x, cut, lo, hi, backward=back, to_end=te, **sc)


def test_walks_stay_in_the_band_and_rescore():
    for x, y, lo, hi, sc in _cases(6, 300):
        for back in (False, True):
            for te in (False, True):
                t = B.trace(x, y, lo, hi, backward=back, to_end=te, **sc)
                if t["score"] == B.NINF:
                    continue
                cells = B.path_cells(t["cons_x"], t["cons_y"], t["end_x"], t["end_y"])
                assert all(B.in_band(i, j, lo, hi) for i, j in cells), (x, y, lo, hi, t)
                assert B.rescore(t["cons_x"], t["cons_y"], **sc) == t["score"]
                assert len(t["cons_x"].replace("-", "")) == t["end_x"] and len(t["cons_y"].replace("-", "")) == t["end_y"]


def test_hand_worked_three_rows():
    """x = ACG against y = ATCG, match 3, mismatch -3, o = 5, e = 1.  Unbanded: A/A (3), the T of y against a gap (-5), C/C and G/G
    (+6): 4 at (3,4), on diagonal 1.  Under the band [0, 0] only the main diagonal exists: H(1,1) = 3, H(2,2) = 3 - 3 = 0,
    H(3,3) = 0 - 3 = -3; the gap is forbidden, the best extension drops to 3 at (1,1) and the read's end costs -3 at column 3.
    Under [-1, 1] the gap fits and the unbanded answer is back."""
    x, y = b"ACG", b"ATCG"
    H = B.matrices_loops(x, y, 0, 0)[0]
    assert [H[k, k] for k in range(4)] == [0.0, 3.0, 0.0, -3.0]
    assert B.locate(x, y, 0, 0) == dict(score=3.0, end_x=1, end_y=1, to_end_score=-3.0, to_end_y=3)
    t = B.trace(x, y, 0, 0, to_end=True)
    assert (t["cons_x"], t["cons_y"], t["cigar"]) == ("GCA", "CTA", "3M")
    wide = B.locate(x, y, -1, 1)
    assert wide == X.locate(x, y) == dict(score=4.0, end_x=3, end_y=4, to_end_score=4.0, to_end_y=4)
    t = B.trace(x, y, -1, 1)
    assert (t["cons_x"], t["cons_y"], t["cigar"]) == ("GC-A", "GCTA", "1M1D2M")
    # a window shorter than the read under the diagonal alone: the end is unreachable
    assert B.locate(x, b"AC", 0, 0) == dict(score=6.0, end_x=2, end_y=2, to_end_score=B.NINF, to_end_y=-1)


@pytest.mark.parametrize("lo,hi", [(1, 2), (-2, -1)])
def test_a_band_must_hold_the_anchor(lo, hi):
    with pytest.raises(AssertionError):
        B.matrices(b"ACGT", b"ACGT", lo, hi)
