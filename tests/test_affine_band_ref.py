"""Pins the checker of the banded affine pairs (tests/affine_band_ref.py), no GPU and no project code: a band that covers the matrix is
the unbanded checker (tests/affine_ref.py, tests/affine_trace_ref.py), bytes of the strings included; widening a band never lowers the
score; the strings' value is the score and each of their cells lies in the band; the model's two statements (out-of-band cells hold
-inf / an out-of-band neighbour holds H = 0) give the same in-band cells; a plain three-loop banded DP agrees; and recorded answers
(tests/golden/affine_band_pins.json) stay what they were."""
import json
import os

import numpy as np

from tests import affine_band_ref as br, affine_ref, affine_trace_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SCORINGS = [dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0), dict(match=2.0, mismatch=-1.0, gap_open=2.0, gap_extend=2.0),
            dict(match=5.0, mismatch=-4.0, gap_open=8.0, gap_extend=3.0)]


def _case(rng, mmax=14, nmax=18, letters=3):
    m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(1, nmax + 1))
    x = bytes(rng.integers(65, 65 + letters, m).astype(np.uint8))
    y = bytes(rng.integers(65, 65 + letters, n).astype(np.uint8))
    lo = int(rng.integers(-m - 2, n + 2))
    hi = lo + int(rng.integers(0, 9))
    return x, y, lo, hi


def _loops(x, y, lo, hi, match, mismatch, gap_open, gap_extend):
    """The banded model by three plain loops over the in-band cells only; everything else is -inf (a dict without the key)."""
    m, n = len(x), len(y)
    ninf = float("-inf")
    H, E, F = {}, {}, {}
    for i in range(m + 1):
        for j in range(n + 1):
            if (i == 0 or j == 0) and lo <= j - i <= hi:
                H[i, j] = 0.0
    best, bi, bj = 0.0, 0, 0
    for j in range(1, n + 1):
        for i in range(1, m + 1):
            if not lo <= j - i <= hi:
                continue
            s = match if x[i - 1] == y[j - 1] else mismatch
            E[i, j] = max(E.get((i, j - 1), ninf) - gap_extend, H.get((i, j - 1), ninf) - gap_open)
            F[i, j] = max(F.get((i - 1, j), ninf) - gap_extend, H.get((i - 1, j), ninf) - gap_open)
            H[i, j] = max(0.0, H.get((i - 1, j - 1), ninf) + s, E[i, j], F[i, j])
            if H[i, j] > best:
                best, bi, bj = H[i, j], i, j
    return best, bi, bj


def test_covering_band_is_the_unbanded_checker():
    rng = np.random.default_rng(11)
    for k in range(120):
        x, y, _, _ = _case(rng)
        sc = SCORINGS[k % len(SCORINGS)]
        m, n = len(x), len(y)
        for lo, hi in ((1 - m, n - 1), (-m - 5, n + 7), (-10 ** 12, 10 ** 12)):
            assert br.locate(x, y, lo, hi, **sc) == affine_ref.locate(x, y, **sc)
            got, exp = br.trace(x, y, lo, hi, **sc), affine_trace_ref.trace(x, y, **sc)
            for f in exp:
                assert got[f] == exp[f], (f, x, y, sc)


def test_plain_loops_agree():
    rng = np.random.default_rng(12)
    for k in range(400):
        x, y, lo, hi = _case(rng)
        sc = SCORINGS[k % len(SCORINGS)]
        assert br.locate(x, y, lo, hi, **sc) == _loops(x, y, lo, hi, **sc), (x, y, lo, hi, sc)


def test_widening_never_lowers_the_score():
    rng = np.random.default_rng(13)
    for k in range(150):
        x, y, lo, hi = _case(rng)
        sc = SCORINGS[k % len(SCORINGS)]
        last = -1.0
        for w in range(0, 8):
            s = br.locate(x, y, lo - w, hi + w, **sc)[0]
            assert s >= last
            last = s
        assert last <= affine_ref.locate(x, y, **sc)[0]


def test_strings_are_worth_the_score_and_stay_in_the_band():
    rng = np.random.default_rng(14)
    seen_gap = 0
    for k in range(300):
        x, y, lo, hi = _case(rng, 20, 24, 2)
        sc = SCORINGS[k % len(SCORINGS)]
        t = br.trace(x, y, lo, hi, **sc)
        if t["score"] == 0:
            assert (t["end_x"], t["end_y"], t["cons_x"], t["cons_y"], t["pos"]) == (0, 0, "", "", 0)
            continue
        assert br.rescore(t["cons_x"], t["cons_y"], **sc) == t["score"]
        cells = br.cells_of(t["cons_x"], t["cons_y"], t["end_x"], t["end_y"])
        assert cells == t["cells"]
        assert all(lo <= j - i <= hi and i >= 1 and j >= 1 for i, j in cells)
        assert lo <= t["end_y"] - t["end_x"] <= hi
        seen_gap += "-" in t["cons_x"] + t["cons_y"]
    assert seen_gap > 10


def test_both_statements_of_the_model_agree():
    rng = np.random.default_rng(15)
    for k in range(300):
        x, y, lo, hi = _case(rng)
        sc = SCORINGS[k % len(SCORINGS)]
        H, E, F, S, band = br.matrices(x, y, lo, hi, **sc)
        H0, E0, F0, _, _ = br.matrices(x, y, lo, hi, zero_outside=True, **sc)
        inner = band.copy()
        inner[0, :] = False
        inner[:, 0] = False
        assert np.array_equal(H[inner], H0[inner])
        # E and F differ only where both are negative (-o from a zero neighbour against -inf): never where they decide a cell
        assert np.array_equal(np.maximum(E[inner], 0.0), np.maximum(E0[inner], 0.0))
        assert np.array_equal(np.maximum(F[inner], 0.0), np.maximum(F0[inner], 0.0))
        assert br.end_cell(H, band) == br.end_cell(H0, band)


def test_a_band_that_binds():
    a, ins, b = "ACGTTGCAAGGCTTAC", "T" * 20, "GGATCCATTGCAGTCA"
    x, y = a + b, a + ins + b
    full = affine_ref.locate(x, y)[0]
    banded = br.locate(x, y, -5, 5)[0]
    assert full == 3.0 * 32 - (5 + 19) and banded == 3.0 * 16 and banded < full
    assert br.locate(y, x, -5, 5)[0] == 3.0 * 16                      # the mirror case: the insert in x


def test_pins():
    with open(os.path.join(HERE, "golden", "affine_band_pins.json")) as f:
        pins = json.load(f)
    assert len(pins) >= 24
    for p in pins:
        t = br.trace(p["x"], p["y"], p["lo"], p["hi"], **p["scoring"])
        for f in ("score", "end_x", "end_y", "begin_x", "pos", "cons_x", "cons_y", "cigar"):
            assert t[f] == p[f], (f, p)
