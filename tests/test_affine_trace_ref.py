"""Pins tests/affine_trace_ref.py, the checker of the affine-gap traceback, independently of itself: the walk's strings are worth
the score and spell the two substrings between begin and end cell, score and end cell are those of tests/affine_ref.py, no
alignment ending at the end cell beats it (brute force on tiny inputs), the three priorities of the rule on hand-made ties, the
known pairs of tests/test_gpu_affine.py, and the statement of lemma L17: the walk over the window alone equals the
walk over the full matrices.  No GPU and no project code."""
import numpy as np
import pytest

from tests import affine_ref, affine_trace_ref as tr

A = "ACGGTCATGCTA"
B = "GTACCTGAATCG"
KNOWN = [(A + B, "CCCC" + A + "TTT" + B + "CCCC", (24, 31), "12M3D12M"), (A + "GGG" + B, "CCCC" + A + B + "CCCC", (27, 28), "12M3I12M")]
KNOWN_SCORES = {(5, 1): 65, (5, 5): 57, (1, 1): 69, (2, 2): 66, (7, 2): 61}
SCORINGS = [(3, -3, 5, 1), (2, -1, 3, 1), (1, -1, 2, 2), (5, -4, 10, 3)]


def _random_problems(count, seed, mmax=24, nmax=60):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        alpha = np.frombuffer(b"ACGT" if k % 2 == 0 else b"AC", dtype=np.uint8)
        m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(1, nmax + 1))
        x = alpha[rng.integers(0, len(alpha), m)].tobytes()
        y = bytearray(alpha[rng.integers(0, len(alpha), n)].tobytes())
        if k % 3 == 0 and m >= 8 and n >= m + 3:                    # a planted copy with a 3-column insert
            at = int(rng.integers(0, n - m - 2))
            y[at:at + m + 3] = x[:m // 2] + alpha[rng.integers(0, len(alpha), 3)].tobytes() + x[m // 2:]
        elif k % 3 == 1 and n >= m:                                 # an exact copy
            at = int(rng.integers(0, n - m + 1))
            y[at:at + m] = x
        out.append((x.decode(), bytes(y).decode(), SCORINGS[k % len(SCORINGS)]))
    return out


def _ungap(s):
    return s.replace("-", "")[::-1]


def test_walk_is_worth_the_score_and_spells_the_substrings():
    for x, y, sc in _random_problems(150, 11):
        r = tr.trace(x, y, *sc)
        assert (r["score"], r["end_x"], r["end_y"]) == affine_ref.locate(x, y, *sc), (x, y, sc)
        if r["score"] == 0:
            assert (r["pos"], r["cons_x"], r["cons_y"], r["cigar"], r["begin_x"]) == (0, "", "", "", 0)
            continue
        assert tr.rescore(r["cons_x"], r["cons_y"], *sc) == r["score"], (x, y, sc, r)
        assert _ungap(r["cons_x"]) == x[r["begin_x"] - 1:r["end_x"]], (x, y, sc, r)
        assert _ungap(r["cons_y"]) == y[r["begin_y"] - 1:r["end_y"]], (x, y, sc, r)
        assert r["cons_x"][-1] != "-" and r["cons_y"][-1] != "-" and r["cons_x"][0] != "-" and r["cons_y"][0] != "-"


def _alignments_ending_at(i, j):
    """Every sequence of steps (D = diagonal, E = a column of y against '-', F = a row of x against '-') from some cell to
    (i, j), as (begin row - 1, begin column - 1, steps in forward order)."""
    out = []

    def grow(ci, cj, steps):
        if steps:
            out.append((ci, cj, steps))
        if ci > 0 and cj > 0:
            grow(ci - 1, cj - 1, "D" + steps)
        if cj > 0:
            grow(ci, cj - 1, "E" + steps)
        if ci > 0:
            grow(ci - 1, cj, "F" + steps)

    grow(i, j, "")
    return out


def test_no_alignment_ending_at_the_end_cell_scores_higher():
    rng = np.random.default_rng(5)
    for k in range(40):
        m, n = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        x = "".join("AC"[v] for v in rng.integers(0, 2, m))
        y = "".join("AC"[v] for v in rng.integers(0, 2, n))
        sc = SCORINGS[k % len(SCORINGS)]
        r = tr.trace(x, y, *sc)
        if r["score"] == 0:
            assert not set(x) & set(y)
            continue
        best = 0.0
        for bi, bj, steps in _alignments_ending_at(r["end_x"], r["end_y"]):
            cx, cy, i, j = [], [], bi, bj
            for s in steps:
                if s == "D":
                    cx.append(x[i]); cy.append(y[j]); i += 1; j += 1
                elif s == "E":
                    cx.append("-"); cy.append(y[j]); j += 1
                else:
                    cx.append(x[i]); cy.append("-"); i += 1
            best = max(best, tr.rescore("".join(cx), "".join(cy), *sc))
        assert best == r["score"], (x, y, sc, best, r)


def test_tie_diagonal_over_E():
    x, y, sc = "ACA", "ACCA", (2, -1, 1, 1)
    H, E, F, S = tr.matrices(x, y, *sc)
    assert H[2, 3] == H[1, 2] + S[2, 3] == E[2, 3] > 0              # the walk meets (2, 3) in state M: diagonal and E tie
    r = tr.trace(x, y, *sc)
    assert (r["score"], r["cons_x"], r["cons_y"], r["cigar"], r["pos"]) == (5.0, "AC-A", "ACCA", "1M1D2M", 1)   # E first: 2M1D1M


def test_tie_E_over_F():
    x, y, sc = "ACG", "CAG", (4, -1, 2, 1)
    H, E, F, S = tr.matrices(x, y, *sc)
    assert H[2, 2] == E[2, 2] == F[2, 2] > H[1, 1] + S[2, 2]        # (2, 2) in state M: E and F tie, the diagonal is worse
    r = tr.trace(x, y, *sc)
    assert (r["score"], r["cons_x"], r["cons_y"], r["cigar"]) == (6.0, "G-C", "GAC", "1M1D1M")   # F first: 1M1I1M
    assert (r["begin_x"], r["begin_y"], r["end_x"], r["end_y"]) == (2, 1, 3, 3)


def test_tie_open_over_extend():
    x, y, sc = "AACA", "ACCGA", (4, -1, 2, 1)
    H, E, F, S = tr.matrices(x, y, *sc)
    assert E[3, 4] == H[3, 3] - 2 == E[3, 3] - 1                    # (3, 4) in state E: opening here and extending tie
    r = tr.trace(x, y, *sc)
    assert (r["score"], r["cons_x"], r["cons_y"], r["cigar"]) == (9.0, "A-CAA", "AGCCA", "3M1D1M")   # extending: a gap of 2


@pytest.mark.parametrize("go,ge", sorted(KNOWN_SCORES))
def test_known_pairs(go, ge):
    for x, y, end, cig in KNOWN:
        r = tr.trace(x, y, 3, -3, go, ge)
        assert r["score"] == KNOWN_SCORES[(go, ge)] and (r["end_x"], r["end_y"]) == end
        assert (r["begin_x"], r["begin_y"], r["pos"]) == (1, 5, 5) and r["cigar"] == cig, r
        assert tr.rescore(r["cons_x"], r["cons_y"], 3, -3, go, ge) == r["score"]


def _window_trace(x, y, match, mismatch, gap_open, gap_extend):
    """Lemma L17: the same walk over rows 1 .. end_x and the columns (end_y - W, end_y] alone behind a zero border, W = end_x +
    ceil((smax * end_x - score) / gap_extend) + 2, clamped at column 1.  (result, clamped)"""
    H = tr.matrices(x, y, match, mismatch, gap_open, gap_extend)[0]
    score, i, j = tr.end_cell(H)
    smax = max(match, mismatch, 0)
    W = i + int(np.ceil((smax * i - score) / float(gap_extend))) + 2
    clamped = W >= j
    nw = j if clamped else W
    wl = j - nw
    xw, yw = x[:i], y[wl:j]
    Hw, Ew, Fw, Sw = tr.matrices(xw, yw, match, mismatch, gap_open, gap_extend)
    assert Hw[i, nw] == score
    cx, cy, pos = tr.walk(xw, yw, Hw, Ew, Fw, Sw, i, nw, gap_open)
    return (cx, cy, pos + wl), clamped


def test_L17_window_walk_equals_full_walk():
    counts = {True: 0, False: 0}
    for x, y, sc in _random_problems(300, 23, mmax=10, nmax=90):
        r = tr.trace(x, y, *sc)
        if r["score"] == 0:
            continue
        got, clamped = _window_trace(x, y, *sc)
        counts[clamped] += 1
        assert got == (r["cons_x"], r["cons_y"], r["pos"]), (x, y, sc, clamped, got, r)
    assert counts[True] >= 30 and counts[False] >= 30, counts
