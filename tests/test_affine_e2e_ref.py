"""Pins tests/affine_e2e_ref.py, the checker of the end-to-end mode of the affine pairs calls, independently of itself: its two
restatements of the model agree, a planted substring scores match * m and ends at its FIRST copy, the score never exceeds the local
score of tests/affine_ref.py and equals it when the local alignment spans all of x, the strings are worth the score and spell all
of x, no fit alignment beats the score (brute force on tiny inputs), the column-0 run of F moves, and the statement of lemma L19
(DESIGN.md §3.8): the walk over the W-column window alone equals the walk over the full matrices, clamped and unclamped, negative
scores included.  No GPU and no project code."""
import numpy as np

from tests import affine_e2e_ref as er, affine_ref

SCORINGS = [(3, -3, 5, 1), (2, -1, 3, 1), (1, -1, 2, 2), (5, -4, 10, 3), (1, -10, 4, 1)]


def _random_problems(count, seed, mmax=20, nmax=70):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        alpha = np.frombuffer(b"ACGT" if k % 2 == 0 else b"AC", dtype=np.uint8)
        m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(1, nmax + 1))
        x = alpha[rng.integers(0, len(alpha), m)].tobytes()
        y = bytearray(alpha[rng.integers(0, len(alpha), n)].tobytes())
        if k % 4 == 0 and m >= 8 and n >= m + 3:                    # a planted copy with a 3-column insert
            at = int(rng.integers(0, n - m - 2))
            y[at:at + m + 3] = x[:m // 2] + alpha[rng.integers(0, len(alpha), 3)].tobytes() + x[m // 2:]
        elif k % 4 == 1 and n >= m:                                 # an exact copy
            at = int(rng.integers(0, n - m + 1))
            y[at:at + m] = x
        elif k % 4 == 2:                                            # nothing in common: a negative score
            y = bytearray(b"T" * n) if k % 2 else bytearray(b"N" * n)
        out.append((x.decode(), bytes(y).decode(), SCORINGS[k % len(SCORINGS)]))
    return out


def _ungap(s):
    return s.replace("-", "")[::-1]


def test_loops_and_diagonals_agree():
    negative = 0
    for x, y, sc in _random_problems(300, 5):
        a, b = er.matrices_loops(x, y, *sc), er.matrices(x, y, *sc)
        for u, v in zip(a, b):
            assert np.array_equal(u, v), (x, y, sc)
        ra, rb = er.trace(x, y, *sc, mats=er.matrices_loops), er.trace(x, y, *sc)
        assert ra == rb, (x, y, sc)
        negative += ra["score"] < 0
    assert negative > 30                                             # the no-floor side is exercised


def test_column_zero_border_and_empty_problems():
    H, E, F, _ = er.matrices("ACGT", "AC", 3, -3, 5, 2)
    assert H[:, 0].tolist() == [0, -5, -7, -9, -11] and F[1:, 0].tolist() == [-5, -7, -9, -11]
    assert (H[0] == 0).all() and (E[:, 0] < -1e17).all() and (F[0] < -1e17).all()
    for x, y in (("", "ACGT"), ("ACGT", ""), ("", "")):
        r = er.trace(x, y)
        assert (r["score"], r["end_x"], r["end_y"], r["pos"], r["cons_x"], r["cons_y"], r["cigar"], r["begin_x"]) == (0, 0, 0, 0, "", "", "", 0)


def test_planted_substring_ends_at_its_first_copy():
    rng = np.random.default_rng(7)
    for m in (1, 5, 17, 40):
        x = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), m)).decode()
        y = "N" * 6 + x + "N" * 9 + x + "N" * 4
        r = er.trace(x, y, 3, -3, 5, 1)
        assert (r["score"], r["end_x"], r["end_y"], r["begin_y"], r["cigar"]) == (3 * m, m, 6 + m, 7, "%dM" % m)


def test_never_above_the_local_score_and_equal_when_local_spans_x():
    equal = 0
    for x, y, sc in _random_problems(300, 9):
        r = er.trace(x, y, *sc)
        ls, li, lj = affine_ref.locate(x, y, *sc)
        assert r["score"] <= ls, (x, y, sc)
        from tests import affine_trace_ref as tr
        lt = tr.trace(x, y, *sc)
        if ls > 0 and lt["begin_x"] == 1 and lt["end_x"] == len(x):
            assert r["score"] == ls, (x, y, sc)
            equal += 1
    assert equal > 30


def test_strings_are_worth_the_score_and_spell_all_of_x():
    for x, y, sc in _random_problems(300, 13):
        r = er.trace(x, y, *sc)
        assert r["end_x"] == len(x) and 1 <= r["end_y"] <= len(y) and r["begin_x"] == 1
        assert er.rescore(r["cons_x"], r["cons_y"], *sc) == r["score"], (x, y, sc, r)
        assert _ungap(r["cons_x"]) == x, (x, y, sc, r)
        ycols = _ungap(r["cons_y"])
        if ycols:
            assert y[r["begin_y"] - 1:r["begin_y"] - 1 + len(ycols)] == ycols, (x, y, sc, r)
        else:
            assert r["pos"] == 0 and r["cigar"] == "%dI" % len(x)


def _fit_values(x, y, sc):
    """Brute force: the best value, per end column, of every alignment of ALL of x to a substring of y (possibly empty)."""
    match, mismatch, go, ge = sc
    m, n = len(x), len(y)
    best = {}

    def grow(i, j, last, val):
        # forward from (i, j): i letters of x and columns up to j consumed
        if i == m:
            if j >= 1:
                best[j] = max(best.get(j, -1e18), val)
            # a trailing gap in x ('-' against y letters) can only lower the value at a later column: still enumerated below
        if i < m and j < n:
            grow(i + 1, j + 1, "M", val + (match if x[i] == y[j] else mismatch))
        if j < n and i > 0:                                          # '-' against y[j] (not in front of x: the flank is free)
            grow(i, j + 1, "E", val - (ge if last == "E" else go))
        if i < m:
            grow(i + 1, j, "F", val - (ge if last == "F" else go))

    for j0 in range(n + 1):
        grow(0, j0, "M", 0.0)
    return best


def test_brute_force_on_tiny_inputs():
    rng = np.random.default_rng(17)
    for k in range(60):
        m, n = int(rng.integers(1, 5)), int(rng.integers(1, 6))
        x = "".join("AC"[v] for v in rng.integers(0, 2, m))
        y = "".join("AC"[v] for v in rng.integers(0, 2, n))
        sc = SCORINGS[k % len(SCORINGS)]
        H = er.matrices(x, y, *sc)[0]
        best = _fit_values(x, y, sc)
        for j in range(1, n + 1):
            assert H[m, j] == best[j], (x, y, sc, j, H[m, j], best[j])


def test_junk_in_front_is_one_run_in_column_zero():
    # mismatch -10: five letters of junk in front of the copy are cheaper as one gap of rows than as mismatches, and the window
    # starts at the copy, so the gap lies in column 0
    y = "ACGTTGCAAGGCTTAC"
    x = "TTTTT" + y[:12]
    r = er.trace(x, y + "GG", 1, -10, 4, 1)
    assert r["score"] == 12 - (4 + 4) and r["cigar"] == "5I12M" and r["begin_y"] == 1 and r["end_y"] == 12
    # all of x against nothing it matches: one run of rows, no letter of y, pos 0 ... or mismatches where they are cheaper
    r = er.trace("AAAA", "CCCCCC", 1, -10, 4, 1)
    assert (r["score"], r["end_y"], r["cigar"], r["pos"]) == (-7, 1, "4I", 0)
    r = er.trace("AAAA", "CCCCCC", 3, -1, 5, 1)
    assert (r["score"], r["end_y"], r["cigar"], r["pos"]) == (-4, 4, "4M", 1)


def test_window_lemma_L19():
    clamped = unclamped = negative = 0
    for x, y, sc in _random_problems(300, 21, mmax=10, nmax=90):
        full = er.trace(x, y, *sc)
        win, cl, corner = er.window_trace(x, y, full["score"], full["end_y"], *sc)
        assert corner == full["score"], (x, y, sc)
        assert win == full, (x, y, sc, win, full)
        clamped += cl
        unclamped += not cl
        negative += full["score"] < 0
    assert clamped > 30 and unclamped > 30 and negative > 30
    # every cell of row m is a legitimate end cell of the lemma, not only the best one
    for x, y, sc in _random_problems(100, 23, mmax=8, nmax=60):
        H, E, F, S = er.matrices(x, y, *sc)
        for c in range(1, len(y) + 1, 7):
            cx, cy, pos = er.walk(x, y, H, E, F, S, len(x), c, sc[2])
            win, _, corner = er.window_trace(x, y, H[len(x), c], c, *sc)
            assert corner == H[len(x), c] and (win["cons_x"], win["cons_y"], win["pos"]) == (cx, cy, pos), (x, y, sc, c)
