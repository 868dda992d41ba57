"""The checker of the global alignment between two anchors (tests/affine_global_ref.py) is checked before it judges the device (no GPU):
against an independent textbook Gotoh recursion written here, against the enumeration of ALL alignments of tiny pairs, against its own
strings, against the to-end half of the extension checker, under bands, reversed, and on two planted cases."""
import functools
import itertools
import random

import pytest

from tests import affine_extend_band_ref as BR
from tests import affine_extend_ref as ER
from tests import affine_global_ref as G

SCORINGS = [dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0), dict(match=3.0, mismatch=-10.0, gap_open=5.0, gap_extend=1.0),
            dict(match=1.0, mismatch=-1.0, gap_open=1.0, gap_extend=1.0), dict(match=2.0, mismatch=-4.0, gap_open=3.0, gap_extend=3.0)]
NINF = float("-inf")


def _rand(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def gotoh_global(x, y, match, mismatch, gap_open, gap_extend):
    """Textbook three-state global alignment: M ends in a letter pair, X in a letter of x against '-', Y in a letter of y against '-'."""
    o, e = gap_open, gap_extend

    @functools.lru_cache(maxsize=None)
    def f(i, j, st):
        if i == 0 and j == 0:
            return 0.0 if st == "M" else NINF
        if st == "M":
            if i == 0 or j == 0:
                return NINF
            s = match if x[i - 1] == y[j - 1] else mismatch
            return s + max(f(i - 1, j - 1, "M"), f(i - 1, j - 1, "X"), f(i - 1, j - 1, "Y"))
        if st == "X":
            if i == 0:
                return NINF
            return max(f(i - 1, j, "M") - o, f(i - 1, j, "X") - e, f(i - 1, j, "Y") - o)
        if j == 0:
            return NINF
        return max(f(i, j - 1, "M") - o, f(i, j - 1, "Y") - e, f(i, j - 1, "X") - o)

    return max(f(len(x), len(y), st) for st in "MXY")


@pytest.mark.parametrize("sc", SCORINGS)
def test_equals_an_independent_gotoh_recursion(sc):
    rng = random.Random(17)
    sizes = [(m, n) for m in range(13) for n in range(13)] + [(40, 33), (27, 40), (40, 40), (1, 40), (38, 2)]
    for m, n in sizes:
        x, y = _rand(rng, m), _rand(rng, n)
        assert G.score(x, y, **sc) == gotoh_global(x, y, **sc), (x, y)


def _all_alignments(m, n):
    """Every sequence of M / I / D that consumes m letters of x and n of y."""
    if m == 0 and n == 0:
        yield ""
        return
    if m and n:
        for t in _all_alignments(m - 1, n - 1):
            yield t + "M"
    if m:
        for t in _all_alignments(m - 1, n):
            yield t + "I"
    if n:
        for t in _all_alignments(m, n - 1):
            yield t + "D"


def _value(ops, x, y, match, mismatch, gap_open, gap_extend):
    i = j = 0
    total, last = 0.0, "M"
    for op in ops:
        if op == "M":
            total += match if x[i] == y[j] else mismatch
            i, j = i + 1, j + 1
        else:
            total -= gap_extend if op == last else gap_open
            i, j = i + (op == "I"), j + (op == "D")
        last = op
    return total


@pytest.mark.parametrize("sc", SCORINGS)
def test_equals_the_maximum_over_all_alignments(sc):
    paths = {(m, n): list(_all_alignments(m, n)) for m in range(5) for n in range(5)}
    for (m, n), ops in paths.items():
        for x in map("".join, itertools.product("AC", repeat=m)):
            for y in map("".join, itertools.product("AC", repeat=n)):
                assert G.score(x, y, **sc) == max(_value(t, x, y, **sc) for t in ops), (x, y)


@pytest.mark.parametrize("sc", SCORINGS)
def test_strings_hold_both_sequences_and_rescore(sc):
    rng = random.Random(5)
    for _ in range(60):
        m, n = rng.randrange(0, 30), rng.randrange(0, 30)
        x, y = _rand(rng, m), _rand(rng, n)
        for back in (False, True):
            for band in (None, (-6, 6)):
                lo, hi = band if band else (None, None)
                t = G.trace(x, y, lo, hi, backward=back, **sc)
                assert t["score"] == G.score(x, y, lo, hi, backward=back, **sc)
                if t["score"] == NINF:
                    assert not G.reachable(m, n, lo, hi) and (t["end_x"], t["end_y"], t["pos"], t["cons_x"], t["cons_y"]) == (0, 0, 0, "", "")
                    continue
                assert (t["end_x"], t["end_y"], t["pos"]) == (m, n, 1 if n else 0)
                cx, cy = t["cons_x"], t["cons_y"]
                # from the far end to the anchor: reversed for a forward pair, reading order for a backward pair
                assert cx.replace("-", "") == (x if back else x[::-1]) and cy.replace("-", "") == (y if back else y[::-1])
                if cx:
                    assert G.rescore(cx, cy, **sc) == t["score"]
                else:
                    assert t["score"] == 0.0
                if band and cx:
                    xs, ys = (x[::-1], y[::-1]) if back else (x, y)
                    assert all(lo <= j - i <= hi for i, j in BR.path_cells(cx, cy, len(xs), len(ys)))


@pytest.mark.parametrize("sc", SCORINGS)
def test_to_end_is_the_best_global_prefix(sc):
    rng = random.Random(29)
    for _ in range(25):
        m, n = rng.randrange(1, 25), rng.randrange(0, 30)
        x, y = _rand(rng, m), _rand(rng, n)
        ts, tj = ER.to_end(ER.matrices(x, y, **sc)[0]) if n else (G.score(x, "", **sc), 0)
        col = [G.score(x, y[:j], **sc) for j in range(n + 1)]
        assert ts == max(col) and tj == col.index(max(col))
        if n:
            ts, tj = BR.to_end(BR.matrices(x, y, -4, 4, **sc)[0])
            col = [G.score(x, y[:j], -4, 4, **sc) for j in range(n + 1)]
            assert ts == max(col) and tj == (col.index(max(col)) if ts != NINF else -1)


def test_bands():
    rng = random.Random(3)
    sc = SCORINGS[0]
    for _ in range(40):
        m, n = rng.randrange(0, 20), rng.randrange(0, 20)
        x, y = _rand(rng, m), _rand(rng, n)
        # a band that covers the matrix is the unbanded answer
        for lo, hi in ((-m, n), (-m - 3, n + 5)):
            assert G.trace(x, y, lo, hi, **sc) == G.trace(x, y, **sc)
        # a band that misses n - m is unreachable, one that holds it on its edge is not
        d = n - m
        if d > 0:
            assert G.score(x, y, -2, d - 1, **sc) == NINF and G.score(x, y, -2, d, **sc) > NINF
            assert G.trace(x, y, -2, d - 1, **sc)["cons_x"] == ""
        if d < 0:
            assert G.score(x, y, d + 1, 2, **sc) == NINF and G.score(x, y, d, 2, **sc) > NINF
        # a narrower band never scores higher
        if abs(d) <= 2:
            assert G.score(x, y, -2, 2, **sc) <= G.score(x, y, -5, 5, **sc) <= G.score(x, y, **sc)


@pytest.mark.parametrize("sc", SCORINGS)
def test_the_reversed_pair_has_the_same_score(sc):
    rng = random.Random(11)
    for _ in range(40):
        x, y = _rand(rng, rng.randrange(0, 30)), _rand(rng, rng.randrange(0, 30))
        assert G.score(x[::-1], y[::-1], **sc) == G.score(x, y, **sc) == G.score(x, y, backward=True, **sc)


def test_planted_cases():
    # y = A + GGG + B, x = A + B, A ends in 'A' and B starts with 'C'.  All 40 letters of x can match only with the one gap of exactly
    # the three G (moved one place to the left the gap would hold "AGG" and x's last 'A' of A would meet a 'G'; moved to the right, B's
    # 'C' would): 40 matches at 3 and one gap of three letters at 5 + 1 + 1 under 3 / -3 / 5 / 1: 120 - 7 = 113, CIGAR 20M3D20M.
    # Nothing scores higher: n - m = 3 forces at least three gap letters, one run of them is the cheapest, and 40 matches is all of x.
    rng = random.Random(1)
    A, B = _rand(rng, 19) + "A", "C" + _rand(rng, 19)
    x, y = A + B, A + "GGG" + B
    t = G.trace(x, y)
    assert t["score"] == 113.0 and t["cigar"] == "20M3D20M"
    assert G.trace(x, y, backward=True)["cigar"] == "20M3D20M" and G.score(x, y, -2, 2) == NINF and G.score(x, y, 0, 3) == 113.0
    # a window 20 columns too long: the extension stops at column 40 with all 40 matches, the corner pays a gap of 20: it matters
    y2 = x + _rand(rng, 20)
    ts, tj = ER.to_end(ER.matrices(x, y2)[0])
    assert (ts, tj) == (120.0, 40) and G.score(x, y2) == 120.0 - (5.0 + 19.0) and G.score(x, y2) != ts
