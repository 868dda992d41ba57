"""Lemma L20 of DESIGN.md §3.3 — what the thin stage of the prefix filter rests on — checked on full matrices of the oracle (no GPU),
and the numpy emulation of the stage (tests/prefix_thin.py) on hand-built cases.

For a read of m rows with an exact score B0 <= B above smax (m - P) and above smax P2, every optimal alignment crosses rows P and P2;
with c / c2 the columns of its last cells in those rows, k the horizontal steps between them and c' = c + k:
  (1) H(P, c) >= thr = B0 - smax (m - P), and H(P, c') >= thr as well: row P flags the sub-chunk of c';
  (2) c' <= c2 <= c' + (P2 - P) <= c' + W12, W12 = (P2 - P) + floor(smax (P2 - P) / g) — the window of the thin stage;
  (3) H(P2, c2) >= thr2 = B0 - smax (m - P2).
c2 <= c + W12 holds for the path's own crossing only while k <= smax (P2 - P) / g; a longer gap between the two rows is paid for by the
rows above P, and then it is the flag at c', not the one at c, whose window holds c2 (test_gap_longer_than_the_rows_between_pay_for)."""
import numpy as np
import pytest

from oracle import binding as ob
from prefix_cascade import Read
from prefix_filter import LAG
from prefix_thin import P2, bound2, emulate_pass, geometry, item_values, item_window
from row_sampled_fold import SUB

SCORINGS = [(3.0, -3.0, 2.0), (1.0, -1.0, 4.0), (5.0, -4.0, 1.0)]


def _paths(H, x, y, i, j, scoring, prefer):
    """One optimal path into cell (i, j), as the list of its cells from the end backwards; `prefer` orders the three moves."""
    match, mismatch, gap = scoring
    cells = []
    while H[i, j] > 0:
        cells.append((i, j))
        s = match if x[i - 1] == y[j - 1] else mismatch
        moves = {"d": (H[i - 1, j - 1] + s == H[i, j], i - 1, j - 1), "l": (H[i, j - 1] - gap == H[i, j], i, j - 1),
                 "u": (H[i - 1, j] - gap == H[i, j], i - 1, j)}
        for mv in prefer:
            ok, pi, pj = moves[mv]
            if ok:
                i, j = pi, pj
                break
        else:
            raise AssertionError("no predecessor")
    return cells


def _check(x, y, P, scoring, slacks=(0,)):
    """The three statements for every optimal end cell of x against y, three paths each; returns (the largest c2 - c seen, the
    number of (B0, end cell) pairs that met the lemma's conditions and were checked)."""
    match, mismatch, gap = scoring
    m = len(x)
    H = ob.fill(x, y, ob.F32, match, mismatch, gap).astype(np.float64)
    B = H.max()
    g = geometry(m, P, match, gap)
    widest = checked = 0
    for below in slacks:
        B0 = B - below
        if not (B0 > match * (m - P) and B0 > match * P2):
            continue
        thr, thr2 = B0 - match * (m - P), B0 - match * (m - P2)
        for i, j in zip(*np.nonzero(H == B)):
            assert i > P2, "an optimal alignment ends in row %d, not below row P2" % i
            checked += 1
            for prefer in ("dlu", "lud", "udl"):
                cells = _paths(H, x, y, int(i), int(j), scoring, prefer)
                c = max(cj for ci, cj in cells if ci == P)
                c2 = max(cj for ci, cj in cells if ci == P2)
                k = sum(1 for (ai, aj), (bi, bj) in zip(cells, cells[1:]) if ai == bi and P < ai <= P2)
                assert H[P, c] >= thr and H[P2, c2] >= thr2, (P, c, c2, H[P, c], thr, H[P2, c2], thr2)
                cp = c + k
                assert cp <= c2 <= cp + (P2 - P) <= cp + g["W12"] and H[P, cp] >= thr, (c, k, c2, H[P, cp], thr)
                # the window of the sub-chunk that row P flags for c' (0-based column c' - 1) holds c2
                s = (cp - 1) // SUB
                assert s * SUB - LAG <= cp - 1 and c2 - 1 < (s + 1) * SUB + g["W12"]
                widest = max(widest, c2 - c)
    return widest, checked


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("P", [22, 26])
@pytest.mark.parametrize("m", [60, 150])
def test_lemma_on_full_matrices(m, P, scoring):
    """Noisy copies of a read in a random reference: substitutions, and gaps of both kinds in the rows around P and P2."""
    rng = np.random.default_rng(100 * m + P + int(scoring[0]))
    done = []
    for trial in range(6):
        x = bytes(rng.choice(list(b"ACGT"), m).astype(np.uint8))
        copy = bytearray(x)
        for _ in range(trial):                                       # substitutions anywhere
            at = int(rng.integers(0, m))
            copy[at] = ord("A") if copy[at] != ord("A") else ord("C")
        if trial % 2:                                                # a deletion and an insertion between rows P and P2
            del copy[P + 3]
            copy[P + 7:P + 7] = b"T"
        y = bytes(rng.choice(list(b"ACGT"), 700).astype(np.uint8)) + bytes(copy) + bytes(rng.choice(list(b"ACGT"), 500).astype(np.uint8))
        done.append(_check(x, y, P, scoring, slacks=(0, scoring[0], 2 * scoring[0]))[1])
    assert done == [3] * 6, done                                     # (no trial is vacuous: one end cell each, checked at all three B0)


def _with_gap(rng, m, at_row, k):
    """(x, y): x over G / T, y over A / C with a copy of x that has k extra columns (A) behind row at_row."""
    x = bytes(rng.choice(list(b"GT"), m).astype(np.uint8))
    pad = bytes(rng.choice(list(b"AC"), 600).astype(np.uint8))
    return x, pad + x[:at_row] + b"A" * k + x[at_row:] + pad


def test_crossing_at_the_end_of_the_window():
    """3 / -3 / 2, P = 26: 18 gap columns behind row 27 are what the 12 rows between P and P2 can pay for, c2 = c + W12 exactly."""
    scoring, P = SCORINGS[0], 26
    x, y = _with_gap(np.random.default_rng(5), 150, 27, 18)
    assert geometry(150, P, 3.0, 2.0)["W12"] == 30
    assert _check(x, y, P, scoring) == (30, 1)


def test_gap_longer_than_the_rows_between_pay_for():
    """35 gap columns behind row 27 cost 70, which rows 1 .. 27 (81) pay: B = 380 > 372.  c2 = c + 47 lies outside the window of the
    flag at c, and inside the window of the flag at c' = c + 35 (row P decays along the gap: 78 - 70 = 8 = thr)."""
    scoring, P = SCORINGS[0], 26
    x, y = _with_gap(np.random.default_rng(6), 150, 27, 35)
    assert ob.score_only(x, y, ob.F32, *scoring) == 380.0
    assert _check(x, y, P, scoring) == (47, 1)


def test_own_columns_start_63_in_front_of_the_sub_chunk():
    """A copy of the read's first P2 letters whose last column is s SUB - 63 (0-based) shows in the item's first value; one column
    further left it is outside the own columns and shows nowhere."""
    scoring, P, s = SCORINGS[0], 26, 3
    rng = np.random.default_rng(7)
    x = bytes(rng.choice(list(b"GT"), 150).astype(np.uint8))
    for shift, seen in ((0, True), (1, False)):
        y = bytearray(rng.choice(list(b"AC"), 6 * SUB).astype(np.uint8))
        end = s * SUB - LAG - shift                                  # 0-based column of the copy's last letter
        y[end - P2 + 1:end + 1] = x[:P2]
        vals = item_values(x, bytes(y), s, P, scoring)
        assert len(vals) == 3 and (vals[0] == 3.0 * P2) == seen and max(vals[1:]) < 3.0 * P2, (shift, vals)
    assert item_window(6 * SUB, s, 30, 128) == (s * SUB - 64 - 128, s * SUB - 63, (s + 1) * SUB + 30)
    assert item_window(300, 0, 30, 128) == (0, 0, 286) and item_window(300, 1, 30, 128) == (64, 193, 300)


def test_score_at_the_bound_of_P2_is_not_thinned():
    """m = 60, P = 26: a read is certified from B0 > 102 and thinned only from B0 > smax P2 = 114.  39 matching letters (117) are
    thinned, 38 (114) are not.  The copy crosses row P two columns in front of a sub-chunk's end and row P decays into the next: two
    flags, over a cap of one.  Row P2 reaches its own threshold in both (twelve gaps down from row P leave 54 of 78): the read that is
    thinned offends after the stage, the other one before it."""
    scoring, R = SCORINGS[0], 13
    rng = np.random.default_rng(8)
    core = bytes(rng.choice(list(b"GT"), 39).astype(np.uint8))
    y = bytes(rng.choice(list(b"AC"), 3 * SUB - 28).astype(np.uint8)) + core + bytes(rng.choice(list(b"AC"), 500).astype(np.uint8))
    assert bound2(60, 3.0) == 114.0
    for letters, thinned in ((39, True), (38, False)):
        r = Read(core[:letters] + b"N" * (60 - letters), y, scoring, (R,))
        got = emulate_pass([r], R, 1)
        e = got["reads"][0]
        assert e["B0"] == 3.0 * letters and e["thinned"] == thinned and len(e["flagged"]) == 2, e
        assert e["why"] == ("over the cap after thinning" if thinned else "over the cap"), e   # (row P2 keeps both: 78 - 12 gaps down)
        assert got["thinned"] == (1 if thinned else 0) and (got["items"] > 0) == thinned


def test_flow_case_stays_clear_of_the_caps():
    """The batch of tests/test_gpu_prefix_thin_flow.py: no drawn read's flag count, at any height that certifies it, lies within a
    factor of two of query_flag_cap or of a thin cap; the planted reads draw one flag per decoy and one per copy that shares their prefix."""
    from prefix_thin_flow_case import DECOYS, HEIGHTS, SCORING, build, clear_of_the_caps, flag_counts
    case = build()
    for k, r in enumerate(case["state"]):
        for R, flags in flag_counts(r).items():
            assert clear_of_the_caps(flags), (k, R, flags)
    for x in [case["stays_over"]] + case["family"]:
        flags = flag_counts(Read(x, case["y"], SCORING, HEIGHTS))
        own = x == case["stays_over"]
        assert len(DECOYS) + (1 if own else len(case["family"])) <= flags[13] < 235 and clear_of_the_caps(flags[13]), flags
        # (row P2 over the range: about what survives the thin stage — everything of (b), the own copy of (a))
        assert (flags[19] == len(DECOYS) + 1) if own else (1 <= flags[19] <= 3), flags
