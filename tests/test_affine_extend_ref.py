"""Pins tests/affine_extend_ref.py, the checker of the anchored seed extension, independently of itself: its two restatements of the
model agree, the borders are the gaps the header states, the strings of every traced pair are worth its score and spell the letters
the lengths name, the score is >= 0 and 0 exactly at end 0 / 0, a window cut at an exact copy of the read gives score = to_end_score =
match * m at (m, m), no anchored alignment beats either score (brute force on tiny inputs), a backward trace is the forward trace of
the reversed inputs, and the recorded pairs of tests/golden/affine_extend_pins.json (both directions, both trace choices, the
degenerate pairs; written once by `python -m tests.test_affine_extend_ref`) still come out.  No GPU and no project code."""
import json
import os

import numpy as np

from tests import affine_extend_ref as xr

SCORINGS = [(3, -3, 5, 1), (2, -1, 3, 1), (1, -1, 2, 2), (5, -4, 10, 3), (1, -10, 4, 1)]
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affine_extend_pins.json")
PIN_FIELDS = ("score", "end_x", "end_y", "pos", "cons_x", "cons_y", "cigar", "to_end_score", "to_end_y")


def _random_problems(count, seed, mmax=20, nmax=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        alpha = np.frombuffer(b"ACGT" if k % 2 == 0 else b"AC", dtype=np.uint8)
        m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(1, nmax + 1))
        x = alpha[rng.integers(0, len(alpha), m)].tobytes()
        y = bytearray(alpha[rng.integers(0, len(alpha), n)].tobytes())
        if k % 4 == 0 and m >= 8 and n >= m + 3:                    # a copy from the anchor on with a 3-column insert
            y[:m + 3] = x[:m // 2] + alpha[rng.integers(0, len(alpha), 3)].tobytes() + x[m // 2:]
        elif k % 4 == 1 and n >= m:                                 # an exact copy at the anchor
            y[:m] = x
        elif k % 4 == 2:                                            # nothing in common: extend nothing
            y = bytearray(b"T" * n) if k % 2 else bytearray(b"N" * n)
        elif n >= m // 2 + 4:                                       # half a copy, then foreign letters: a clip
            y[:m // 2] = x[:m // 2]
        out.append((x.decode(), bytes(y).decode(), SCORINGS[k % len(SCORINGS)]))
    return out


def _kw(sc):
    return dict(match=sc[0], mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])


def test_loops_and_diagonals_agree():
    zero = clipped = 0
    for k, (x, y, sc) in enumerate(_random_problems(300, 5)):
        a, b = xr.matrices_loops(x, y, *sc), xr.matrices(x, y, *sc)
        for u, v in zip(a, b):
            assert np.array_equal(u, v), (x, y, sc)
        for back in (False, True):
            for te in (False, True):
                ra, rb = xr.trace(x, y, back, te, mats=xr.matrices_loops, **_kw(sc)), xr.trace(x, y, back, te, **_kw(sc))
                assert ra == rb, (x, y, sc, back, te)
        r = xr.trace(x, y, **_kw(sc))
        zero += r["score"] == 0
        clipped += 0 < r["end_x"] < len(x)
    assert zero > 30 and clipped > 30


def test_borders_and_degenerate_pairs():
    H, E, F, _ = xr.matrices("ACGT", "ACG", 3, -3, 5, 2)
    assert H[:, 0].tolist() == [0, -5, -7, -9, -11] and F[1:, 0].tolist() == [-5, -7, -9, -11]
    assert H[0].tolist() == [0, -5, -7, -9] and E[0, 1:].tolist() == [-5, -7, -9]
    assert (E[:, 0] < -1e17).all() and (F[0] < -1e17).all()
    for back in (False, True):
        for te in (False, True):
            for y in ("ACGT", ""):
                r = xr.trace("", y, back, te)
                assert [r[f] for f in PIN_FIELDS] == [0, 0, 0, 0, "", "", "", 0, 0]
        r = xr.trace("ACGT", "", back, False, gap_open=5, gap_extend=2)
        assert [r[f] for f in PIN_FIELDS] == [0, 0, 0, 0, "", "", "", -11, 0]
        r = xr.trace("ACGT", "", back, True, gap_open=5, gap_extend=2)
        assert (r["score"], r["end_x"], r["end_y"], r["pos"], r["cons_y"], r["cigar"]) == (-11, 4, 0, 0, "----", "4I")
        assert r["cons_x"] == ("ACGT" if back else "TGCA")


def test_strings_are_worth_the_score_and_spell_the_lengths():
    for x, y, sc in _random_problems(300, 11):
        for back in (False, True):
            xs, ys = (x[::-1], y[::-1]) if back else (x, y)
            for te in (False, True):
                r = xr.trace(x, y, back, te, **_kw(sc))
                assert xr.rescore(r["cons_x"], r["cons_y"], *sc) == r["score"], (x, y, sc, back, te)
                # from the far end to the anchor: reversed in the frame the model runs in
                assert r["cons_x"].replace("-", "")[::-1] == xs[:r["end_x"]] and r["cons_y"].replace("-", "")[::-1] == ys[:r["end_y"]]
                assert r["pos"] == (1 if r["end_y"] else 0)
                if te:
                    assert r["end_x"] == len(x) and (r["score"], r["end_y"]) == (r["to_end_score"], r["to_end_y"])
                else:
                    assert r["score"] >= 0 and (r["score"] == 0) == (r["end_x"] == 0 and r["end_y"] == 0)
                    assert (r["score"] == 0) == (r["end_x"] == 0) == (r["end_y"] == 0)
                    assert r["score"] >= r["to_end_score"]


def test_window_cut_at_an_exact_copy():
    rng = np.random.default_rng(3)
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    for m in (1, 2, 17, 40):
        x = alpha[rng.integers(0, 4, m)].tobytes().decode()
        for tail in ("", "ACGTTGCAAC"):
            for back in (False, True):
                y = (tail + x) if back else (x + tail)
                r = xr.locate(x, y, back, match=3, mismatch=-3, gap_open=5, gap_extend=1)
                assert (r["score"], r["end_x"], r["end_y"], r["to_end_score"], r["to_end_y"]) == (3 * m, m, m, 3 * m, m), (m, tail, back)
                assert xr.trace(x, y, back)["cigar"] == "%dM" % m


def _anchored_alignments(m, n):
    """Every alignment from (0,0) to (i,j) as a list of ops, for all end cells: paths of M / I / D moves."""
    best = {}

    def go(i, j, ops):
        best.setdefault((i, j), []).append(ops)
        if i < m and j < n:
            go(i + 1, j + 1, ops + "M")
        if i < m:
            go(i + 1, j, ops + "I")
        if j < n:
            go(i, j + 1, ops + "D")
    go(0, 0, "")
    return best


def test_brute_force_on_tiny_inputs():
    rng = np.random.default_rng(17)
    alpha = np.frombuffer(b"AC", dtype=np.uint8)
    paths = {}
    for trial in range(40):
        m, n = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        x = alpha[rng.integers(0, 2, m)].tobytes().decode()
        y = alpha[rng.integers(0, 2, n)].tobytes().decode()
        sc = SCORINGS[trial % len(SCORINGS)]
        if (m, n) not in paths:
            paths[(m, n)] = _anchored_alignments(m, n)
        H = xr.matrices(x, y, *sc)[0]
        for (i, j), all_ops in paths[(m, n)].items():
            top = -1e18
            for ops in all_ops:
                a = b = 0
                cx, cy = [], []
                for op in ops:
                    cx.append(x[a] if op != "D" else "-")
                    cy.append(y[b] if op != "I" else "-")
                    a += op != "D"
                    b += op != "I"
                top = max(top, xr.rescore("".join(cx), "".join(cy), *sc))
            assert H[i, j] == top, (x, y, sc, i, j)


def test_backward_is_forward_on_the_reversed_inputs():
    for x, y, sc in _random_problems(100, 23):
        for te in (False, True):
            b, f = xr.trace(x, y, True, te, **_kw(sc)), xr.trace(x[::-1], y[::-1], False, te, **_kw(sc))
            for field in PIN_FIELDS:
                if field != "cigar":
                    assert b[field] == f[field], (field, x, y, sc)
            assert b["cigar"] == xr.cigar(f["cons_x"][::-1], f["cons_y"][::-1])
    # a left extension: the seed sits behind the window; the insert lies where the original strings have it
    y, x = "TTTTACGTACGGACGT", "ACGTACGACGT"
    r = xr.trace(x, y, True, False)
    assert (r["score"], r["end_x"], r["end_y"], r["cigar"]) == (3 * 11 - 5, 11, 12, "7M1D4M")
    assert r["cons_x"].replace("-", "") == x and r["cons_y"] == y[4:]


def pin_cases():
    cases = [("", "ACGT", (3, -3, 5, 1)), ("ACGT", "", (3, -3, 5, 2)), ("", "", (3, -3, 5, 1)), ("AAAA", "CCCCCC", (3, -3, 5, 1)),
             ("AAAA", "CCCCCC", (3, -10, 5, 1)), ("A", "A", (3, -3, 5, 1)), ("ACGTACGTAC", "ACGTACGTAC", (3, -3, 5, 1)),
             ("ACGTACGTACTTTTT", "ACGTACGTACGGGGGGGG", (3, -3, 5, 1)), ("GGGACGTACGT", "ACGTACGT", (1, -10, 4, 1))]
    cases += _random_problems(4, 29)
    out = []
    for x, y, sc in cases:
        for back in (False, True):
            for te in (False, True):
                out.append(dict(x=x, y=y, scoring=list(sc), backward=back, to_end=te))
    return out


def test_pins():
    with open(PINS) as f:
        pins = json.load(f)
    assert len(pins) >= 48
    assert {(p["backward"], p["to_end"]) for p in pins} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(not p["x"] for p in pins) and any(not p["y"] and p["x"] for p in pins)
    for p in pins:
        r = xr.trace(p["x"], p["y"], p["backward"], p["to_end"], **_kw(p["scoring"]))
        assert {f: r[f] for f in PIN_FIELDS} == p["expect"], p


if __name__ == "__main__":
    rows = pin_cases()
    for p in rows:
        r = xr.trace(p["x"], p["y"], p["backward"], p["to_end"], **_kw(p["scoring"]))
        p["expect"] = {f: r[f] for f in PIN_FIELDS}
    with open(PINS, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("wrote %d pins" % len(rows))
