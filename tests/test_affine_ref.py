"""Pins tests/affine_ref.py, the checker of the affine-gap GPU tests (CPU only): at gap_open == gap_extend it is the reference's
linear model and must equal the reference's oracle; its two implementations must agree at gap_open > gap_extend; and it must give
the known answers of two small problems whose best alignment holds one three-letter gap, horizontal in one and vertical in the other."""
import numpy as np
import pytest

from tests import affine_ref

SCORINGS = [(3, -3, 2), (1, -1, 4), (2, 0, 1), (10, -2, 1), (5, -4, 7)]

A = "ACGGTCATGCTA"
B = "GTACCTGAATCG"
# (x, y, end cell): a gap of three columns of y, and a gap of three rows of x
KNOWN = [(A + B, "CCCC" + A + "TTT" + B + "CCCC", (24, 31)),
         (A + "GGG" + B, "CCCC" + A + B + "CCCC", (27, 28))]
KNOWN_SCORES = {(5, 1): 65, (5, 5): 57, (1, 1): 69, (2, 2): 66, (7, 2): 61}      # at 3 / -3


def _letters(rng, n, alpha):
    a = np.frombuffer(alpha, dtype=np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def _pairs(seed, count, mmax=40, nmax=120, gapped=False):
    rng = np.random.default_rng(seed)
    for k in range(count):
        alpha = b"ACGT" if k % 2 == 0 else b"AC"
        m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(1, nmax + 1))
        x, y = _letters(rng, m, alpha), bytearray(_letters(rng, n, alpha))
        if k % 3 == 0 and n >= m:                                   # a copy of x in y, so that long alignments occur
            at = int(rng.integers(0, n - m + 1))
            y[at:at + m] = x
        elif gapped and k % 3 == 1 and n >= m + 2 and m >= 8:       # ... with two letters inserted in its middle
            at = int(rng.integers(0, n - m - 1))
            y[at:at + m + 2] = x[:m // 2] + _letters(rng, 2, alpha) + x[m // 2:]
        yield k, x, bytes(y)


def test_linear_case_equals_the_oracle(oracle):
    bad = []
    for k, x, y in _pairs(20261, 300):
        ma, mi, g = SCORINGS[k % len(SCORINGS)]
        exp = oracle.locate(x, y, 0, match=float(ma), mismatch=float(mi), gap=float(g))
        got = affine_ref.locate(x, y, ma, mi, g, g)
        if (float(exp[0]), int(exp[1]), int(exp[2])) != got:
            bad.append((k, exp, got))
    assert not bad, bad[:5]
    # nothing matches: score 0, end 0 / 0 (the oracle's all-zero result)
    assert affine_ref.locate("AAAA", "CCCCCC", 3, -3, 2, 2) == (0.0, 0, 0)
    assert tuple(oracle.locate(b"AAAA", b"CCCCCC", 0)) == (0.0, 0, 0)


def test_both_implementations_agree_under_affine_gaps():
    affine = [(3, -3, 5, 1), (1, -1, 4, 2), (2, 0, 3, 1), (10, -2, 12, 1), (5, -4, 9, 7)]
    bad, differs = [], 0
    for k, x, y in _pairs(77003, 120, mmax=24, nmax=60, gapped=True):
        ma, mi, go, ge = affine[k % len(affine)]
        a = affine_ref.locate(x, y, ma, mi, go, ge)
        b = affine_ref.locate_loops(x, y, ma, mi, go, ge)
        if a != b:
            bad.append((k, a, b))
        differs += a != affine_ref.locate(x, y, ma, mi, go, go)
    assert not bad, bad[:5]
    assert differs > 10, "the inputs must tell affine gaps from linear ones"
    xs = [x for _, x, _ in _pairs(5, 7)]
    y = _letters(np.random.default_rng(9), 90, b"ACGT")
    s, i, j = affine_ref.locate_batch(xs, y, 3, -3, 5, 1)
    assert [(float(s[k]), int(i[k]), int(j[k])) for k in range(7)] == [affine_ref.locate(x, y, 3, -3, 5, 1) for x in xs]


@pytest.mark.parametrize("impl", [affine_ref.locate, affine_ref.locate_loops])
def test_known_answers(impl):
    for x, y, end in KNOWN:
        for (go, ge), score in KNOWN_SCORES.items():
            assert impl(x, y, 3, -3, go, ge) == (float(score), end[0], end[1]), (x, go, ge)
