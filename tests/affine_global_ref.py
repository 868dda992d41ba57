"""The checker of the global alignment between two anchors (mi355_sw_affine_global_run / _trace): the anchored model of
include/mi355_sw.h, whose answer is the corner H(m, n).  The matrices and the walk are those of tests/affine_extend_ref.py and, under a
band lo <= j - i <= hi, of tests/affine_extend_band_ref.py; what this file adds is written from the header's text:

    score = H(m, n), end_x = m, end_y = n; the walk starts in state M at (m, n)
    m = 0, n = 0: score 0, empty strings;  m >= 1, n = 0: -(o + (m-1) e), x against m '-';  m = 0, n >= 1: -(o + (n-1) e), n '-' against y
    under a band the corner is reachable exactly when lo <= n - m <= hi; else score -inf, end 0 / 0, pos 0, empty strings

A backward pair is the forward model on both strings reversed; its strings read left to right in the original strings and the CIGAR is
in reading order for both directions.  Scores are integers, so every comparison is exact.  No project code;
tests/test_affine_global_ref.py pins it."""
from tests import affine_extend_band_ref as BR
from tests import affine_extend_ref as ER
from tests.affine_trace_ref import _b, cigar, rescore  # noqa: F401  (cigar and rescore: for the tests)

NINF = float("-inf")


def reachable(m, n, lo=None, hi=None):
    return lo is None or lo <= n - m <= hi


def _gap(g, gap_open, gap_extend):
    return 0.0 if g < 1 else -(float(gap_open) + (g - 1) * float(gap_extend))


def _mats(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut):
    if lo is None:
        return ER.matrices(x, y, match, mismatch, gap_open, gap_extend, lut)
    return BR.matrices(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)


def score(x, y, lo=None, hi=None, backward=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """What mi355_sw_affine_global_run must return for the pair (x, y), under the band [lo, hi] where one is given."""
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    m, n = len(x), len(y)
    assert (lo is None) == (hi is None) and (lo is None or lo <= 0 <= hi)
    if not reachable(m, n, lo, hi):
        return NINF
    if m == 0 or n == 0:
        return _gap(m + n, gap_open, gap_extend)
    return float(_mats(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)[0][m, n])


def trace(x, y, lo=None, hi=None, backward=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """dict(score, end_x, end_y, pos, cons_x, cons_y, cigar): what mi355_sw_affine_global_trace must return."""
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    m, n = len(x), len(y)
    assert (lo is None) == (hi is None) and (lo is None or lo <= 0 <= hi)
    if not reachable(m, n, lo, hi):
        return dict(score=NINF, end_x=0, end_y=0, pos=0, cons_x="", cons_y="", cigar="")
    if m == 0 or n == 0:
        s = _gap(m + n, gap_open, gap_extend)
        cx = "".join(chr(c) for c in x[::-1]) if m else "-" * n
        cy = "".join(chr(c) for c in y[::-1]) if n else "-" * m
    else:
        H, E, F, S = _mats(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)
        s = float(H[m, n])
        cx, cy = ER.walk(x, y, H, E, F, S, m, n, gap_open)
    return dict(score=s, end_x=m, end_y=n, pos=1 if n > 0 else 0, cons_x=cx, cons_y=cy,
                cigar=cigar(cx[::-1], cy[::-1]) if backward else cigar(cx, cy))
