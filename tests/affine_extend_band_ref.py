"""The checker of the anchored seed extension inside a diagonal band (mi355_sw_affine_extend_run_band / _trace_band): a restatement
of the model of include/mi355_sw.h.  Only the cells with

    lo <= j - i <= hi          i the letters of x, j the columns of y consumed from the anchor (0,0); lo <= 0 <= hi

are part of the matrix; outside H = E = F = -inf (there is no floor, so it is -inf and not 0).  Inside

    E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)
    F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)
    H(i,j) = max(H(i-1,j-1) + s, E(i,j), F(i,j))
    H(0,0) = 0,   H(0,j) = E(0,j) = -(o + (j-1) e) for in-band j >= 1,   H(i,0) = F(i,0) = -(o + (i-1) e) for in-band i >= 1

twice — plain loops (`matrices_loops`) and one numpy operation per anti-diagonal (`matrices`) — then `best` (the first maximum of H
over the in-band cells in column-major order, as lengths), `to_end` (the maximum of row m over its in-band columns 0..n at the
smallest column; (-inf, -1) where the band misses row m: unreachable), `walk` (the anchored rule of tests/affine_extend_ref.py: an
equality with -inf never holds) and `trace`, the dict the device must return.  `path_cells` lists the cell of every emitted letter
pair or gap letter, `clip` is the host's window clip.  A backward pair is the forward model on both strings reversed, under the same
band.  Scores are integers, so every comparison is exact.  No project code; tests/test_affine_extend_band_ref.py pins it."""
import numpy as np

from tests.affine_extend_ref import _scores, walk  # noqa: F401
from tests.affine_trace_ref import _b, cigar, rescore  # noqa: F401  (cigar and rescore: for the tests)

NINF = float("-inf")


def in_band(i, j, lo, hi):
    return lo <= j - i <= hi


def reachable(m, n, lo):
    """Row m holds an in-band cell of columns 0..n."""
    return lo <= n - m


def clip(m, n, hi):
    """Columns of the window that hold an in-band cell: those beyond m + hi are out of band in every row."""
    return min(n, m + min(hi, n))


def _borders(m, n, lo, hi, go, ge):
    assert lo <= 0 <= hi
    H = np.full((m + 1, n + 1), NINF)
    E = np.full((m + 1, n + 1), NINF)
    F = np.full((m + 1, n + 1), NINF)
    H[0, 0] = 0.0
    for i in range(1, m + 1):
        if in_band(i, 0, lo, hi):
            H[i, 0] = F[i, 0] = -(go + (i - 1) * ge)
    for j in range(1, n + 1):
        if in_band(0, j, lo, hi):
            H[0, j] = E[0, j] = -(go + (j - 1) * ge)
    return H, E, F


def matrices_loops(x, y, lo, hi, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(H, E, F, S), each [m + 1, n + 1], cell by cell."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    go, ge = float(gap_open), float(gap_extend)
    S = _scores(x, y, match, mismatch, lut)
    H, E, F = _borders(m, n, lo, hi, go, ge)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if not in_band(i, j, lo, hi):
                continue
            E[i, j] = max(E[i, j - 1] - ge, H[i, j - 1] - go)
            F[i, j] = max(F[i - 1, j] - ge, H[i - 1, j] - go)
            H[i, j] = max(H[i - 1, j - 1] + S[i, j], E[i, j], F[i, j])
    return H, E, F, S


def matrices(x, y, lo, hi, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(H, E, F, S) as matrices_loops, one vector operation per anti-diagonal."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    go, ge = float(gap_open), float(gap_extend)
    S = _scores(x, y, match, mismatch, lut)
    H, E, F = _borders(m, n, lo, hi, go, ge)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        keep = (j - i >= lo) & (j - i <= hi)
        i, j = i[keep], j[keep]
        if not len(i):
            continue
        e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
        f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
        E[i, j] = e
        F[i, j] = f
        H[i, j] = np.maximum(H[i - 1, j - 1] + S[i, j], np.maximum(e, f))
    return H, E, F, S


def best(H):
    """(score, end_x, end_y) of the best extension: the first maximum over the in-band cells in column-major order, as lengths."""
    top = float(H.max())
    j = int(np.nonzero((H == top).any(axis=0))[0][0])
    i = int(np.nonzero(H[:, j] == top)[0][0])
    return top, i, j


def to_end(H):
    """(to_end_score, to_end_y): the maximum of row m over its in-band columns and the smallest such column; (-inf, -1): none."""
    row = H[H.shape[0] - 1, :]
    top = float(row.max())
    if top == NINF:
        return NINF, -1
    return top, int(np.nonzero(row == top)[0][0])


_to_end = to_end                                           # (trace has a parameter of that name)


def path_cells(cons_x, cons_y, i, j):
    """The cell each emitted letter pair or gap letter lies on, walking the strings from the traced cell (i, j) to the anchor."""
    cells = []
    for a, b in zip(cons_x, cons_y):
        cells.append((i, j))
        if a != "-":
            i -= 1
        if b != "-":
            j -= 1
    assert (i, j) == (0, 0), (i, j)
    return cells


def locate(x, y, lo, hi, backward=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=matrices):
    """dict(score, end_x, end_y, to_end_score, to_end_y): what mi355_sw_affine_extend_run_band must return."""
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    H = mats(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)[0]
    s, i, j = best(H)
    ts, tj = to_end(H)
    return dict(score=s, end_x=i, end_y=j, to_end_score=ts, to_end_y=tj)


def trace(x, y, lo, hi, backward=False, to_end=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=matrices):
    """dict(score, end_x, end_y, pos, cons_x, cons_y, cigar, to_end_score, to_end_y) of the traced alignment: the best extension, or with
    to_end the one that ends in (m, to_end_y) — an empty alignment of score -inf where the band cannot reach row m."""
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    H, E, F, S = mats(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)
    ts, tj = _to_end(H)
    if to_end and tj < 0:
        return dict(score=NINF, end_x=0, end_y=0, pos=0, cons_x="", cons_y="", cigar="", to_end_score=ts, to_end_y=tj)
    s, i, j = (ts, len(x), tj) if to_end else best(H)
    cx, cy = walk(x, y, H, E, F, S, i, j, gap_open)
    return dict(score=s, end_x=i, end_y=j, pos=1 if j > 0 else 0, cons_x=cx, cons_y=cy,
                cigar=cigar(cx[::-1], cy[::-1]) if backward else cigar(cx, cy), to_end_score=ts, to_end_y=tj)
