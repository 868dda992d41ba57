"""The checker of the end-to-end ("fit", "glocal") mode of the affine pairs calls: a restatement of the model of include/mi355_sw.h

    E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)
    F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)
    H(i,j) = max(H(i-1,j-1) + s, E(i,j), F(i,j))                        no zero floor
    H(0,j) = 0, E(0,j) = F(0,j) = -inf   for j = 0..n                   the window's flanks are free
    H(i,0) = F(i,0) = -(o + (i-1) e), E(i,0) = -inf   for i >= 1

twice — three plain loops (`matrices_loops`) and one numpy operation per anti-diagonal (`matrices`) — then score / end column (the
smallest column of the maximum of row m), the walk by the header's rule over the full matrices, and `trace`, the dict the device
must return.  `window_trace` restates lemma L19: the same walk over the columns (c - W, c] behind the model's own
column-0 border.  Scores are integers, so every comparison is exact.  `cigar`, `rescore` and the byte helpers are those of
tests/affine_trace_ref.py.  No project code; tests/test_affine_e2e_ref.py pins it."""
import math

import numpy as np

from tests.affine_trace_ref import NEG, _b, _table, cigar, rescore  # noqa: F401  (cigar and rescore: for the tests)


def _scores(x, y, match, mismatch, lut):
    m, n = len(x), len(y)
    S = np.zeros((m + 1, n + 1))
    if m and n:
        S[1:, 1:] = _table(match, mismatch, lut)[x.astype(np.intp)[:, None], y.astype(np.intp)[None, :]]
    return S


def _borders(m, n, go, ge):
    H = np.zeros((m + 1, n + 1))
    E = np.full((m + 1, n + 1), NEG)
    F = np.full((m + 1, n + 1), NEG)
    for i in range(1, m + 1):
        H[i, 0] = F[i, 0] = -(go + (i - 1) * ge)
    return H, E, F


def matrices_loops(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(H, E, F, S), each [m + 1, n + 1], cell by cell."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    go, ge = float(gap_open), float(gap_extend)
    S = _scores(x, y, match, mismatch, lut)
    H, E, F = _borders(m, n, go, ge)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            E[i, j] = max(E[i, j - 1] - ge, H[i, j - 1] - go)
            F[i, j] = max(F[i - 1, j] - ge, H[i - 1, j] - go)
            H[i, j] = max(H[i - 1, j - 1] + S[i, j], E[i, j], F[i, j])
    return H, E, F, S


def matrices(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(H, E, F, S) as matrices_loops, one vector operation per anti-diagonal."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    go, ge = float(gap_open), float(gap_extend)
    S = _scores(x, y, match, mismatch, lut)
    H, E, F = _borders(m, n, go, ge)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
        f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
        E[i, j] = e
        F[i, j] = f
        H[i, j] = np.maximum(H[i - 1, j - 1] + S[i, j], np.maximum(e, f))
    return H, E, F, S


def end_cell(H):
    """(score, m, smallest column 1..n that holds the maximum of row m); (0, 0, 0) without rows or without columns."""
    m, n = H.shape[0] - 1, H.shape[1] - 1
    if m < 1 or n < 1:
        return 0.0, 0, 0
    row = H[m, 1:]
    best = float(row.max())
    return best, m, int(np.nonzero(row == best)[0][0]) + 1


def walk(x, y, H, E, F, S, i, j, gap_open, column0_is_border=True):
    """The rule from state M at (i, j): (reversed cons_x, reversed cons_y, pos).  Stops in row 0 only.  column0_is_border=False:
    column 0 is the edge of an unclamped window, and arriving there below row 0 raises AssertionError."""
    x, y = _b(x), _b(y)
    go = float(gap_open)
    cx, cy = [], []
    pos, state = 0, "M"
    while True:
        if state == "M":
            if i == 0:
                break
            if j == 0:
                assert column0_is_border, "the walk left an unclamped window"
                state = "F"
            elif H[i, j] == H[i - 1, j - 1] + S[i, j]:
                cx.append(chr(x[i - 1]))
                cy.append(chr(y[j - 1]))
                pos = j
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                assert H[i, j] == F[i, j]
                state = "F"
        elif state == "E":
            cx.append("-")
            cy.append(chr(y[j - 1]))
            pos = j
            if E[i, j] == H[i, j - 1] - go:
                state = "M"
            j -= 1
        else:
            cx.append(chr(x[i - 1]))
            cy.append("-")
            if F[i, j] == H[i - 1, j] - go:
                state = "M"
            i -= 1
    return "".join(cx), "".join(cy), pos


def locate(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(score, end_x, end_y)."""
    return end_cell(matrices(x, y, match, mismatch, gap_open, gap_extend, lut)[0])


def _result(score, i, j, cx, cy, pos):
    bx = 1 if i > 0 else 0
    return dict(score=score, end_x=i, end_y=j, begin_x=bx, begin_y=pos, pos=pos, cons_x=cx, cons_y=cy, cigar=cigar(cx, cy))


def trace(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=matrices):
    """dict(score, end_x, end_y, begin_x, begin_y, pos, cons_x, cons_y, cigar) of x against y: what the device must return."""
    H, E, F, S = mats(x, y, match, mismatch, gap_open, gap_extend, lut)
    score, i, j = end_cell(H)
    cx, cy, pos = walk(x, y, H, E, F, S, i, j, gap_open) if i > 0 else ("", "", 0)
    return _result(score, i, j, cx, cy, pos)


def window_columns(m, score, smax, gap_extend):
    """W of lemma L19: m + ceil((max(smax, 0) m - score) / e) + 2."""
    return m + int(math.ceil(max(0.0, max(float(smax), 0.0) * m - float(score)) / float(gap_extend))) + 2


def window_trace(x, y, score, c, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, W=None):
    """Lemma L19: the walk from (m, c) over the columns (c - W, c] of y alone, behind the model's own column-0 border — the window
    is clamped at column 1 where W >= c.  Returns (result dict with pos in the coordinates of y, clamped, corner value); the walk
    reaching local column 0 of an unclamped window raises AssertionError, as the device reports status 1."""
    xb, yb = _b(x), _b(y)
    m = len(xb)
    if W is None:
        tab = _table(match, mismatch, lut)
        smax = float(tab[xb.astype(np.intp)[:, None], yb.astype(np.intp)[None, :]].max()) if m and len(yb) else 0.0
        W = window_columns(m, score, smax, gap_extend)
    clamped = W >= c
    nw = c if clamped else W
    wl = c - nw
    yw = yb[wl:c]
    H, E, F, S = matrices(xb, yw, match, mismatch, gap_open, gap_extend, lut)
    i, j = m, nw
    cx, cy, pos = walk(xb, yw, H, E, F, S, i, j, gap_open, column0_is_border=clamped)
    return _result(float(H[m, nw]), m, c, cx, cy, pos + wl if pos else 0), clamped, float(H[m, nw])
