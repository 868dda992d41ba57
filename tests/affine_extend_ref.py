"""The checker of the anchored seed extension of the affine pairs calls (mi355_sw_affine_extend_run / _trace): a restatement of the
model of include/mi355_sw.h

    E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)
    F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)
    H(i,j) = max(H(i-1,j-1) + s, E(i,j), F(i,j))                          no zero floor
    H(0,0) = 0
    H(0,j) = E(0,j) = -(o + (j-1) e), F(0,j) = -inf   for j >= 1          the anchor is fixed: a flank is a gap
    H(i,0) = F(i,0) = -(o + (i-1) e), E(i,0) = -inf   for i >= 1

twice — plain loops (`matrices_loops`) and one numpy operation per anti-diagonal (`matrices`) — then `best` (the first maximum of H
over ALL cells, (0,0) included, in column-major order, reported as lengths), `to_end` (the maximum of row m over columns 0..n, the
smallest column), `walk` (the header's rule from state M at a cell down to (0,0): diagonal over E over F, opening over extending;
only E moves in row 0, only F moves in column 0) and `trace`, the dict the device must return.  A backward pair is the forward model
on both strings reversed: `trace` reverses its inputs itself, and the strings of a backward pair therefore read left to right in the
original strings.  Scores are integers, so every comparison is exact.  `cigar`, `rescore` and the byte helpers are those of
tests/affine_trace_ref.py.  No project code; tests/test_affine_extend_ref.py pins it."""
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
    for j in range(1, n + 1):
        H[0, j] = E[0, j] = -(go + (j - 1) * ge)
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


def best(H):
    """(score, end_x, end_y) of the best extension: the first maximum over all cells in column-major order, as lengths.  Cell (0,0)
    = 0 competes and column 0 wins every tie, so score 0 comes with 0 / 0."""
    top = float(H.max())
    j = int(np.nonzero((H == top).any(axis=0))[0][0])
    i = int(np.nonzero(H[:, j] == top)[0][0])
    return top, i, j


def to_end(H):
    """(to_end_score, to_end_y): the maximum of row m over columns 0..n and the smallest such column."""
    row = H[H.shape[0] - 1, :]
    top = float(row.max())
    return top, int(np.nonzero(row == top)[0][0])


_to_end = to_end                                           # (trace has a parameter of that name)


def walk(x, y, H, E, F, S, i, j, gap_open):
    """The rule from state M at (i, j) down to (0, 0): (cons_x, cons_y), from the far end to the anchor."""
    x, y = _b(x), _b(y)
    go = float(gap_open)
    cx, cy = [], []
    state = "M"
    while True:
        if state == "M":
            if i == 0 and j == 0:
                break
            if i == 0:
                state = "E"
            elif j == 0:
                state = "F"
            elif H[i, j] == H[i - 1, j - 1] + S[i, j]:
                cx.append(chr(x[i - 1]))
                cy.append(chr(y[j - 1]))
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                assert H[i, j] == F[i, j]
                state = "F"
        elif state == "E":
            cx.append("-")
            cy.append(chr(y[j - 1]))
            if E[i, j] == H[i, j - 1] - go:
                state = "M"
            j -= 1
        else:
            cx.append(chr(x[i - 1]))
            cy.append("-")
            if F[i, j] == H[i - 1, j] - go:
                state = "M"
            i -= 1
    return "".join(cx), "".join(cy)


def locate(x, y, backward=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=matrices):
    """dict(score, end_x, end_y, to_end_score, to_end_y): what mi355_sw_affine_extend_run must return."""
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    H = mats(x, y, match, mismatch, gap_open, gap_extend, lut)[0]
    s, i, j = best(H)
    ts, tj = to_end(H)
    return dict(score=s, end_x=i, end_y=j, to_end_score=ts, to_end_y=tj)


def trace(x, y, backward=False, to_end=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=matrices):
    """dict(score, end_x, end_y, pos, cons_x, cons_y, cigar, to_end_score, to_end_y) of the traced alignment of x against y: the best
    extension, or with to_end the alignment that ends in (m, to_end_y).  The CIGAR is in reading order for both directions."""
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    H, E, F, S = mats(x, y, match, mismatch, gap_open, gap_extend, lut)
    ts, tj = _to_end(H)
    s, i, j = (ts, len(x), tj) if to_end else best(H)
    cx, cy = walk(x, y, H, E, F, S, i, j, gap_open)
    return dict(score=s, end_x=i, end_y=j, pos=1 if j > 0 else 0, cons_x=cx, cons_y=cy,
                cigar=cigar(cx[::-1], cy[::-1]) if backward else cigar(cx, cy), to_end_score=ts, to_end_y=tj)
