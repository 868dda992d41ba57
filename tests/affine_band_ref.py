"""The checker of the banded affine-gap tests: the local Gotoh recurrence of include/mi355_sw.h restricted to a diagonal band

    band_lo <= j - i <= band_hi          i the 1-based row of x, j the 1-based column of y, both bounds signed

    E(i,j) = max(E(i,j-1) - gap_extend, H(i,j-1) - gap_open)
    F(i,j) = max(F(i-1,j) - gap_extend, H(i-1,j) - gap_open)
    H(i,j) = max(0, H(i-1,j-1) + s, E(i,j), F(i,j))           inside the band; H = 0 on the borders that lie in the band
    H = E = F = -inf                                           outside the band: such a cell is not part of the matrix

(numpy, one vector operation per anti-diagonal, all three matrices kept), the first maximum in column-major order among the in-band
cells, and the walk of the header's traceback rule in plain Python over those matrices.  An equality with -inf never holds (a finite
value is never equal to NEG, and NEG absorbs every score added to it), so the walk never leaves the band.  Scores are integers, so
every comparison is exact.  `zero_outside=True` computes the other statement of the model — an out-of-band neighbour holds H = 0,
E = F = -inf — which gives the same in-band cells (tests/test_affine_band_ref.py).

No project code.  tests/test_affine_band_ref.py pins it."""
import numpy as np

NEG = -1.0e18


def _b(s):
    if isinstance(s, (bytes, bytearray)):
        return np.frombuffer(bytes(s), dtype=np.uint8)
    if isinstance(s, np.ndarray):
        return s.astype(np.uint8)
    return np.frombuffer(s.encode("latin-1"), dtype=np.uint8)


def _table(match, mismatch, lut):
    if lut is not None:
        return np.asarray(lut, dtype=np.float64).reshape(256, 256)
    t = np.full((256, 256), float(mismatch))
    t[np.arange(256), np.arange(256)] = float(match)
    return t


def effective_band(m, n, lo, hi):
    """(lo_e, hi_e): the band clipped to the diagonals the matrix has, 1 - m .. n - 1.  lo_e > hi_e: it misses the matrix."""
    return max(int(lo), 1 - m), min(int(hi), n - 1)


def in_band_mask(m, n, lo, hi):
    """[m + 1, n + 1] bool: lo <= j - i <= hi."""
    d = np.arange(n + 1)[None, :] - np.arange(m + 1)[:, None]
    return (d >= lo) & (d <= hi)


def matrices(x, y, lo, hi, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, zero_outside=False):
    """(H, E, F, S, band), each [m + 1, n + 1]; out-of-band cells hold NEG in all three (zero_outside: H = 0 there)."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    go, ge = float(gap_open), float(gap_extend)
    band = in_band_mask(m, n, lo, hi)
    out_h = 0.0 if zero_outside else NEG
    H = np.where(band, 0.0, out_h)
    E = np.full((m + 1, n + 1), NEG)
    F = np.full((m + 1, n + 1), NEG)
    S = np.zeros((m + 1, n + 1))
    if m and n:
        S[1:, 1:] = _table(match, mismatch, lut)[x.astype(np.intp)[:, None], y.astype(np.intp)[None, :]]
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        inb = band[i, j]
        e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
        f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
        h = np.maximum(np.maximum(H[i - 1, j - 1] + S[i, j], 0.0), np.maximum(e, f))
        E[i, j] = np.where(inb, e, NEG)
        F[i, j] = np.where(inb, f, NEG)
        H[i, j] = np.where(inb, h, out_h)
    return H, E, F, S, band


def end_cell(H, band):
    """(score, row, column) of the first maximum in column-major order among the in-band cells, 1-based; zeros when none is positive."""
    Hb = np.where(band, H, NEG)
    Hb[0, :] = NEG
    Hb[:, 0] = NEG
    best = float(Hb.max()) if Hb.size else 0.0
    if not best > 0:
        return 0.0, 0, 0
    cols = np.nonzero((Hb == best).any(axis=0))[0]
    j = int(cols[0])
    i = int(np.nonzero(Hb[:, j] == best)[0][0])
    return best, i, j


def walk(x, y, H, E, F, S, i, j, gap_open):
    """The traceback rule from state M at (i, j): (reversed cons_x, reversed cons_y, pos, the cells of the emitted letters)."""
    x, y = _b(x), _b(y)
    go = float(gap_open)
    cx, cy, cells = [], [], []
    pos, state = 0, "M"
    while True:
        if state == "M":
            if i <= 0 or j <= 0 or H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + S[i, j]:
                cx.append(chr(x[i - 1]))
                cy.append(chr(y[j - 1]))
                cells.append((i, j))
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
            cells.append((i, j))
            pos = j
            if E[i, j] == H[i, j - 1] - go:
                state = "M"
            j -= 1
        else:
            cx.append(chr(x[i - 1]))
            cy.append("-")
            cells.append((i, j))
            if F[i, j] == H[i - 1, j] - go:
                state = "M"
            i -= 1
    return "".join(cx), "".join(cy), pos, cells


def cigar(cons_x, cons_y):
    """Forward run-length string of the reversed pair: M letter pair, I letter of x against '-', D letter of y against '-'."""
    assert len(cons_x) == len(cons_y)
    ops = ["D" if a == "-" else ("I" if b == "-" else "M") for a, b in zip(cons_x[::-1], cons_y[::-1])]
    out, k = [], 0
    while k < len(ops):
        l = k
        while l < len(ops) and ops[l] == ops[k]:
            l += 1
        out.append("%d%s" % (l - k, ops[k]))
        k = l
    return "".join(out)


def rescore(cons_x, cons_y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """Value of the aligned pair: substitution scores of the letter pairs minus gap_open for the first and gap_extend for every
    further letter of each run of gaps in one string."""
    assert len(cons_x) == len(cons_y)
    tab = _table(match, mismatch, lut)
    total, last = 0.0, "M"
    for a, b in zip(cons_x, cons_y):
        assert not (a == "-" and b == "-")
        op = "D" if a == "-" else ("I" if b == "-" else "M")
        if op == "M":
            total += float(tab[ord(a), ord(b)])
        else:
            total -= float(gap_extend) if op == last else float(gap_open)
        last = op
    return total


def cells_of(cons_x, cons_y, end_x, end_y):
    """The cell of every emitted letter pair or gap letter of the reversed strings, from the end cell backwards."""
    i, j, out = end_x, end_y, []
    for a, b in zip(cons_x, cons_y):
        out.append((i, j))
        if a != "-":
            i -= 1
        if b != "-":
            j -= 1
    return out


def locate(x, y, lo, hi, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(score, row, column) of x against y inside the band."""
    H, E, F, S, band = matrices(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)
    return end_cell(H, band)


def trace(x, y, lo, hi, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """dict(score, end_x, end_y, begin_x, begin_y, pos, cons_x, cons_y, cigar, cells) of x against y inside the band [lo, hi]: what the
    device must return (cells: the checker's own record of the walk, not a field of the device's result)."""
    H, E, F, S, band = matrices(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)
    score, i, j = end_cell(H, band)
    cx, cy, pos, cells = walk(x, y, H, E, F, S, i, j, gap_open) if score > 0 else ("", "", 0, [])
    bx = i + 1 - (len(cx) - cx.count("-")) if score > 0 else 0
    return dict(score=score, end_x=i, end_y=j, begin_x=bx, begin_y=pos, pos=pos, cons_x=cx, cons_y=cy, cigar=cigar(cx, cy), cells=cells)
