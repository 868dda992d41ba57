"""The checker of the affine-gap traceback tests: the full Gotoh matrices by the recurrence of include/mi355_sw.h

    E(i,j) = max(E(i,j-1) - gap_extend, H(i,j-1) - gap_open)
    F(i,j) = max(F(i-1,j) - gap_extend, H(i-1,j) - gap_open)
    H(i,j) = max(0, H(i-1,j-1) + s, E(i,j), F(i,j))           H = 0 on the borders; E, F = -inf there

(numpy, one vector operation per anti-diagonal, all three matrices kept), the first maximum in column-major order, and the walk of
the header's traceback rule in plain Python over those full matrices: state M stops at H == 0, prefers the diagonal, then E, then F;
states E and F emit one gap letter and return to M when the gap was opened here (the opening wins a tie with the extension).  Scores
are integers, so every comparison is exact.  Plus `cigar` and `rescore`, the value of an aligned pair of strings.

No project code and no window: nothing here rests on lemma L17.  tests/test_affine_trace_ref.py pins it."""
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


def matrices(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(H, E, F, S), each [m + 1, n + 1]; S[i, j] = f(x[i], y[j]) (row and column 0 unused)."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    go, ge = float(gap_open), float(gap_extend)
    H = np.zeros((m + 1, n + 1))
    E = np.full((m + 1, n + 1), NEG)
    F = np.full((m + 1, n + 1), NEG)
    S = np.zeros((m + 1, n + 1))
    if m and n:
        S[1:, 1:] = _table(match, mismatch, lut)[x.astype(np.intp)[:, None], y.astype(np.intp)[None, :]]
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        e = np.maximum(E[i, j - 1] - ge, H[i, j - 1] - go)
        f = np.maximum(F[i - 1, j] - ge, H[i - 1, j] - go)
        E[i, j] = e
        F[i, j] = f
        H[i, j] = np.maximum(np.maximum(H[i - 1, j - 1] + S[i, j], 0.0), np.maximum(e, f))
    return H, E, F, S


def end_cell(H):
    """(score, row, column) of the first maximum in column-major order, 1-based; (0, 0, 0) for an all-zero matrix."""
    best = float(H.max()) if H.size else 0.0
    if not best > 0:
        return 0.0, 0, 0
    cols = np.nonzero((H == best).any(axis=0))[0]
    j = int(cols[0])
    i = int(np.nonzero(H[:, j] == best)[0][0])
    return best, i, j


def walk(x, y, H, E, F, S, i, j, gap_open):
    """The traceback rule from state M at (i, j): (reversed cons_x, reversed cons_y, pos)."""
    x, y = _b(x), _b(y)
    go = float(gap_open)
    cx, cy = [], []
    pos, state = 0, "M"
    while True:
        if state == "M":
            if i <= 0 or j <= 0 or H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + S[i, j]:
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
    """Value of the aligned pair (either direction: the value of an alignment does not depend on it): substitution scores of
    the letter pairs minus gap_open for the first and gap_extend for every further letter of each run of gaps in one string."""
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


def trace(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """dict(score, end_x, end_y, begin_x, begin_y, pos, cons_x, cons_y, cigar) of x against y: what the device must return."""
    H, E, F, S = matrices(x, y, match, mismatch, gap_open, gap_extend, lut)
    score, i, j = end_cell(H)
    cx, cy, pos = walk(x, y, H, E, F, S, i, j, gap_open) if score > 0 else ("", "", 0)
    bx = i + 1 - (len(cx) - cx.count("-")) if score > 0 else 0
    return dict(score=score, end_x=i, end_y=j, begin_x=bx, begin_y=pos, pos=pos, cons_x=cx, cons_y=cy, cigar=cigar(cx, cy))


def trace_batch(xs, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    return [trace(x, y, match, mismatch, gap_open, gap_extend, lut) for x in xs]
