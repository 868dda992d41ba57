"""The checker of the affine-gap tests: a numpy restatement of the recurrence in include/mi355_sw.h

    E(i,j) = max(E(i,j-1) - gap_extend, H(i,j-1) - gap_open)
    F(i,j) = max(F(i-1,j) - gap_extend, H(i-1,j) - gap_open)
    H(i,j) = max(0, H(i-1,j-1) + s, E(i,j), F(i,j))           H = 0 on the borders; E, F = -inf there

swept by anti-diagonals, with the first maximum in column-major order (smallest column of y, then smallest row of x; 1-based;
0 / 0 for an all-zero matrix), and a plain three-loop version for tiny inputs.  tests/test_affine_ref.py pins both: to each other,
to known answers, and — where gap_open == gap_extend makes the model the reference's linear one — to the reference's oracle.
No GPU and no project code is needed here."""
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


def locate_batch(xs, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(score[nq], row[nq], column[nq]) of every x of `xs` against y: one sweep over the anti-diagonals for all of them."""
    xs = [_b(x) for x in xs]
    y = _b(y)
    nq, n = len(xs), len(y)
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    best = np.zeros(nq)
    bi = np.zeros(nq, dtype=np.int64)
    bj = np.zeros(nq, dtype=np.int64)
    M = int(lens.max()) if nq else 0
    if M == 0 or n == 0:
        return best, bi, bj
    tab = _table(match, mismatch, lut)
    X = np.zeros((nq, M), dtype=np.intp)
    for k, x in enumerate(xs):
        X[k, :len(x)] = x
    yi = y.astype(np.intp)
    go, ge = float(gap_open), float(gap_extend)
    # diagonals indexed by the row: cell (i, j) of diagonal d = i + j sits at index i
    Hpp = np.zeros((nq, M + 1))
    Hp = np.zeros((nq, M + 1))
    Ep = np.full((nq, M + 1), NEG)
    Fp = np.full((nq, M + 1), NEG)
    rows = np.arange(nq)
    for d in range(2, M + n + 1):
        lo, hi = max(1, d - n), min(M, d - 1)
        ii = np.arange(lo, hi + 1)
        jj = d - ii
        s = tab[X[:, ii - 1], yi[jj - 1][None, :]]
        e = np.maximum(Ep[:, lo:hi + 1] - ge, Hp[:, lo:hi + 1] - go)
        f = np.maximum(Fp[:, lo - 1:hi] - ge, Hp[:, lo - 1:hi] - go)
        h = np.maximum(np.maximum(Hpp[:, lo - 1:hi] + s, 0.0), np.maximum(e, f))
        Hc = np.zeros((nq, M + 1))
        Ec = np.full((nq, M + 1), NEG)
        Fc = np.full((nq, M + 1), NEG)
        Hc[:, lo:hi + 1] = h
        Ec[:, lo:hi + 1] = e
        Fc[:, lo:hi + 1] = f
        # first maximum: on one diagonal the smallest column is the largest row
        hm = np.where(ii[None, :] <= lens[:, None], h, -1.0)
        dmax = hm.max(axis=1)
        cand = (dmax > 0.0) & (dmax >= best)
        if cand.any():
            ci = ii[hm.shape[1] - 1 - np.argmax(hm[:, ::-1] == dmax[:, None], axis=1)]
            cj = d - ci
            take = cand & ((dmax > best) | (cj < bj) | ((cj == bj) & (ci < bi)))
            best = np.where(take, dmax, best)
            bi = np.where(take, ci, bi)
            bj = np.where(take, cj, bj)
        Hpp, Hp, Ep, Fp = Hp, Hc, Ec, Fc
    return best, bi, bj


def locate(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """(score, row, column) of x against y."""
    s, i, j = locate_batch([x], y, match, mismatch, gap_open, gap_extend, lut)
    return float(s[0]), int(i[0]), int(j[0])


def locate_loops(x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    """The same by three plain loops (columns, rows, and the scan for the first maximum): tiny inputs only."""
    x, y = _b(x), _b(y)
    m, n = len(x), len(y)
    tab = _table(match, mismatch, lut)
    H = [[0.0] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    for j in range(1, n + 1):
        for i in range(1, m + 1):
            E[i][j] = max(E[i][j - 1] - gap_extend, H[i][j - 1] - gap_open)
            F[i][j] = max(F[i - 1][j] - gap_extend, H[i - 1][j] - gap_open)
            H[i][j] = max(0.0, H[i - 1][j - 1] + float(tab[x[i - 1], y[j - 1]]), E[i][j], F[i][j])
    best, bi, bj = 0.0, 0, 0
    for j in range(1, n + 1):
        for i in range(1, m + 1):
            if H[i][j] > best:
                best, bi, bj = H[i][j], i, j
    return float(best), bi, bj
