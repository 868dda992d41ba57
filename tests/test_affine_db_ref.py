"""Lemma L18, the row window of the affine-gap traceback, stated as tests/test_affine_trace_ref.py states L17: the
walk of tests/affine_trace_ref.py over the rows (end_x - Wr, end_x] alone behind a zero border, Wr = end_y + ceil((smax * end_y -
score) / gap_extend) + 2, equals the walk over the full matrices — clamped at row 1 and unclamped, alone and together with the
L17 window of columns, which is what the device fills: the smaller of the two windows in each dimension.  Plus the byte classes of
the database-search kernel's profile, restated in a few lines: bytes with equal score rows against the reference's letters share
a class; and the lane scheme of sw_affine_prof_kernel (columns of y on 16 lanes, rows of x skewed by the lane, F and H - o per
column, E handed from lane to lane, the orderable key) emulated step by step in float32 against tests/affine_ref.py.  No GPU and no
project code."""
import numpy as np

from tests import affine_trace_ref as tr

SCORINGS = [(3, -3, 5, 1), (2, -1, 3, 1), (1, -1, 2, 2), (5, -4, 10, 3)]


def _random_problems(count, seed, mmax=90, nmax=10):
    """Long x against short y (the database-search shape), some with a planted copy of y carrying a 3-row insert, some with
    an exact copy."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        alpha = np.frombuffer(b"ACGT" if k % 2 == 0 else b"AC", dtype=np.uint8)
        m, n = int(rng.integers(1, mmax + 1)), int(rng.integers(1, nmax + 1))
        y = alpha[rng.integers(0, len(alpha), n)].tobytes()
        x = bytearray(alpha[rng.integers(0, len(alpha), m)].tobytes())
        if k % 3 == 0 and n >= 8 and m >= n + 3:
            at = int(rng.integers(0, m - n - 2))
            x[at:at + n + 3] = y[:n // 2] + alpha[rng.integers(0, len(alpha), 3)].tobytes() + y[n // 2:]
        elif k % 3 == 1 and m >= n:
            at = int(rng.integers(0, m - n + 1))
            x[at:at + n] = y
        out.append((bytes(x).decode(), y.decode(), SCORINGS[k % len(SCORINGS)]))
    return out


def _window_trace(x, y, match, mismatch, gap_open, gap_extend, rows=True, cols=False):
    """The walk over the window behind the end cell alone: ((cons_x, cons_y, pos), row window clamped, column window clamped)."""
    H = tr.matrices(x, y, match, mismatch, gap_open, gap_extend)[0]
    score, i, j = tr.end_cell(H)
    smax = max(match, mismatch, 0)
    Wr = j + int(np.ceil((smax * j - score) / float(gap_extend))) + 2
    Wc = i + int(np.ceil((smax * i - score) / float(gap_extend))) + 2
    rclamped = not rows or Wr >= i
    cclamped = not cols or Wc >= j
    mw = i if rclamped else Wr
    nw = j if cclamped else Wc
    xw, yw = x[i - mw:i], y[j - nw:j]
    Hw, Ew, Fw, Sw = tr.matrices(xw, yw, match, mismatch, gap_open, gap_extend)
    assert Hw[mw, nw] == score
    cx, cy, pos = tr.walk(xw, yw, Hw, Ew, Fw, Sw, mw, nw, gap_open)
    return (cx, cy, pos + (j - nw)), rclamped, cclamped


def test_L18_row_window_walk_equals_full_walk():
    counts = {True: 0, False: 0}
    for x, y, sc in _random_problems(300, 29):
        r = tr.trace(x, y, *sc)
        if r["score"] == 0:
            continue
        got, rclamped, _ = _window_trace(x, y, *sc)
        counts[rclamped] += 1
        assert got == (r["cons_x"], r["cons_y"], r["pos"]), (x, y, sc, rclamped, got, r)
    assert counts[True] >= 30 and counts[False] >= 30, counts


def test_L17_and_L18_windows_together():
    """Both windows at once, on shapes where either one, both or neither is shorter than the matrix."""
    seen = set()
    problems = _random_problems(150, 31) + _random_problems(150, 37, mmax=40, nmax=40) + \
        [(y, x, sc) for x, y, sc in _random_problems(100, 41)]
    for x, y, sc in problems:
        r = tr.trace(x, y, *sc)
        if r["score"] == 0:
            continue
        got, rclamped, cclamped = _window_trace(x, y, *sc, rows=True, cols=True)
        seen.add((rclamped, cclamped))
        assert got == (r["cons_x"], r["cons_y"], r["pos"]), (x, y, sc, rclamped, cclamped, got, r)
    assert (False, True) in seen and (True, False) in seen and (True, True) in seen, seen


def byte_classes(lut, letters):
    """cls[256] and the number of classes: bytes of x with the same scores against `letters` (the reference's) share one, numbered
    in the order of their first byte."""
    rows = np.asarray(lut, dtype=np.float64).reshape(256, 256)[:, sorted(letters)]
    cls, reps = np.zeros(256, dtype=np.int64), []
    for a in range(256):
        for c, b in enumerate(reps):
            if np.array_equal(rows[a], rows[b]):
                cls[a] = c
                break
        else:
            cls[a] = len(reps)
            reps.append(a)
    return cls, len(reps)


def test_byte_classes():
    ident = np.full((256, 256), -3.0)
    ident[np.arange(256), np.arange(256)] = 3.0
    cls, n = byte_classes(ident, b"ACGT")
    assert n == 5 and len({int(cls[b]) for b in b"ACGT"}) == 4 and cls[ord("N")] == cls[0] == cls[255]
    rng = np.random.default_rng(3)
    aa = b"ACDEFGHIKLMNPQRSTVWY"
    lut = np.full((256, 256), -4.0)
    lut[np.ix_(list(aa), list(aa))] = rng.integers(-4, 12, (20, 20))
    cls, n = byte_classes(lut, aa)
    assert n == 21 and len({int(cls[b]) for b in aa}) == 20 and cls[ord("B")] == cls[ord("-")]
    lut[ord("B")] = lut[ord("D")]                                   # a twenty-first letter that scores as D does
    cls, n = byte_classes(lut, aa)
    assert n == 21 and cls[ord("B")] == cls[ord("D")]
    # columns of letters the reference does not contain do not split a class
    lut[ord("A"), ord("Z")] = 7.0
    assert byte_classes(lut, aa)[1] == 21


# ---- the lane scheme of sw_affine_prof_kernel, emulated step by step --------------------------------------------------------------
def _slot(x, y, R, match, mismatch, gap_open, gap_extend, lut=None):
    """One 16-lane slot as the kernel runs it (csrc/sw_affine_prof_kernel.h), in float32 scaled by 2^-k: lane l holds columns
    l R .. l R + R - 1 of y and works on row k - l at step k; per column F and Ho = H - o, the profile holds s + o; Ho of the lane's
    last column and Erun go to the next lane between steps, lane 0 takes -o for both; key = bits(H) | (31 - column in the lane),
    strict '>' per step keeps the first row; then (value, smaller column, smaller row) across the lanes."""
    f32 = np.float32
    xb, yb = tr._b(x), tr._b(y)
    m, n = len(xb), len(yb)
    tab = tr._table(match, mismatch, lut)
    smax = max(0.0, float(tab[:, yb].max()))
    k = max(1, int(np.floor(np.log2(smax * (n + 1) + 1))) + 2)
    sc = f32(2.0 ** -k)
    o, e = f32(gap_open) * sc, f32(gap_extend) * sc
    PAD = f32(-1.0e30)
    F = np.full((16, R), -o, dtype=f32)
    Ho = np.full((16, R), -o, dtype=f32)
    up_prev = np.full(16, -o, dtype=f32)
    eout = np.full(16, -o, dtype=f32)
    blk = np.zeros(16, dtype=f32)
    tl = np.zeros(16, dtype=np.int64)
    for step in range(m + 16):
        up = np.concatenate([[-o], Ho[:-1, R - 1]]).astype(f32)     # DPP row_shr:1, `old` = -o in the first lane
        erun = np.concatenate([[-o], eout[:-1]]).astype(f32)
        for l in range(16):
            t = step - l
            diag, er, best = up_prev[l], erun[l], f32(0)
            for r in range(R):
                j = l * R + r
                s = (f32(tab[xb[t], yb[j]]) * sc + o) if 0 <= t < m and j < n else PAD
                w = Ho[l, r]
                xv = min(max(diag + s, f32(0)), f32(1))
                f = max(F[l, r] - e, w)
                h = max(xv, f, er)
                key = np.array([h], dtype=f32).view(np.uint32)[0] | np.uint32(31 - r)
                best = max(best, np.array([key], dtype=np.uint32).view(f32)[0])
                Ho[l, r] = h - o
                er = max(er - e, Ho[l, r])
                F[l, r] = f
                diag = w
            eout[l] = er
            if best > blk[l]:
                tl[l], blk[l] = t, best
        up_prev = up
    cand = []
    for l in range(16):
        kb = int(np.array([blk[l]], dtype=f32).view(np.uint32)[0])
        v = float(np.array([kb & ~31], dtype=np.uint32).view(f32)[0]) * 2.0 ** k
        if v > 0:
            cand.append((-v, l * R + (31 - (kb & 31)) + 1, int(tl[l]) + 1))
    if not cand:
        return 0.0, 0, 0
    v, j, i = min(cand)
    return -v, i, j


def test_lane_scheme_of_the_database_kernel():
    from tests import affine_ref
    rng = np.random.default_rng(43)
    cases = 0
    for k in range(60):
        alpha = np.frombuffer(b"ACGT" if k % 2 == 0 else b"AC", dtype=np.uint8)
        R = (2, 3, 4)[k % 3]
        n = int(rng.integers(1, 16 * R + 1))                        # with and without padding columns
        m = int(rng.integers(1, 70))
        y = alpha[rng.integers(0, len(alpha), n)].tobytes()
        x = bytearray(alpha[rng.integers(0, len(alpha), m)].tobytes())
        if k % 4 == 0 and m >= n // 2 + 3 and n >= 8:               # half of y, three rows of x against a gap, the other half
            x[:n // 2 + 3] = (y[:n // 4] + bytes(alpha[rng.integers(0, len(alpha), 3)]) + y[n // 4:n // 2])
        sc = SCORINGS[k % len(SCORINGS)]
        assert _slot(bytes(x), y, R, *sc) == affine_ref.locate(bytes(x), y, *sc), (x, y, R, sc)
        cases += 1
    # ties: the same maximum in two rows of one column, and in a later column at an earlier row
    y = "ACGTTGCAAGGCTTAACCGGATCGATTACG"
    for x in (y[5:15] + "NNNNNNNNNNNN" + y[5:15], y[18:28] + "NNNNNNNNNNNN" + y[5:15]):
        for R in (2, 5):
            assert _slot(x, y, R, *SCORINGS[0]) == affine_ref.locate(x, y, *SCORINGS[0]), (x, R)
    assert cases == 60
