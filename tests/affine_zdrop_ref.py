"""The checker of the banded extension under the z-drop stop rule (mi355_sw_affine_extend_run_zdrop / _trace_zdrop): a restatement of
the rule of include/mi355_sw.h on top of tests/affine_extend_band_ref.py (`br`), whose matrices hold -inf outside the band and only
the real columns 0..n.

    r_i = max over the in-band columns 0 <= j <= n of H(i, j), c_i its smallest column (-inf: row i has no such column)
    running best (B, bi, bj), (0, 0, 0) at the anchor; rows i = 1 .. m - 1 in order:
        r_i > B:    (B, bi, bj) = (r_i, i, c_i)
        otherwise:  d = |(i - bi) - (c_i - bj)|;  stop after row i when B - r_i - d e > zdrop   (r_i = -inf: for every finite zdrop)
    rows_done = the stop row, or m

twice — `stop_row_loops` row by row, `stop_row` with whole-array operations (the running best of row i is the first maximum of
r_0 .. r_{i-1}, r_0 = H(0,0) = 0 at column 0) — then `locate` and `trace`, the dicts the device must return: by the DEFINITION BY
TRUNCATION they are br.locate / br.trace on the first rows_done letters of x (of the reversed x for a backward pair), same window,
same band, with to_end_score = -inf and to_end_y = -1 where the pair stopped, and rows_done.  Scores are integers, so every
comparison is exact.  No project code; tests/test_affine_zdrop_ref.py pins it."""
import numpy as np

from tests import affine_extend_band_ref as br
from tests.affine_trace_ref import _b

NINF = float("-inf")


def row_maxima_loops(H):
    """(r, c), each [m + 1]: the maximum of every row of H and its smallest column; cell by cell."""
    m1, n1 = H.shape
    r, c = [NINF] * m1, [0] * m1
    for i in range(m1):
        for j in range(n1):
            if H[i, j] > r[i]:
                r[i], c[i] = float(H[i, j]), j
    return np.array(r), np.array(c, dtype=np.int64)


def row_maxima(H):
    return H.max(axis=1), H.argmax(axis=1).astype(np.int64)         # (argmax: the first maximum)


def stop_row_loops(H, gap_extend, zdrop):
    """rows_done of the matrix H [m + 1, n + 1] (out-of-band cells -inf), row by row as the header states the rule."""
    m = H.shape[0] - 1
    r, c = row_maxima_loops(H)
    B, bi, bj = 0.0, 0, 0
    for i in range(1, m):
        if r[i] > B:
            B, bi, bj = float(r[i]), i, int(c[i])
            continue
        if r[i] == NINF:
            if zdrop < float("inf"):
                return i
            continue
        d = abs((i - bi) - (int(c[i]) - bj))
        if B - r[i] - d * float(gap_extend) > zdrop:
            return i
    return m


def stop_row(H, gap_extend, zdrop):
    """stop_row_loops without a loop over the rows."""
    m = H.shape[0] - 1
    if m < 2:
        return m
    r, c = row_maxima(H)
    assert r[0] == 0.0 and c[0] == 0                                # the anchor is row 0's maximum: every other border cell is negative
    rows = np.arange(m + 1)
    cm = np.maximum.accumulate(r)                                   # cm[i] = max(r_0 .. r_i) >= 0
    new = np.concatenate(([True], r[1:] > cm[:-1]))                 # row i raised the running maximum (strictly)
    first = np.maximum.accumulate(np.where(new, rows, 0))           # the earliest row that holds cm[i]
    i = rows[1:m]
    B, bi = cm[i - 1], first[i - 1]
    bj = c[bi]
    d = np.abs((i - bi) - (c[i] - bj))
    with np.errstate(invalid="ignore"):
        stop = ~(r[i] > B) & (B - r[i] - d * float(gap_extend) > zdrop)
    hit = np.nonzero(stop)[0]
    return int(i[hit[0]]) if len(hit) else m


def _cut(x, s, backward):
    """The first s letters of x in the direction of the extension: of the reversed string for a backward pair."""
    x = _b(x)
    return x[len(x) - s:] if backward else x[:s]


def rows_done(x, y, lo, hi, zdrop, backward=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=br.matrices,
              rule=stop_row):
    x, y = _b(x), _b(y)
    if backward:
        x, y = x[::-1], y[::-1]
    if len(x) == 0:
        return 0
    H = mats(x, y, lo, hi, match, mismatch, gap_open, gap_extend, lut)[0]
    return rule(H, gap_extend, zdrop)


def locate(x, y, lo, hi, zdrop, backward=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mats=br.matrices):
    """dict(score, end_x, end_y, to_end_score, to_end_y, rows_done): what mi355_sw_affine_extend_run_zdrop must return."""
    s = rows_done(x, y, lo, hi, zdrop, backward, match, mismatch, gap_open, gap_extend, lut, mats)
    out = br.locate(_cut(x, s, backward), y, lo, hi, backward, match, mismatch, gap_open, gap_extend, lut, mats)
    if s < len(_b(x)):
        out["to_end_score"], out["to_end_y"] = NINF, -1
    out["rows_done"] = s
    return out


def trace(x, y, lo, hi, zdrop, backward=False, to_end=False, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None,
          mats=br.matrices):
    """br.trace's dict and rows_done: the traced alignment of the truncated pair; traced to_end on a pair that stopped it is the empty
    alignment of score -inf."""
    s = rows_done(x, y, lo, hi, zdrop, backward, match, mismatch, gap_open, gap_extend, lut, mats)
    stopped = s < len(_b(x))
    if stopped and to_end:
        out = dict(score=NINF, end_x=0, end_y=0, pos=0, cons_x="", cons_y="", cigar="")
    else:
        out = br.trace(_cut(x, s, backward), y, lo, hi, backward, to_end, match, mismatch, gap_open, gap_extend, lut, mats)
    if stopped:
        out["to_end_score"], out["to_end_y"] = NINF, -1
    out["rows_done"] = s
    return out
