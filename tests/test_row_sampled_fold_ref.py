"""The sampled running maximum of sw_score_kernel, emulated in numpy against the oracle's full matrix (no GPU).

A one-strip MK = 4 instance folds the running maximum every 4th step, and then only the rows r of a lane with r % RK == RK - 1 and the
lane's last row.  The emulation keeps the kernel's geometry: lane l of a tile owns rows l * R .. l * R + R - 1, at step t it is at column
t - l, rows beyond the query and columns beyond the reference are padding (their diagonal term is the zero floor, the two gap terms
pass through), and a tile reports one value per sub-chunk of 256 steps.  Checked: every sub-chunk value is a lower bound, and every
cell that holds the maximum lies in a sub-chunk — its own or the next one — whose value is within (RK - 1 + MK - 1) gaps of it.
RK and MK are read from the headers the library is built from."""
import numpy as np
import pytest

from oracle import binding as ob
from row_sampled_fold import FOLD_ROW_STRIDE, MK, SEG, SUB, folded_rows, row_stride, sampled_sub_values, slack, tile_matrix


def make_pair(rng, SL, R, m, n, end_row, end_col, alpha=b"ACGT"):
    """A random reference of n and a query of m bases with a planted hit: the query's first end_row bases are random and end at 0-based
    column end_col of the reference, the rest is a letter the reference does not hold (so that the hit's alignment ends in row end_row)."""
    x = bytes(rng.choice(list(alpha), end_row).astype(np.uint8)) + b"N" * (m - end_row)
    y = bytearray(rng.choice(list(alpha), n).astype(np.uint8))
    y[end_col - end_row + 1:end_col + 1] = x[:end_row]
    return x, bytes(y)


SCORINGS = [(3.0, -3.0, 2.0), (5.0, -4.0, 3.0), (2.0, -1.0, 1.0)]
SHAPES = [(8, 19, 150), (16, 10, 150), (8, 19, 152), (16, 10, 160)]   # (lanes, rows per lane, query length): with and without padding rows


def test_header_constants():
    assert MK == 4
    assert FOLD_ROW_STRIDE >= 1
    for R in (10, 13, 19, 32):
        rows = folded_rows(R)
        assert rows[-1] == R - 1
        gaps = np.diff([-1] + rows)                                  # rows between one folded row and the next, the first included
        assert gaps.max() == row_stride(R), (R, rows)                # a cell is at most RK - 1 rows above the next folded row
        assert slack(R, 2.0) == (row_stride(R) + 2) * 2.0


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "%g_%g_%g" % s)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_len%d" % s)
def test_sampled_fold_bounds(shape, scoring):
    SL, R, m = shape
    match, mismatch, gap = scoring
    n = 3 * SUB + 77                                                 # four sub-chunks, the last one short
    rng = np.random.default_rng(1000 * SL + R + int(10 * match))
    lanes = sorted({0, SL // 2, (m - 1) // R})                       # first, a middle and the last lane that holds query rows
    cases = []
    for lane in lanes:
        for r in range(R):
            i = lane * R + r + 1                                     # the hit ends in row r of the lane (1-based matrix row i)
            if i > m:
                continue
            for end_col in (SUB + 40 + r, 2 * SUB - 1, n - 1):       # mid sub-chunk (every step residue over r), last column of a
                if end_col - i + 1 >= 0:                             # sub-chunk, last column of the reference
                    cases.append((i, end_col))
    worst = 0.0
    for i, end_col in cases:
        x, y = make_pair(rng, SL, R, m, n, i, end_col)
        H = ob.fill(x, y, ob.F32, match, mismatch, gap)
        nsub = -(-n // SUB)
        steps = -(-(nsub * SUB + SL) // SEG) * SEG
        E = tile_matrix(x, y, SL, R, steps, match, mismatch, gap)
        assert np.array_equal(E[:m + 1, :n + 1], H.astype(np.float64)), "the emulated cells differ from the oracle's matrix"
        val, _ = sampled_sub_values(E, SL, R, n)
        colmax = H.max(axis=0)[1:]                                   # true maximum per 0-based column
        M = float(H.max())
        # lower bounds: what a sub-chunk reports comes from cells of columns up to its end (padding only decays them)
        for s in range(nsub):
            assert val[s] <= colmax[:min((s + 1) * SUB, n)].max(), (shape, scoring, i, end_col, s)
        key = float(val.max())
        assert key <= M
        for j in np.flatnonzero(colmax == M):
            s = int(j) // SUB
            seen = max(val[s], val[s + 1] if s + 1 < nsub else 0.0)
            assert seen >= M - slack(R, gap), (shape, scoring, i, end_col, int(j), M, seen)
            assert seen >= key - slack(R, gap)
            worst = max(worst, M - seen)
    # the cases reach beyond the slack of a fold that takes every row: a filter left at (MK - 1) gaps would lose a maximum here
    if row_stride(R) > 1:
        assert worst > (MK - 1) * gap, (shape, scoring, worst)
