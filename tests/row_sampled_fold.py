"""Shared by tests/test_row_sampled_fold_ref.py and tests/test_gpu_row_sampled_fold.py: the row stride and the slack of the sampled
running maximum of sw_score_kernel as the headers give them, and a numpy emulation of what a tile publishes."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
SUB = 256                                                            # columns (steps of lane 0) per sub-chunk
SEG = 64                                                             # steps per segment (kSeg): a tile runs whole segments


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, "%s not found in %s" % (name, header)
    return int(m.group(1))


FOLD_ROW_STRIDE = _constant("sw_score_kernel.h", "kFoldRowStride")
MK = _constant("host_score.h", "kScoreMK")


def row_stride(R):
    """fold_row_stride(R, MK) of sw_score_kernel.h for a sampled instance."""
    return min(R, FOLD_ROW_STRIDE)


def folded_rows(R):
    RK = row_stride(R)
    return sorted({r for r in range(R) if r % RK == RK - 1} | {R - 1})


def slack(R, gap):
    """sample_slack of host_score.h, integer scoring."""
    return (row_stride(R) - 1 + MK - 1) * gap


def tile_matrix(x, y, SL, R, ncols, match, mismatch, gap):
    """The cells a tile of SL lanes x R rows computes over `ncols` columns: rows beyond |x| and columns beyond |y| are padding."""
    rows = SL * R
    xs = np.frombuffer(x, dtype=np.uint8)
    ys = np.frombuffer(y, dtype=np.uint8)
    E = np.zeros((rows + 1, ncols + 1), dtype=np.float64)
    jg = gap * np.arange(ncols + 1, dtype=np.float64)
    for i in range(1, rows + 1):
        a = np.zeros(ncols + 1, dtype=np.float64)
        a[1:] = E[i - 1, 1:] - gap                                   # N - g
        if i <= len(xs):
            s = np.where(ys == xs[i - 1], match, mismatch)
            a[1:len(ys) + 1] = np.maximum(a[1:len(ys) + 1], E[i - 1, 0:len(ys)] + s)   # NW + s
        np.maximum(a, 0.0, out=a)
        a[0] = 0.0
        E[i] = np.maximum.accumulate(a + jg) - jg                    # W - g along the row: H(j) = max_k<=j a(k) - (j - k) g
        E[i, 0] = 0.0
    return E


def sampled_sub_values(E, SL, R, n):
    """What the tile publishes per sub-chunk: folded steps t % MK == MK - 1, folded rows, lane l at column t - l."""
    nsub = -(-n // SUB)
    steps = -(-(nsub * SUB + SL) // SEG) * SEG
    val = np.zeros(nsub, dtype=np.float64)
    for lane in range(SL):
        t = np.arange(lane, steps)                                   # column t - lane >= 0 (0-based), matrix column t - lane + 1
        t = t[t % MK == MK - 1]
        sub = np.minimum(t // SUB, nsub - 1)
        for r in folded_rows(R):
            np.maximum.at(val, sub, E[1 + lane * R + r, t - lane + 1])
    return val, steps
