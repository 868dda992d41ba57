"""Shared by tests/test_prefix_stage_ref.py and tests/test_gpu_prefix_stage.py: one range [lo, hi) of a reference of N columns per case,
and five reads planted at its two ends.  The prefix tiles (SL = 2 lanes x R = 19 rows, 256-column tiles) stage 32 reference codes per
lane and segment with dword and 16-byte loads (sw_score_kernel.h stage_load); a lane's span starts at a column = lo (mod 32), so what
decides the load's byte shift is lo & 3, and what decides where the cut at hi falls in a dword and in a 16-byte vector is hi - lo."""
import numpy as np

from prefix_filter import LANES
from row_sampled_fold import SUB

R = 19
P = LANES * R                                                        # 38 rows
M = 150                                                              # read length: the first P letters are planted, the rest is 'N'
N = 41_003                                                           # columns of the reference: more than 128 tiles in every range
PARTLY = 128 * SUB + 300                                             # hi - lo that leaves the second workgroup's last tile 44 columns
INSIDE = 10                                                          # columns of the straddling copy in front of hi
SCORING = (3.0, -3.0, 2.0)

# lo: every lo & 3, lo & 15 != 0, below and above one lane span (32 columns).  hi: the end of the buffer (the loads of the last span
# reach into the allocation's slack), cuts in mid dword and in mid 16-byte vector, and a last tile that lies only partly in the range
PAIRS = [(0, N), (1, N - 1), (2, N - 5), (3, N - 17), (5, N), (13, N - 1), (31, N - 5), (33, N - 17), (0, PARTLY), (13, 13 + PARTLY)]

NAMES = ["ends_at_hi", "starts_at_lo", "straddles_hi", "in_front_of_lo", "no_hit"]


def batch(lo, hi):
    """(reads, reference) of the range [lo, hi): NAMES says what each read is."""
    rng = np.random.default_rng(7000 + 64 * lo + (N - hi))
    y = bytearray(rng.choice(list(b"ACGT"), N).astype(np.uint8))

    def letters(k):
        return bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))

    def read(prefix):
        return prefix + b"N" * (M - len(prefix))

    at_hi = letters(P)                                               # its P letters end in column hi - 1
    y[hi - P:hi] = at_hi
    at_lo = letters(P)                                               # ... in column lo + P - 1: the alignment starts in the range's first column
    y[lo:lo + P] = at_lo
    # the copy lies across hi: INSIDE columns in front of it (the last letters of at_hi, which stay as they are) and the better part,
    # up to P - INSIDE columns, behind it — as many as the buffer has
    across = at_hi[P - INSIDE:] + letters(P - INSIDE)
    beyond = min(P - INSIDE, N - hi)
    y[hi:hi + beyond] = across[INSIDE:INSIDE + beyond]
    # the copy ends in column lo - 1: as many of its last letters as there are columns in front of lo
    front = letters(P)
    y[0:lo] = front[P - min(lo, P):]
    reads = [read(at_hi), read(at_lo), read(across), read(front), letters(M)]
    return reads, bytes(y)
