"""Shared by tests/test_prefix_filter_ref.py and tests/test_gpu_prefix_filter.py: the prefix-row filter of a short-read bucket (DESIGN.md
§3.3 L19) as the host applies it, emulated in numpy on the oracle's matrices — the sampled prefix values with the emulation of
tests/row_sampled_fold.py, the two locate rounds on exact windows of the oracle."""
import math

import numpy as np

from oracle import binding as ob
from row_sampled_fold import SEG, SUB, sampled_sub_values, slack, tile_matrix

LANES = 2                                                            # kPrefixLanes of host_score.h
LAG = 63                                                             # columns a candidate window starts in front of its sub-chunk


def geometry(m, R, match, gap):
    """P, W, D of the lemma for a read of m rows on R rows per lane: the end cell lies at most W columns right of its crossing of row
    P, i.e. in the flagged sub-chunk or one of the D to its right."""
    P = LANES * R
    W = (m - P) + int(math.floor(match * (m - P) / gap))
    return P, W, -(-W // SUB)


def bound(m, R, match, gap):
    """A read whose best exact score B0 is not above this cannot be certified: an offender."""
    P = LANES * R
    return match * (m - P) + slack(R, gap)


def prefix_values(x, y, R, match, mismatch, gap):
    """Per-sub-chunk values of the sampled sweep of the first P rows of x over all of y (one tile: the range)."""
    n = len(y)
    nsub = -(-n // SUB)
    steps = -(-(nsub * SUB + LANES) // SEG) * SEG
    E = tile_matrix(x[:LANES * R], y, LANES, R, steps, match, mismatch, gap)
    val, _ = sampled_sub_values(E, LANES, R, n)
    return val


def window_best(x, y, s, match, mismatch, gap):
    """Exact maximum and its first cell (column first, then row; 1-based, as the float engine orders cells) over the window of
    sub-chunk s: own columns s * SUB - LAG .. (s + 1) * SUB - 1 (0-based), behind the full margin of L1."""
    m, n = len(x), len(y)
    lo = max(0, s * SUB - LAG)
    hi = min((s + 1) * SUB, n)
    margin = m + int(math.ceil(match * m / gap)) + 2
    wl = max(0, lo - margin)
    H = ob.fill(x, y[wl:hi], ob.F32, match, mismatch, gap)[:, 1 + lo - wl:]
    best = float(H.max())
    if not best > 0:
        return 0.0, 0, 0
    cols = np.flatnonzero(H.max(axis=0) == best)
    j = int(cols[0])
    i = int(np.flatnonzero(H[:, j] == best)[0])
    return best, i, lo + j + 1


def emulate(x, y, R, match, mismatch, gap, cap):
    """The filter on one read: dict(offender, why, B0, evaluated (sorted sub-chunks), result (score, end_x, end_y))."""
    m, n = len(x), len(y)
    nsub = -(-n // SUB)
    P, W, D = geometry(m, R, match, gap)
    val = prefix_values(x, y, R, match, mismatch, gap)
    out = dict(offender=True, why="", B0=0.0, evaluated=[], result=None, values=val)
    if not val.max() > 0:
        out["why"] = "no prefix value"
        return out
    s0 = int(np.flatnonzero(val == val.max())[0])
    round1 = [s for s in range(s0, s0 + D + 1) if s < nsub]
    best = {s: window_best(x, y, s, match, mismatch, gap) for s in round1}
    B0 = max(b[0] for b in best.values())
    out["B0"] = B0
    out["evaluated"] = round1
    if not B0 > bound(m, R, match, gap):
        out["why"] = "B0 cannot certify"
        return out
    thr = B0 - match * (m - P) - slack(R, gap)
    flagged = [int(f) for f in np.flatnonzero(val >= thr)]
    if len(flagged) > cap:                                           # (the filter's count exceeds the cap)
        out["why"] = "over the cap"
        return out
    for f in flagged:
        for s in range(f, f + D + 1):
            if s < nsub and s not in best:
                best[s] = window_best(x, y, s, match, mismatch, gap)
    top = max(b[0] for b in best.values())
    first = min((b[2], b[1]) for b in best.values() if b[0] == top)
    out.update(offender=False, evaluated=sorted(best), result=(top, first[1], first[0]))
    return out


def covers(evaluated, j):
    """Does the window of an evaluated sub-chunk hold 0-based column j?"""
    s = j // SUB
    return s in evaluated or (s + 1 in evaluated and j >= (s + 1) * SUB - LAG)
