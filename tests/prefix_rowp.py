"""Shared by tests/test_prefix_rowp_ref.py, tests/test_gpu_prefix_rowp_tiles.py and tests/test_gpu_prefix_probe_height.py: the row-P
variant of the prefix filter emulated in numpy on the oracle's cell rule.  A row-P tile folds row P = LANES * R
alone — lane LANES - 1, its row R - 1, at the steps t % MK == MK - 1 — so its slack is (MK - 1) gaps; the two locate rounds are those of
tests/prefix_filter.py with that slack and the extra condition B0 > smax P; and a probed bucket picks its height as align_range_core
does (host_pipeline.h)."""
import math

import numpy as np

import prefix_filter
from prefix_filter import LANES, window_best
from row_sampled_fold import MK, SEG, SUB, tile_matrix

LISTED = (13, 16, 19, 26, 32)                                        # kR8M of host_score.h
PROBE = 64                                                           # kPrefixProbe: a bucket of >= 8 * PROBE reads is probed


def slack(gap):
    """rowp_slack of host_score.h."""
    return (MK - 1) * gap


def geometry(m, R, match, gap):
    P = LANES * R
    W = (m - P) + int(math.floor(match * (m - P) / gap))
    return P, W, -(-W // SUB)


def bound(m, R, match, gap):
    """prefix_bound of host_score.h for a row-P pass: a read whose B0 is not above it offends."""
    P = LANES * R
    return max(match * (m - P) + slack(gap), match * P)


def rowp_fold(E, R, steps, first_sub, nsub):
    """Values per sub-chunk of row P of the tile matrix E over `steps` steps: step t belongs to sub-chunk first_sub(t) (clipped to nsub)."""
    lane = LANES - 1
    val = np.zeros(nsub, dtype=np.float64)
    t = np.arange(lane, steps)
    t = t[t % MK == MK - 1]
    j = t - lane + 1                                                 # matrix column of lane LANES - 1 at step t
    np.maximum.at(val, np.clip(first_sub(t), 0, nsub - 1), E[LANES * R, j])
    return val


def rowp_values(x, y, R, match, mismatch, gap):
    """The range as ONE tile (what the lemma speaks of): value of every sub-chunk."""
    n = len(y)
    nsub = -(-n // SUB)
    steps = -(-(nsub * SUB + LANES) // SEG) * SEG
    E = tile_matrix(x[:LANES * R], y, LANES, R, steps, match, mismatch, gap)
    return rowp_fold(E, R, steps, lambda t: t // SUB, nsub)


def rowp_tile_values(x, y, R, chunk, warm, match, mismatch, gap):
    """What the device leaves per sub-chunk when the range is cut into tiles of `chunk` own columns behind `warm` warm-up columns
    (multiples of 64; warm = 0 for a lone tile): a tile starts from a zero border `warm` columns in front of its own, sees padding
    behind its own last column and in front of the range, and the steps of its warm-up count for its first sub-chunk.  One value per
    sub-chunk of every tile, the last tile's beyond the range included (decayed copies of real cells)."""
    n = len(y)
    ntiles = -(-n // chunk)
    if ntiles == 1:
        warm = 0
    spt = chunk // SUB
    steps = -(-(warm + chunk + LANES) // SEG) * SEG
    out = []
    for c in range(ntiles):
        lo, hi = c * chunk, min((c + 1) * chunk, n)
        front = max(0, warm - lo)                                    # padding columns in front of the range: cells stay 0
        E = tile_matrix(x[:LANES * R], y[lo - warm + front:hi], LANES, R, steps, match, mismatch, gap)
        if front:
            E = np.concatenate([E[:, :1], np.zeros((E.shape[0], front)), E[:, 1:steps + 1 - front]], axis=1)
        out.append(rowp_fold(E, R, steps, lambda t: (t - warm) // SUB, spt))
    return np.concatenate(out)


def emulate(x, y, R, match, mismatch, gap, cap, rowp=True, vote_R=0):
    """One read through the filter at R rows per lane: dict(offender, why, B0, evaluated, result, values).  rowp=False: the fold over
    all prefix rows (tests/prefix_filter.py emulate).  vote_R (a probe at a lower height): also `vote`, whether a row-P pass at vote_R
    could certify the read as far as this sweep can tell — B0 above that bound, and that threshold within the cap on THESE values."""
    if not rowp:
        return prefix_filter.emulate(x, y, R, match, mismatch, gap, cap)
    m, n = len(x), len(y)
    nsub = -(-n // SUB)
    P, W, D = geometry(m, R, match, gap)
    val = rowp_values(x, y, R, match, mismatch, gap)
    out = dict(offender=True, why="", B0=0.0, evaluated=[], result=None, values=val, vote=False)
    if not val.max() > 0:
        out["why"] = "no prefix value"
        return out
    s0 = int(np.flatnonzero(val == val.max())[0])
    best = {s: window_best(x, y, s, match, mismatch, gap) for s in range(s0, s0 + D + 1) if s < nsub}
    B0 = max(b[0] for b in best.values())
    out.update(B0=B0, evaluated=sorted(best))
    if vote_R and B0 > bound(m, vote_R, match, gap):
        out["vote"] = int(np.count_nonzero(val >= B0 - match * (m - LANES * vote_R) - slack(gap))) <= cap
    if not B0 > bound(m, R, match, gap):
        out["why"] = "B0 cannot certify"
        return out
    thr = B0 - match * (m - P) - slack(gap)
    flagged = [int(f) for f in np.flatnonzero(val >= thr)]
    if len(flagged) > cap:
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


def low_height(R, minlen, maxlen, match, gap):
    """prefix_low_R of host_score.h: the next lower listed R when a row-P pass of it is eligible for the bucket, else 0."""
    lower = [r for r in LISTED if r < R]
    if not lower:
        return 0
    low = max(lower)
    return low if minlen > LANES * low and match * minlen > bound(maxlen, low, match, gap) else 0


def emulate_bucket(reads, y, R, match, mismatch, gap, cap, low=True, run=map):
    """A bucket of equally long reads (in the order the library sweeps them) through the filter as align_range_core runs it: the
    probe of the first PROBE reads picks the height of the rest.  Returns dict(launches=[(R, fold, count)], offenders=set of
    positions, outcome); `run` maps the per-read emulation (a thread pool's map)."""
    n = len(reads)
    m = len(reads[0])
    one = lambda Rr, rowp, vote_R=0: (lambda x: emulate(x, y, Rr, match, mismatch, gap, cap, rowp, vote_R))
    if n < 8 * PROBE:
        e = list(run(one(R, False), reads))
        return dict(launches=[(R, False, n)], offenders={k for k in range(n) if e[k]["offender"]}, outcome="unprobed")
    lowR = low_height(R, m, m, match, gap) if low else 0
    probe = list(run(one(lowR or R, bool(lowR), R if lowR else 0), reads[:PROBE]))
    off = {k for k in range(PROBE) if probe[k]["offender"]}
    launches = [(lowR or R, bool(lowR), PROBE)]
    if not lowR:
        if 2 * len(off) > PROBE:
            return dict(launches=launches, offenders=off, outcome="probe_failed")
        rest = list(run(one(R, False), reads[PROBE:]))
        launches.append((R, False, n - PROBE))
        return dict(launches=launches, offenders=off | {PROBE + k for k, e in enumerate(rest) if e["offender"]}, outcome="own")
    if 2 * len(off) > PROBE:                                         # (prefix_bucket gives up: the whole probe offends)
        off = set(range(PROBE))
    if 16 * len(off) <= PROBE:
        rest = list(run(one(lowR, True), reads[PROBE:]))
        launches.append((lowR, True, n - PROBE))
        return dict(launches=launches, offenders=off | {PROBE + k for k, e in enumerate(rest) if e["offender"]}, outcome="low")
    if 2 * sum(1 for e in probe if not e["vote"]) > PROBE:
        return dict(launches=launches, offenders=off, outcome="probe_failed")
    riders = sorted(k for k in off if probe[k]["vote"])
    order = riders + list(range(PROBE, n))                           # (equal lengths: the stable sort keeps this order)
    rest = list(run(one(R, True), [reads[k] for k in order]))
    launches.append((R, True, len(order)))
    offenders = (off - set(riders)) | {order[k] for k, e in enumerate(rest) if e["offender"]}
    return dict(launches=launches, offenders=offenders, outcome="own_rowp", riders=riders)
