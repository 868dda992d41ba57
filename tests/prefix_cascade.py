"""Shared by tests/test_prefix_cascade_ref.py, tests/test_gpu_prefix_step_tiles.py and tests/test_gpu_prefix_cascade.py: the prefix
filter's heights as a chain (host_pipeline.h prefix_chain) emulated in numpy on the oracle's cell rule.

A row-P tile with fold stride `mk` folds row P = LANES * R alone at the steps t % mk == mk - 1; its slack is (mk - 1) gaps — none for
the tiles that fold at every step (mk = 1).  A bucket of at least CHAIN reads probes its first PROBE reads at the lowest eligible
height, starts the rest at the lowest height the probe's offender count pays for, and gives the offenders of that pass one pass at the
next height."""
import math

import numpy as np

from oracle import binding as ob
from prefix_filter import LANES, window_best
from row_sampled_fold import MK, SEG, SUB, tile_matrix

LISTED = (13, 16, 19, 26, 32)                                        # kR8M of host_score.h
PROBE = 64                                                           # kPrefixProbe
CHAIN = 16 * PROBE                                                   # kPrefixChain: buckets from this size on take the chain


def slack(gap, mk=1):
    """rowp_slack of host_score.h for an instance that folds every mk-th step."""
    return (mk - 1) * gap


def geometry(m, R, match, gap):
    P = LANES * R
    W = (m - P) + int(math.floor(match * (m - P) / gap))
    return P, W, -(-W // SUB)


def bound(m, R, match, gap, mk=1):
    """prefix_bound of host_score.h for a row-P pass: a read whose B0 is not above it offends."""
    P = LANES * R
    return max(match * (m - P) + slack(gap, mk), match * P)


def fold(row, steps, first_sub, nsub, mk=1):
    """Values per sub-chunk of `row`, row P of a tile's matrix by matrix column: lane LANES - 1 is at column t - (LANES - 1) + 1 at
    step t, and the steps t % mk == mk - 1 are folded."""
    lane = LANES - 1
    val = np.zeros(nsub, dtype=np.float64)
    t = np.arange(lane, steps)
    t = t[t % mk == mk - 1]
    np.maximum.at(val, np.clip(first_sub(t), 0, nsub - 1), row[t - lane + 1])
    return val


def tile_values(x, y, R, chunk, warm, match, mismatch, gap, mk=1):
    """What the device leaves per sub-chunk when the range is cut into tiles of `chunk` own columns behind `warm` warm-up columns: a
    tile starts from a zero border `warm` columns in front of its own, sees padding behind its own last column and in front of the
    range, and the steps of its warm-up count for its first sub-chunk (tests/prefix_rowp.py rowp_tile_values, any fold stride)."""
    n = len(y)
    ntiles = -(-n // chunk)
    if ntiles == 1:
        warm = 0
    spt = chunk // SUB
    steps = -(-(warm + chunk + LANES) // SEG) * SEG
    out = []
    for c in range(ntiles):
        lo, hi = c * chunk, min((c + 1) * chunk, n)
        front = max(0, warm - lo)
        E = tile_matrix(x[:LANES * R], y[lo - warm + front:hi], LANES, R, steps, match, mismatch, gap)
        if front:
            E = np.concatenate([E[:, :1], np.zeros((E.shape[0], front)), E[:, 1:steps + 1 - front]], axis=1)
        out.append(fold(E[LANES * R], steps, lambda t: (t - warm) // SUB, spt, mk))
    return np.concatenate(out)


def range_values(x, y, Rs, scoring, mks=(1, MK)):
    """{(R, mk): value of every sub-chunk} of the range as ONE tile (what the lemma speaks of) for the heights Rs: the oracle's matrix
    of the read's first 2 max(Rs) rows holds row 2 R of every lower prefix; behind the range's last column a tile sees padding, where
    a cell is what its west and north neighbours leave of themselves, a gap each."""
    match, mismatch, gap = scoring
    n = len(y)
    nsub = -(-n // SUB)
    steps = -(-(nsub * SUB + LANES) // SEG) * SEG
    top = LANES * max(Rs)
    H = ob.fill(x[:top], y, ob.F32, match, mismatch, gap).astype(np.float64)
    npad = steps + 1 - (n + 1)
    pad = np.zeros((top + 1, npad + 1))
    pad[:, 0] = H[:, n]
    jg = gap * np.arange(npad + 1, dtype=np.float64)
    for i in range(1, top + 1):
        a = np.maximum(pad[i - 1] - gap, 0.0)
        a[0] = H[i, n]
        pad[i] = np.maximum.accumulate(a + jg) - jg
    out = {}
    for R in Rs:
        row = np.concatenate([H[LANES * R], pad[LANES * R, 1:]])
        for mk in mks:
            out[R, mk] = fold(row, steps, lambda t: t // SUB, nsub, mk)
    return out


class Read:
    """One read against one reference: its sub-chunk values at every height of `Rs`, computed once, and its exact windows."""

    def __init__(self, x, y, scoring, Rs):
        self.x, self.y, self.scoring = x, y, scoring
        self.nsub = -(-len(y) // SUB)
        self.val = range_values(x, y, Rs, scoring)
        self.windows = {}

    def window(self, s):
        if s not in self.windows:
            self.windows[s] = window_best(self.x, self.y, s, *self.scoring)
        return self.windows[s]

    def emulate(self, R, cap, mk=1, vote_Rs=()):
        """The read through a row-P pass at R rows per lane: dict(offender, why, B0, evaluated, result, votes).  votes[r] for r in
        vote_Rs: could a pass at r certify the read as far as THIS sweep can tell — B0 above that bound and that threshold within the
        cap on these values (prefix_bucket: vote)."""
        match, mismatch, gap = self.scoring
        m = len(self.x)
        P, W, D = geometry(m, R, match, gap)
        val = self.val[R, mk]
        out = dict(offender=True, why="", B0=0.0, evaluated=[], result=None, votes={r: False for r in vote_Rs})
        if not val.max() > 0:
            out["why"] = "no prefix value"
            return out
        s0 = int(np.flatnonzero(val == val.max())[0])
        best = {s: self.window(s) for s in range(s0, s0 + D + 1) if s < self.nsub}
        B0 = max(b[0] for b in best.values())
        out.update(B0=B0, evaluated=sorted(best))
        for r in vote_Rs:
            if B0 > bound(m, r, match, gap, mk):
                out["votes"][r] = int(np.count_nonzero(val >= B0 - match * (m - LANES * r) - slack(gap, mk))) <= cap
        if not B0 > bound(m, R, match, gap, mk):
            out["why"] = "B0 cannot certify"
            return out
        flagged = [int(f) for f in np.flatnonzero(val >= B0 - match * (m - P) - slack(gap, mk))]
        if len(flagged) > cap:
            out["why"] = "over the cap"
            return out
        for f in flagged:
            for s in range(f, f + D + 1):
                if s < self.nsub and s not in best:
                    best[s] = self.window(s)
        top = max(b[0] for b in best.values())
        first = min((b[2], b[1]) for b in best.values() if b[0] == top)
        out.update(offender=False, evaluated=sorted(best), result=(top, first[1], first[0]))
        return out


def heights(R, minlen, maxlen, match, gap, mk=1):
    """prefix_heights of host_score.h: the listed R below the bucket's own that a row-P pass is eligible at, then the bucket's own."""
    ok = lambda r: minlen > LANES * r and match * minlen > bound(maxlen, r, match, gap, mk)
    return [r for r in LISTED if r < R and ok(r)] + [R]


def start_height(P, o):
    """prefix_start_height of host_score.h: index of the height the rest of the bucket starts at, -1: the probe has failed."""
    for i in range(len(P) - 1):
        if (o[i] + 2) * P[i + 1] <= PROBE * (P[i + 1] - P[i]):
            return i
    return -1 if 2 * o[-1] > PROBE else len(P) - 1


def emulate_chain(reads, R, cap, mk=1):
    """A bucket of equally long reads (a list of Read, in the order the library sweeps them) through prefix_chain.  Returns
    dict(outcome, launches=[(R, count)], start, riders, second, offenders): positions of the riders, of the reads of the second
    pass, and of the bucket's offenders."""
    n, m = len(reads), len(reads[0].x)
    match, _, gap = reads[0].scoring
    hs = heights(R, m, m, match, gap, mk)
    probe = [r.emulate(hs[0], cap, mk, hs[1:]) for r in reads[:PROBE]]
    poff = [k for k in range(PROBE) if probe[k]["offender"]]
    if 2 * len(poff) > PROBE:                                        # (prefix_bucket gives up: the whole probe offends)
        poff = list(range(PROBE))
    o = [len(poff)] + [sum(1 for e in probe if not e["votes"][r]) for r in hs[1:]]
    launches = [(hs[0], PROBE)]
    st = start_height([LANES * r for r in hs], o)
    if st < 0:
        return dict(outcome="probe_failed", launches=launches, start=None, riders=[], second=[], offenders=set(poff), o=o)
    taller = st + 1 < len(hs)
    riders, pend, offenders = [], [], set()
    for k in poff:
        if st > 0 and probe[k]["votes"][hs[st]]:
            riders.append(k)
        elif taller and probe[k]["votes"][hs[st + 1]]:
            pend.append(k)
        else:
            offenders.add(k)
    order = riders + list(range(PROBE, n))
    rest = [reads[k].emulate(hs[st], cap, mk) for k in order]
    launches.append((hs[st], len(order)))
    roff = [order[k] for k, e in enumerate(rest) if e["offender"]]
    gave_up = 2 * len(roff) > len(order)
    if gave_up:
        roff = list(order)
    B0 = {order[k]: e["B0"] for k, e in enumerate(rest)}
    for k in roff:
        if taller and not gave_up and B0[k] > bound(m, hs[st + 1], match, gap, mk):
            pend.append(k)
        else:
            offenders.add(k)
    if pend:
        second = [reads[k].emulate(hs[st + 1], cap, mk) for k in pend]
        launches.append((hs[st + 1], len(pend)))
        soff = [pend[k] for k, e in enumerate(second) if e["offender"]]
        offenders |= set(pend if 2 * len(soff) > len(pend) else soff)
    return dict(outcome="chain", launches=launches, start=hs[st], riders=riders, second=sorted(pend), offenders=offenders, o=o)


def emulate_parent(reads, R, cap):
    """The flow of a probed bucket below CHAIN reads (tests/prefix_rowp.py emulate_bucket with a low height) on Read states: probe at
    the next lower listed height on the tiles that fold every MK-th step, with a vote for the bucket's own.  Returns
    dict(outcome, launches=[(R, count)], riders, offenders)."""
    n, m = len(reads), len(reads[0].x)
    match, _, gap = reads[0].scoring
    low = max(r for r in LISTED if r < R)
    assert low in heights(R, m, m, match, gap, MK)
    probe = [r.emulate(low, cap, MK, (R,)) for r in reads[:PROBE]]
    off = {k for k in range(PROBE) if probe[k]["offender"]}
    launches = [(low, PROBE)]
    if 2 * len(off) > PROBE:
        off = set(range(PROBE))
    if 16 * len(off) <= PROBE:
        rest = [r.emulate(low, cap, MK) for r in reads[PROBE:]]
        launches.append((low, n - PROBE))
        return dict(outcome="low", launches=launches, riders=[], offenders=off | {PROBE + k for k, e in enumerate(rest) if e["offender"]})
    if 2 * sum(1 for e in probe if not e["votes"][R]) > PROBE:
        return dict(outcome="probe_failed", launches=launches, riders=[], offenders=off)
    riders = sorted(k for k in off if probe[k]["votes"][R])
    order = riders + list(range(PROBE, n))
    rest = [reads[k].emulate(R, cap, MK) for k in order]
    launches.append((R, len(order)))
    return dict(outcome="own_rowp", launches=launches, riders=riders, offenders=(off - set(riders)) | {order[k] for k, e in enumerate(rest) if e["offender"]})
