"""Shared by tests/test_prefix_thin_ref.py, tests/test_gpu_prefix_thin_items.py and tests/test_gpu_prefix_thin_flow.py: the thin stage
of the prefix filter (sw_prefix_thin_kernel.h, host_pipeline.h prefix_bucket round 2) emulated in numpy on the
oracle's matrices, and the chain of tests/prefix_cascade.py with that stage in every pass.

A pass at P rows flags sub-chunk s of a read where row P of the read's first P rows reaches thr = B0 - smax (m - P).  The thin stage
evaluates the read's first P2 = 38 rows over the item's window [s SUB - 64 - warm2, (s + 1) SUB + W12), clipped to the range, from a
zero border, and keeps every sub-chunk in which row P2 reaches thr2 = B0 - smax (m - P2) on the item's own columns, s SUB - 63 onwards."""
import math

import numpy as np

from oracle import binding as ob
from prefix_cascade import PROBE, bound, geometry as chain_geometry, heights, start_height
from prefix_filter import LAG, LANES
from row_sampled_fold import SUB

P2 = 38                                                              # kThinP2 of host_score.h
THIN_CAP_MAX = 1024                                                  # kThinCapMax
ITEMS_MAX = 65536                                                    # kThinItemsMax: flags of all the reads over the cap of one pass
MIN_FLAGS = 1024                                                     # kThinMinFlags


def geometry(m, P, match, gap, sub=SUB):
    """thin_plan of host_pipeline.h: W12, warm2, D2, nout."""
    W12 = (P2 - P) + int(match * (P2 - P) // gap)
    warm2 = P2 + math.ceil(P2 * match / gap)
    W2 = (m - P2) + int(match * (m - P2) // gap)
    return dict(W12=W12, warm2=warm2, D2=-(-W2 // sub), nout=3 + (W12 - 1) // sub)


def thin_cap(qcap):
    """thin_flag_cap of host_score.h: the flags a read may list for the thin stage."""
    return max(qcap, THIN_CAP_MAX)


def bound2(m, match):
    """What B0 must exceed for row P2 to certify the read: prefix_bound(t, m, P2, 0, true)."""
    return match * max(m - P2, P2)


def item_window(n, s, W12, warm2, sub=SUB):
    """(w_lo, own_lo, w_hi) of item s in a range of n columns, 0-based."""
    own_lo = max(0, s * sub - LAG)
    return max(0, own_lo - 1 - warm2), own_lo, min((s + 1) * sub + W12, n)


def item_values(x, y, s, P, scoring, sub=SUB):
    """What the kernel returns for item (x, s) of the range y: the maximum of row P2 of the oracle's matrix of x[:P2] against the
    item's window, per sub-chunk s - 1 + t over the own columns inside it; -1 where there is none."""
    match, mismatch, gap = scoring
    g = geometry(len(x), P, match, gap, sub)
    w_lo, own_lo, w_hi = item_window(len(y), s, g["W12"], g["warm2"], sub)
    out = [-1.0] * g["nout"]
    if w_hi <= own_lo:
        return out
    row = ob.fill(x[:P2], y[w_lo:w_hi], ob.F32, match, mismatch, gap)[P2, 1:]
    for t in range(max(0, s - 1), (w_hi - 1) // sub + 1):
        a, b = max(own_lo, t * sub), min(w_hi, (t + 1) * sub)
        if a < b:
            out[t - (s - 1)] = float(row[a - w_lo:b - w_lo].max())
    return out


def emulate_pass(reads, R, qcap, vote_Rs=(), thin=True):
    """prefix_bucket on the step tiles (fold stride 1, no slack) for `reads` (prefix_cascade.Read, equally long) at R rows per lane.
    Returns dict(reads=[dict(offender, why, B0, votes, thinned)], gave_up, items, kept, thinned, candidates): the pass's thin launch
    (0 items: none) and what it sent to the locate stage in both rounds.  Sub-chunks are SUB columns long: on the device a pass of ONE
    read runs on sub-chunks of 64 (host_score.h score_sub_len), which changes D, the flags and `candidates` — the device tests keep
    two reads or more in every pass they compare."""
    m = len(reads[0].x)
    match, _, gap = reads[0].scoring
    P, _, D = chain_geometry(m, R, match, gap)
    g = geometry(m, P, match, gap)
    thin = thin and P < P2 < m
    fcap = thin_cap(qcap) if thin else qcap
    st = []
    for r in reads:
        val = r.val[R, 1]
        e = dict(offender=True, why="", B0=0.0, votes={v: False for v in vote_Rs}, thinned=False, f1=[], flagged=[])
        st.append(e)
        if not val.max() > 0:
            e["why"] = "no prefix value"
            continue
        s0 = int(np.flatnonzero(val == val.max())[0])
        e["f1"] = [s for s in range(s0, s0 + D + 1) if s < r.nsub]
        e["B0"] = B0 = max(r.window(s)[0] for s in e["f1"])
        for v in vote_Rs:
            if B0 > bound(m, v, match, gap):
                e["votes"][v] = int(np.count_nonzero(val >= B0 - match * (m - LANES * v))) <= qcap
        if not B0 > bound(m, R, match, gap):
            e["why"] = "B0 cannot certify"
            continue
        e["offender"] = False
        e["flagged"] = [int(f) for f in np.flatnonzero(val >= B0 - match * (m - P))]
    out = dict(reads=st, gave_up=False, items=0, kept=0, thinned=0, candidates=0)

    def give_up():
        if 2 * sum(1 for e in st if e["offender"]) > len(st):
            for e in st:
                e["offender"] = True
            out["gave_up"] = True
        return out["gave_up"]

    if give_up():
        return out
    ok2 = lambda e: thin and e["B0"] > bound2(m, match)
    room = ITEMS_MAX                                                 # the reads over the cap with the fewest flags first, while there is room
    for e in sorted((e for e in st if not e["offender"] and len(e["flagged"]) > qcap), key=lambda e: len(e["flagged"])):
        if len(e["flagged"]) <= min(fcap, room) and ok2(e):
            e["thinned"] = True
            room -= len(e["flagged"])
        else:
            e.update(offender=True, why="over the cap")
    if give_up():
        return out
    live = [(r, e) for r, e in zip(reads, st) if not e["offender"]]
    fresh = sum(1 for _, e in live if e["thinned"] or ok2(e) for s in e["flagged"] if s not in e["f1"])
    everybody = thin and fresh > MIN_FLAGS
    ncand = sum(len(e["f1"]) for e in st)
    for r, e in live:
        if everybody and ok2(e) and e["flagged"]:
            e["thinned"] = True
        if not e["thinned"]:
            continue
        thr2 = e["B0"] - match * (m - P2)
        kept = set()
        for s in e["flagged"]:
            for t, v in enumerate(item_values(r.x, r.y, s, P, r.scoring)):
                if v >= thr2:
                    kept.add(s - 1 + t)
        out["items"] += len(e["flagged"])
        out["kept"] += len(kept)
        out["thinned"] += 1
        e["kept"] = sorted(kept)
        if len(kept) > qcap:
            e.update(offender=True, why="over the cap after thinning")
    for r, e in live:
        if e["offender"]:
            continue
        subs, reach = (e["kept"], g["D2"]) if e["thinned"] else (e["flagged"], D)
        f2 = {t for s in subs for t in range(s, s + reach + 1) if t < r.nsub}
        ncand += len(f2 - set(e["f1"]))
    out["candidates"] = ncand
    return out


def emulate_chain(reads, R, qcap, thin=True):
    """prefix_cascade.emulate_chain with the thin stage in every pass.  Adds passes=[(R, count, items, kept)], thinned, thin_items and
    candidates (what the chain's passes sent to the locate stage; the sweep of the bucket's offenders counts its own on top)."""
    n, m = len(reads), len(reads[0].x)
    match, _, gap = reads[0].scoring
    hs = heights(R, m, m, match, gap, 1)
    probe = emulate_pass(reads[:PROBE], hs[0], qcap, hs[1:], thin)
    passes = [probe]
    launches = [(hs[0], PROBE)]
    poff = [k for k in range(PROBE) if probe["reads"][k]["offender"]]
    o = [len(poff)] + [sum(1 for e in probe["reads"] if not e["votes"][r]) for r in hs[1:]]
    st = start_height([LANES * r for r in hs], o)

    def result(**kw):
        kw.update(launches=launches, o=o, passes=[(r, c, p["items"], p["kept"]) for (r, c), p in zip(launches, passes)],
                  thinned=sum(p["thinned"] for p in passes), thin_items=sum(p["items"] for p in passes),
                  candidates=sum(p["candidates"] for p in passes))
        return kw

    if st < 0:
        return result(outcome="probe_failed", start=None, riders=[], second=[], offenders=set(poff))
    taller = st + 1 < len(hs)
    riders, pend, offenders = [], [], set()
    for k in poff:
        if st > 0 and probe["reads"][k]["votes"][hs[st]]:
            riders.append(k)
        elif taller and probe["reads"][k]["votes"][hs[st + 1]]:
            pend.append(k)
        else:
            offenders.add(k)
    order = riders + list(range(PROBE, n))
    rest = emulate_pass([reads[k] for k in order], hs[st], qcap, (), thin)
    passes.append(rest)
    launches.append((hs[st], len(order)))
    for k, e in zip(order, rest["reads"]):
        if not e["offender"]:
            continue
        if taller and not rest["gave_up"] and e["B0"] > bound(m, hs[st + 1], match, gap):
            pend.append(k)
        else:
            offenders.add(k)
    if pend:
        second = emulate_pass([reads[k] for k in pend], hs[st + 1], qcap, (), thin)
        passes.append(second)
        launches.append((hs[st + 1], len(pend)))
        offenders |= {k for k, e in zip(pend, second["reads"]) if e["offender"]}
    return result(outcome="chain", start=hs[st], riders=riders, second=sorted(pend), offenders=offenders)
