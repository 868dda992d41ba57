"""The seeded flow of the chained prefix filter (host_pipeline.h prefix_seeded) on the oracle's full matrices, no GPU:

  * lemma L19, row-P variant with MK = 1, at the LOW heights P = 16 and 20 (kR2Step), as tests/test_prefix_cascade_ref.py has it for
    P = 26, 32 and 38;
  * the flow itself emulated in numpy — seeds, hits, cluster, window, B0, the height by a given background table, flags, windows —
    reproduces the oracle's (score, end_x, end_y) for planted reads, including a read with no intact seed and a read whose best
    alignment is NOT where its seeds cluster (B0 < B);
  * the library's own cluster rule, seed hash and seed-length rule (host functions of sw_seed_kernel.h behind the C-ABI) against
    restatements."""
import math

import numpy as np
import pytest

from oracle import binding as ob
from prefix_cascade import LANES, Read, bound, geometry
from prefix_filter import covers
from row_sampled_fold import SUB

LOW = [8, 10]                                                        # kR2Step
HEIGHTS = [8, 10, 13, 16, 19]                                        # prefix_heights_seeded for 150 bp reads
M = 150
N = 60_000 + 77
SCORING = (3.0, -3.0, 2.0)
CAP = 64 + 1024 // 8
HIT_CAP = 32                                                         # kSeedHitCap
END_PAD = 16                                                         # kSeedEndPad
BASE, MIX = 0x01000193, 0x9E3779B1                                   # kSeedBase, kSeedMix


def _dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(list(letters), n).astype(np.uint8))


def _mutate(rng, x, places):
    x = bytearray(x)
    for at in places:
        x[at] = b"ACGT"[(b"ACGT".index(x[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(x)


def _truth(x, y):
    H = ob.fill(x, y, ob.F32, *SCORING)
    B = float(H.max())
    cells = [(int(i), int(j)) for i, j in np.argwhere(H == B)]
    return B, cells, H


# ---- restatements of sw_seed_kernel.h ---------------------------------------------------------------------------------------------
def seed_k(letters, minlen, n):
    for k in range(1, 33):
        per_read = minlen // k
        if per_read < 4:
            return 0
        if letters ** k >= per_read * n:
            return k
    return 0


def seed_hash(codes):
    h = 0
    for c in codes:
        h = (h * BASE + c + 1) & 0xFFFFFFFF
    return h


def seed_hits(x, y, k):
    index = {}
    for p in range(len(y) - k + 1):
        index.setdefault(y[p:p + k], []).append(p)
    periodic = lambda s: any(s[:-p] == s[p:] for p in range(1, len(s) // 2 + 1))      # seed_periodic: such seeds are left out
    return sorted((p - off, off) for off in range(0, len(x) - k + 1, k) if not periodic(x[off:off + k]) for p in index.get(x[off:off + k], []))


def cluster(hits, width):
    """For every hit as the anchor the hits with start in [anchor, anchor + width]: most distinct offsets, then the lowest start."""
    best = None
    for a, _ in sorted(hits):
        inside = [(s, o) for s, o in hits if a <= s <= a + width]
        d = len({o for _, o in inside})
        if best is None or d > best[2]:
            best = (a, max(s for s, _ in inside), d)
    return best


def emulate_seeded(read, k, table):
    """One read through the seeded flow.  table[R] = function deficit -> expected background flags.  dict(seeded, B0, R, result)."""
    x, y = read.x, read.y
    match, mismatch, gap = read.scoring
    m, n = len(x), len(y)
    hits = seed_hits(x, y, k)
    out = dict(seeded=False, B0=0.0, R=None, result=None, evaluated=[])
    if not hits or len(hits) > HIT_CAP:
        return out
    lo, hi, _ = cluster(hits, -(-int(match * m) // int(gap)))
    c_lo, c_hi = max(0, lo + m - 1 - END_PAD), min(n - 1, hi + m - 1 + END_PAD)
    if c_lo > c_hi:
        return out
    best = {s: read.window(s) for s in range(c_lo // SUB, c_hi // SUB + 1)}
    B0 = max(b[0] for b in best.values())
    if not B0 > 0:
        return out
    out.update(seeded=True, B0=B0)
    for R in HEIGHTS:
        P = LANES * R
        if m > P and B0 > bound(m, R, match, gap) and table[R](match * m - B0) <= CAP:
            break
    else:
        return out                                                   # no height: the full sweep
    P, W, D = geometry(m, R, match, gap)
    flagged = [int(f) for f in np.flatnonzero(read.val[R, 1] >= B0 - match * (m - P))]
    if len(flagged) > CAP:
        return out
    for f in flagged:
        for s in range(f, f + D + 1):
            if s < read.nsub and s not in best:
                best[s] = read.window(s)
    top = max(b[0] for b in best.values())
    first = min((b[2], b[1]) for b in best.values() if b[0] == top)
    out.update(R=R, result=(top, first[1], first[0]), evaluated=sorted(best))
    return out


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(6203)
    y = bytearray(_dna(rng, N))
    copy = lambda o, m=M: bytes(y[o:o + m])
    k = seed_k(4, M, N)
    # a read whose best alignment is NOT where its seeds cluster, on a pass that RUNS: the true copy differs from the read in three
    # letters of three different seeds (B = 3 m - 18, M // k - 3 intact seeds), while a decoy further LEFT differs in every second
    # letter of ONE seed (lone mismatches, 6 each: score 3 m - 30, M // k - 1 intact seeds).  The cluster rule takes the decoy, so B0 is the decoy's score, below B, and
    # still clears the bound of every height (3 (m - 16) = 402 < 420)
    far = _mutate(rng, copy(150 * SUB + 31), [5, 8 * k + 5, 14 * k + 5])
    y[20 * SUB + 9:20 * SUB + 9 + M] = _mutate(rng, far, list(range(7 * k, 8 * k, 2)))
    # no seed at all: a letter the reference does not hold in every seed
    lost = bytearray(copy(200 * SUB + 60))
    for j in range(M // k):
        lost[j * k + k // 2] = ord("N")
    deleted = copy(110 * SUB + 40, M + 1)
    reads = dict(exact=copy(40 * SUB + 17),
                 one_sub=_mutate(rng, copy(60 * SUB + 3), [70]),
                 three_subs=_mutate(rng, copy(133 * SUB + 200), [5, 77, 140]),
                 indel_in_a_seed=deleted[:k + 3] + deleted[k + 4:],      # one reference letter missing inside the second seed
                 no_intact_seed=bytes(lost),
                 elsewhere=far,
                 first_columns=copy(0), last_columns=copy(N - M))
    y = bytes(y)
    out = {}
    for name, x in reads.items():
        B, cells, H = _truth(x, y)
        out[name] = (Read(x, y, SCORING, HEIGHTS), B, cells, {R: H[LANES * R].astype(np.float64) for R in HEIGHTS})
    return k, out


@pytest.mark.parametrize("R", LOW)
def test_lemma_at_the_low_heights(case, R):
    """L19, row-P variant without slack, at P = 16 and 20: every cell that holds B lies at most W columns right of a row-P cell of
    value >= B - smax (m - P), which the fold sees in its own sub-chunk or the next; and a pass at that height on the oracle's values
    reproduces the oracle wherever it does not offend."""
    match, mismatch, gap = SCORING
    k, reads = case
    P, W, D = geometry(M, R, match, gap)
    assert P in (16, 20) and bound(M, R, match, gap) == match * (M - P) > match * P
    for name, (read, B, cells, rows) in reads.items():
        val = read.val[R, 1]
        if B > bound(M, R, match, gap):
            for i, j in cells:
                seg = rows[R][max(0, j - W):j + 1]
                assert i > P and seg.max() >= B - match * (i - P) >= B - match * (M - P), (name, R, i, j)
                c = max(0, j - W) + int(np.argmax(seg))
                s = (c - 1) // SUB
                assert val[s:s + 2].max() >= B - match * (M - P), (name, R, i, j, c)
        e = read.emulate(R, CAP)
        assert e["B0"] <= B
        print("R=%d %-16s B=%g offender=%d %s" % (R, name, B, e["offender"], e["why"]))
        if e["offender"]:
            assert e["why"] == "over the cap" or e["B0"] <= bound(M, R, match, gap), (name, R, e["why"], e["B0"])
            continue
        for i, j in cells:
            assert covers(e["evaluated"], j - 1), (name, R, i, j, e["evaluated"])
        first = min((j, i) for i, j in cells)
        assert e["result"] == (B, first[1], first[0]), (name, R, e["result"], B, first)
    # an exact copy is certified at both low heights: its threshold 3 P is out of the background's reach on 60 k columns
    assert not reads["exact"][0].emulate(R, CAP)["offender"]


def test_seeded_flow_reproduces_the_oracle(case):
    match, mismatch, gap = SCORING
    k, reads = case
    assert k == seed_k(4, M, N) and M // k >= 4
    # a background table in the shape of the measured ones: what a deficit d draws at P rows falls fast with P
    table = {R: (lambda d, P=LANES * R: 0.0 if d <= 0 else 1000.0 * math.exp((d - 1.5 * P + 14.0) / 3.0)) for R in HEIGHTS}
    seen = {}
    for name, (read, B, cells, rows) in reads.items():
        e = emulate_seeded(read, k, table)
        seen[name] = e
        print("%-16s B=%g seeded=%d B0=%g R=%s" % (name, B, e["seeded"], e["B0"], e["R"]))
        assert e["B0"] <= B
        if e["result"] is None:
            continue
        first = min((j, i) for i, j in cells)
        assert e["result"] == (B, first[1], first[0]), (name, e["result"], B, first)
        for i, j in cells:
            assert covers(e["evaluated"], j - 1), (name, i, j)
    # no intact seed: no hit, no seed B0 — the seedless group's business
    lost = seen["no_intact_seed"]
    assert seed_hits(reads["no_intact_seed"][0].x, reads["no_intact_seed"][0].y, k) == []
    assert not lost["seeded"] and lost["B0"] == 0 and lost["result"] is None
    assert all(seen[n]["seeded"] and seen[n]["result"] is not None for n in ("exact", "one_sub", "three_subs", "indel_in_a_seed", "first_columns", "last_columns"))
    assert seen["exact"]["B0"] == match * M and seen["exact"]["R"] == HEIGHTS[0]
    assert seen["exact"]["R"] <= seen["one_sub"]["R"] <= seen["three_subs"]["R"]
    # B0 < B on a pass that runs: the seeds cluster at the decoy, B0 is the decoy's score, and the thresholds taken from that lower B0
    # still find B and its first maximum at the true copy (L19 asks of B0 only that it be an exact alignment score <= B)
    far, (read, B, cells, rows) = seen["elsewhere"], reads["elsewhere"]
    hits = seed_hits(read.x, read.y, k)
    lo, hi, distinct = cluster(hits, -(-int(match * M) // int(gap)))
    assert abs(lo - (20 * SUB + 9)) <= 2 and distinct >= M // k - 1                       # the decoy wins the cluster rule
    at = 20 * SUB + 9
    decoy = float(ob.fill(read.x, read.y[at - 100:at + M + 100], ob.F32, *SCORING).max())      # the oracle's best around the decoy
    assert B == match * M - 18 and far["seeded"] and far["B0"] == decoy == match * M - 6 * ((k + 1) // 2) < B
    assert far["B0"] > bound(M, HEIGHTS[0], match, gap) and far["R"] is not None and far["result"] is not None
    first = min((j, i) for i, j in cells)
    assert first[0] > 150 * SUB and far["result"] == (B, first[1], first[0]), (far, B, first)


def test_cluster_rule(pgs):
    lib = pgs.capi.seed_cluster
    assert lib([], 10) is None
    cases = [
        ([(100, 0), (100, 16), (100, 32)], 10),                      # one diagonal
        ([(100, 0), (103, 16), (500, 0), (500, 16), (500, 32)], 10),  # two clusters: the richer one
        ([(100, 0), (100, 16), (500, 0), (500, 16)], 10),            # a tie: the lowest diagonal
        ([(100, 0), (105, 0), (109, 0), (300, 0), (300, 16)], 10),   # the same offset thrice counts once
        ([(100, 0), (111, 16), (122, 32)], 10),                      # a chain wider than the window is no cluster
        ([(-40, 0), (-38, 16), (7, 32)], 4),                         # negative starts
        ([(5, 16), (5, 0), (3, 32), (4, 48)], 2),                    # unsorted input
    ]
    for hits, width in cases:
        assert lib(hits, width) == cluster(hits, width), (hits, width, lib(hits, width), cluster(hits, width))
    assert lib(cases[1][0], 10) == (500, 500, 3) and lib(cases[2][0], 10) == (100, 100, 2)
    assert lib(cases[3][0], 10) == (300, 300, 2) and lib(cases[4][0], 10)[2] == 1
    rng = np.random.default_rng(77)
    for _ in range(50):
        hits = [(int(rng.integers(-50, 400)), 16 * int(rng.integers(0, 9))) for _ in range(int(rng.integers(1, HIT_CAP + 1)))]
        width = int(rng.integers(0, 60))
        assert lib(hits, width) == cluster(hits, width), (hits, width)


def test_hash_and_seed_length_rule(pgs):
    rng = np.random.default_rng(78)
    for letters in (4, 20, 256):
        for k in (1, 3, 15, 32):
            codes = bytes(rng.integers(0, letters, k + 5, dtype=np.uint8))
            assert pgs.capi.seed_hash(codes[:k]) == seed_hash(codes[:k])
            # it rolls: h' = h B + (c_in + 1) - (c_out + 1) B^k
            h = seed_hash(codes[:k])
            for p in range(5):
                h = (h * BASE + codes[p + k] + 1 - (codes[p] + 1) * pow(BASE, k, 1 << 32)) & 0xFFFFFFFF
                assert h == pgs.capi.seed_hash(codes[p + 1:p + 1 + k])
        for minlen in (3, 16, 50, 150, 1000):
            for n in (1, 1000, 60_077, 4 << 20, 50_000_000, 3_000_000_000):
                assert pgs.capi.seed_k(letters, minlen, n) == seed_k(letters, minlen, n), (letters, minlen, n)
    assert pgs.capi.seed_k(4, 150, 50_000_000) == 15                  # 4^15 = 1.07e9 >= 10 x 5e7 > 4^14
    assert pgs.capi.seed_k(20, 150, 50_000_000) == 7 and pgs.capi.seed_k(256, 150, 50_000_000) == 4
    assert pgs.capi.seed_k(4, 40, 50_000_000) == 0                    # fewer than 4 seeds would fit
    assert pgs.capi.seed_k(1, 150, 1000) == 0
