"""GPU checks of the row-sampled running maximum of sw_score_kernel (a one-strip MK = 4 instance folds every 4th
step, and then only every RK-th row of a lane and the lane's last): the results of align_batch against the oracle, all fields, on
inputs built for the edges of that argument — (a) hits whose best alignment ends in each row of a lane, in the first, a middle and
the last lane; (b) such hits ending in the last column of a sub-chunk, of a tile and of the reference; (c) near-copies within the
slack of the best one in other sub-chunks, which must lose, and one copy just beyond the slack, which must not even be a candidate;
(d) pairs of unequal length, so that a hit ends just above padding rows.  Both engines on the bench shape (8 lanes x 19 rows), one
16-lane shape, and a batch on float32 cells (3.5 / -3.25 / 2).  None of it may cost a second sweep, except the reads whose best score
lies within the slack of zero (hits of up to four bases), which cannot do without one: exactly those are swept again.

A library whose filter slack is left at 3 gaps still returns the oracle's results on these inputs; it fails (a) at that count (it sweeps
again two of the four reads that need it).  That 3 gaps do not cover the row-sampled fold is shown by tests/test_row_sampled_fold_ref.py."""
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from row_sampled_fold import MK, folded_rows, row_stride, slack

pytestmark = pytest.mark.gpu

N = 3 * 65536 + 4096
KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
LEN = 150
ACGT = b"ACGT"
DEFAULT = (3.0, -3.0, 2.0)
# name: (semantics, scoring, option slot, lanes, rows per lane)
CONFIGS = {
    "bench_f32": (0, DEFAULT, None, 8, 19),
    "bench_u8": (1, DEFAULT, None, 8, 19),
    "lanes16_f32": (0, DEFAULT, 16, 16, 10),
    "f32cells": (0, (3.5, -3.25, 2.0), None, 8, 19),
}


@pytest.fixture(scope="module")
def ref(pgs):
    return pgs.synth.dna(911, N).tobytes()


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def hit_read(ref, i, j, length=LEN):
    """A read whose first i bases are the reference's, ending at 0-based column j; the rest is a letter the reference does not hold (with
    gaps cheaper than a match, letters that merely mismatch along the diagonal would still extend the alignment through gaps), so that
    the hit's best alignment ends in row i with score match * i."""
    return bytes(ref[j - i + 1:j + 1]) + b"N" * (length - i)


def lanes3(SL, R):
    return sorted({0, SL // 2, (LEN - 1) // R})                        # first, a middle and the last lane that holds rows of a read


def two_class_reference(seed, ends):
    """A reference of N random G / T with one random A / C string of 150 bases ending at each 0-based column of `ends`.  A read made of a
    piece of such a string (and N) scores only inside the planted strings, so that a hit of a single base is still the read's best
    alignment, and only the few sub-chunks that hold a planted string can be candidates: fewer than any query's budget."""
    rng = np.random.default_rng(seed)
    buf = bytearray(rng.choice(list(b"GT"), N).astype(np.uint8))
    for j in ends:
        buf[j - LEN + 1:j + 1] = bytes(rng.choice(list(b"AC"), LEN).astype(np.uint8))
    return bytes(buf)


def batches_a(SL, R):
    """One batch per lane: read r's hit — the last i bases of its own planted string — ends in row r of the lane."""
    out = []
    for k, lane in enumerate(lanes3(SL, R)):
        rows = [r for r in range(R) if lane * R + r + 1 <= LEN]
        ends = [3000 + 1201 * r + 25_013 * k for r in rows]
        refb = two_class_reference(100 + lane, ends)
        out.append(([hit_read(refb, lane * R + r + 1, j) for r, j in zip(rows, ends)], refb))
    return out


def batch_b(SL, R):
    RK = row_stride(R)
    rows = sorted({r for r in range(R) if r % RK == 0} | {R - 1})      # the rows farthest above the next folded one, and the last
    ends = (100_095, 65_535, 131_071, N - 1)                           # last column of a sub-chunk, of a tile (twice), of the reference
    refb = two_class_reference(200, ends)
    reads = [hit_read(refb, lane * R + r + 1, j) for j in ends for lane in lanes3(SL, R) for r in rows if lane * R + r + 1 <= LEN]
    return reads, refb


def reads_d(ref):
    """Lengths 129, 130, 130, 133, 133 and four of 150 (one tile shape: more than 128 rows): sorted by length, the pairs of a workgroup
    are of unequal length; the short reads' hits end in their last row or two rows above it, just above the padding rows of their tile."""
    out = []
    for k, (length, i) in enumerate(((133, 133), (133, 131), (130, 130), (130, 128), (129, 129))):
        out.append(hit_read(ref, i, 40_000 + 2000 * k, length=length))
    for k in range(4):
        out.append(hit_read(ref, LEN - k, 55_000 + 2000 * k))
    return out


def plant_near_copies(ref, SL, R, scoring, oracle):
    """Part (c).  The read's hit of i bases ends in a folded row at a folded step, so the sweep's key is its exact score M.  Copies of the
    hit with `a` extra reference bases (a gaps each) and without its first b bases (b matches) score M - a g - b match: one per reachable
    value 1 .. slack, each in a sub-chunk of its own (reference 1), one at slack + 1 (reference 2), and a second exact copy (reference 3)."""
    match, mismatch, gap = scoring
    lane = (76 - 1) // R if SL == 8 else (80 - 1) // R
    i = (lane + 1) * R                                                 # 76 on 8 x 19, 80 on 16 x 10: the lane's last row; at match 3 the
    assert (i - 1) % R in folded_rows(R)                               # score stays below the uint8 engine's cap
    j = 141_000
    j += (MK - 1 - lane - j) % MK                                      # (j + lane) % MK == MK - 1: a folded step
    read = hit_read(ref, i, j)
    seg = ref[j - i + 1:j + 1]
    M = match * i
    sl = slack(R, gap)

    def variant(a, b):
        v = bytearray(seg[b:])
        for k in range(a):
            p = 10 + 8 * k + k
            v.insert(p, next(c for c in ACGT if c != v[p] and c != v[p - 1]))
        return bytes(v)

    def put(buf, at, a, b):
        v = variant(a, b)
        free = next(c for c in ACGT if c not in read[:b])               # nothing in front of the copy matches the read's first b bases
        buf[at - 4:at] = bytes([free]) * 4
        buf[at:at + len(v)] = v
        win = bytes(buf[at - 8:at + len(v) + 8])
        got = oracle.align(read, win, 0, match, mismatch, gap)["score"]
        assert got == M - a * gap - b * match, "the planted copy (a=%d, b=%d) scores %r, built for %r" % (a, b, got, M - a * gap - b * match)

    best = {}
    for a in range(8):
        for b in range(4):                                             # (at most three letters in front: a fourth is free)
            d = a * gap + b * match
            if d > 0 and (d not in best or a + b < sum(best[d])):
                best[d] = (a, b)
    near = sorted(d for d in best if d <= sl)
    beyond = min(d for d in best if d > sl)
    assert beyond <= sl + 1 and len(near) >= sl - 2, (near, beyond)    # (3 / -3 / 2: every value 2 .. 14, and 15)
    r1 = bytearray(ref)
    for k, d in enumerate(near):
        put(r1, 143_000 + 2048 * k, *best[d])
    r2 = bytearray(r1)
    put(r2, 190_000, *best[beyond])
    r3 = bytearray(r1)
    put(r3, 195_000, 0, 0)
    companion = hit_read(ref, LEN, 30_000)                             # an exact read: its only candidates are its own sub-chunks
    return [read, companion], bytes(r1), bytes(r2), bytes(r3)


def expected_ops_per_cell(sem, scoring, SL, R):
    """valu_ops_per_cell of host_score.h for the sampled float16 / float32 instance: add, maximum3, add per row, a quarter of a maximum3
    per two folded rows, the DPP move and the per-step overhead."""
    folded = len(folded_rows(R))
    per_step = 3.0 * R + 0.25 * ((folded + 1) // 2) + 1 + (4.0 if SL == 8 else 3.0)
    float32_cells = sem == 0 and any(v != int(v) for v in scoring)
    return per_step / ((1 if float32_cells else 2) * R)


def run(ctx, oracle, name, reads, refb):
    sem, scoring, slot, SL, R = CONFIGS[name]
    with ThreadPoolExecutor(16) as ex:
        exp = list(ex.map(lambda q: oracle.align(q, refb, sem, *scoring), reads))
    ctx.set_option("slot", slot)
    try:
        got = ctx.align_batch(reads, refb, semantics=sem, match=scoring[0], mismatch=scoring[1], gap=scoring[2])
        path, counters, kernel = ctx.last_path(), ctx.last_counters(), ctx.last_kernel()
    finally:
        ctx.set_option("slot", None)
    tags = [t for t in path if t.startswith("score[")]
    first = [t for t in tags if "sampled=1" in t]                      # (a read swept again takes an unsampled instance after these)
    assert first and all(re.search(r"SL=%d,R=%d,.*sampled=1,rows=%d," % (SL, R, row_stride(R)), t) for t in first), path
    print("%s: %d reads, candidates %d, requeried %d, whole_batch_again %d" % (
        name, len(reads), counters["candidates"], counters["requeried"], counters["whole_batch_again"]))
    for k, (g, e) in enumerate(zip(got, exp)):
        for f in KEYS:
            assert g[f] == e[f], "%s, read %d (%d bp): %s %r, oracle %r" % (name, k, len(reads[k]), f, g[f], e[f])
    # No second sweep — except for the reads that cannot do without one: a best score within the slack of zero (a hit of up to four
    # bases in the first lane's first rows) may have decayed to nothing before the fold saw it, in any of the reference's 784
    # sub-chunks, which is more than a query's budget.  Exactly those reads are swept again, each by itself.
    blind = sum(1 for e in exp if e["score"] <= slack(R, scoring[2]))
    assert blind <= 4 and 2 * blind <= len(reads)
    assert counters["requeried"] == blind and counters["whole_batch_again"] == 0, (counters, blind)
    assert kernel["valu_ops_per_cell"] == pytest.approx(expected_ops_per_cell(sem, scoring, SL, R), rel=1e-12), kernel
    assert "every 4th step" in kernel["name"], kernel["name"]
    return counters["candidates"]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hits_ending_in_every_row(ctx, oracle, name):
    """(a): every row of the first, a middle and the last lane."""
    _, _, _, SL, R = CONFIGS[name]
    for reads, refb in batches_a(SL, R):
        run(ctx, oracle, name, reads, refb)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hits_ending_in_last_columns(ctx, oracle, name):
    """(b): the same kind of hit in the last column of a sub-chunk, of a tile and of the reference."""
    _, _, _, SL, R = CONFIGS[name]
    run(ctx, oracle, name, *batch_b(SL, R))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_near_copies_lose_and_beyond_the_slack_is_no_candidate(ctx, oracle, ref, name):
    """(c): copies 1 .. slack below the best lose; a copy slack + 1 below adds no candidate; a second exact copy adds one."""
    _, scoring, _, SL, R = CONFIGS[name]
    reads, r1, r2, r3 = plant_near_copies(ref, SL, R, scoring, oracle)
    c1 = run(ctx, oracle, name, reads, r1)
    c2 = run(ctx, oracle, name, reads, r2)
    c3 = run(ctx, oracle, name, reads, r3)
    assert c2 == c1, "a copy %g below the best (slack %g) became a candidate: %d candidates, %d without it" % (
        slack(R, scoring[2]) + 1, slack(R, scoring[2]), c2, c1)
    assert c3 > c1, "a second exact copy is no candidate: %d candidates, %d without it" % (c3, c1)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_unequal_pairs_above_padding_rows(ctx, oracle, ref, name):
    """(d): reads of 129 - 133 bp paired with longer ones."""
    run(ctx, oracle, name, reads_d(ref), ref)
