"""GPU checks of the mirrored float16 cells that keep only K = H - g (sw_score_kernel kSemF16M, Cell::kDiagFromHg; DESIGN.md §3.3
L14 (g)).

Every case compares Context.score_ranges (the unsampled mirrored instance's raw keys) with oracle.score_only, and all fields of
align_batch with oracle.align, and asserts from last_path that the mirrored sampled instance swept the batch.  The inputs sit where
the change can go wrong: (a) hits ending in the first and the last row of every lane (the diagonal and the north term that now come
through the lane above's K); (b) the border between two tiles of one DPP row; (c) best scores below one gap and around it at a lane
border (K above 1.0 crossing lanes); (d) five scorings, the table one with entries at the -1024 cap, and the largest gap the mirrored
cells admit; (e) unequal pairs and a lone last query; (f) 16 x 10 tiles; (g) the uint8 engine; (h) a 20-letter alphabet."""
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import score_instances as si

pytestmark = pytest.mark.gpu

KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
LEN = 150
N = 20_000
DEFAULT = dict(match=3.0, mismatch=-3.0, gap=2.0)


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(pgs):
    return pgs.synth.dna(20261018, N).tobytes()


def hit_read(refb, i, j, front=0, length=LEN):
    """`front` letters the reference does not hold, then the i bases of the reference that end at 0-based column j, then more of that
    letter: the best alignment is those i bases, in rows front + 1 .. front + i."""
    return b"N" * front + bytes(refb[j - i + 1:j + 1]) + b"N" * (length - front - i)


def lane_edge_reads(refb, SL, R):
    """(a): for every lane of the tile a hit that ends in the lane's first row and one that ends in its last row (the last row that
    holds a base, in the last lane)."""
    out = []
    for lane in range(SL):
        for r in (0, R - 1):
            i = min(lane * R + r + 1, LEN)
            if lane * R < LEN:
                out.append(hit_read(refb, i, 1500 + 601 * len(out)))
    return out


def check(ctx, oracle, reads, refb, sem, SL, R, slot=None, ranges=None, **kw):
    """score_ranges against oracle.score_only, align_batch against oracle.align, and the instances that ran."""
    n = len(refb)
    ranges = ranges or [(0, n), (n // 3 + 1, n - 77)]
    with ThreadPoolExecutor(16) as ex:
        exp = list(ex.map(lambda q: oracle.align(q, refb, sem, **kw), reads))
        raw = list(ex.map(lambda rq: oracle.score_only(rq[1], refb[rq[0][0]:rq[0][1]], sem, **kw), [(r, q) for r in ranges for q in reads]))
    raw = np.array(raw, dtype=np.float64).reshape(len(ranges), len(reads))
    ctx.set_option("slot", slot)
    try:
        got = ctx.align_batch(reads, refb, semantics=sem, **kw)
        path, kernel = ctx.last_path(), ctx.last_kernel()
        keys = ctx.score_ranges(ranges, semantics=sem, **kw)
        path_raw = ctx.last_path()
    finally:
        ctx.set_option("slot", None)
    tags = [t for t in path if t.startswith("score[")]
    first = [t for t in tags if "sampled=1" in t]                        # (a read swept again takes an unsampled instance after these)
    assert first and all(re.search(r"cell=f16,SL=%d,R=%d,.*sampled=1,.*idiag=1,mirror=1\]" % (SL, R), t) for t in first), path
    raw_tags = [t for t in path_raw if t.startswith("score[")]
    assert raw_tags and all(re.search(r"cell=f16,SL=%d,R=%d,.*sampled=0,.*idiag=1,mirror=1\]" % (SL, R), t) for t in raw_tags), path_raw
    assert "mirrored, integer diagonal" in kernel["name"], kernel["name"]
    assert keys.shape == raw.shape
    for r, k in zip(*np.nonzero(keys != raw)):
        raise AssertionError("range [%d, %d) read %d (%d bp): raw key %r, oracle.score_only %r" % (
            ranges[r][0], ranges[r][1], k, len(reads[k]), keys[r, k], raw[r, k]))
    for k, (g, e) in enumerate(zip(got, exp)):
        for f in KEYS:
            assert g[f] == e[f], "read %d (%d bp): %s %r, oracle %r" % (k, len(reads[k]), f, g[f], e[f])
    return kernel


@pytest.mark.parametrize("sem", [0, 1])
def test_hits_ending_in_first_and_last_row_of_every_lane(ctx, oracle, ref, sem):
    """(a), and (g) the uint8 engine on the same batch."""
    reads = lane_edge_reads(ref, 8, 19)
    assert len(reads) == 16
    check(ctx, oracle, reads, ref, sem, 8, 19, **DEFAULT)


def test_lanes16(ctx, oracle, ref):
    """(f): option slot=16 gives 16 x 10 tiles; the same kind of batch, one hit per lane edge."""
    reads = lane_edge_reads(ref, 16, 10)
    assert len(reads) == 30                                             # (the sixteenth lane holds no base of a 150 bp read)
    check(ctx, oracle, reads, ref, 0, 16, 10, slot=16, **DEFAULT)


def test_tile_border_inside_a_dpp_row(pgs, ctx, oracle):
    """(b): two tiles of 8 lanes share a DPP row.  The even tile holds an exact copy of the read, so its last lane carries a large value
    down its last rows for a hundred columns; the odd tile — lanes 8 to 15 of the same row, at the same stream positions — holds a copy
    of the read's first 60 bases starting there.  A value leaking across the border into lane 8 would be the north / diagonal term of
    that hit's first row: 180 would read more than the exact copy's 450."""
    n = 60_000
    base = pgs.synth.dna(77, n)
    x = pgs.synth.dna(78, LEN).tobytes()
    y = pgs.synth.dna(79, LEN).tobytes()
    reads = [x, y]
    ctx.align_batch(reads, base.tobytes(), semantics=0, **DEFAULT)
    CL = int(ctx.last_kernel()["chunk_len"])
    assert 256 <= CL and 8 * CL < n, CL
    buf = bytearray(base.tobytes())
    for q, even in ((x, 2), (y, 4)):                                    # query A in the low halves, query B in the high halves
        end = even * CL + CL // 2                                      # last column of the exact copy, in tile `even`
        buf[end - LEN + 1:end + 1] = q
        for d in (9, 9 + 64):                                          # the same stream positions + the lanes' skew, one tile on
            at = end + CL + d
            buf[at:at + 60] = q[:60]
            buf[at + 60:at + 64] = bytes(c for c in b"ACGT" if c != q[60])[:1] * 4
    refb = bytes(buf)
    kernel = check(ctx, oracle, reads, refb, 0, 8, 19, ranges=[(0, n)], **DEFAULT)
    assert int(kernel["chunk_len"]) == CL                               # the copies lie where the tiles are
    assert oracle.score_only(x, refb, 0, **DEFAULT) == 450.0 and oracle.score_only(y, refb, 0, **DEFAULT) == 450.0


@pytest.mark.parametrize("gap", [7.0, 2040.0])
def test_best_scores_around_one_gap_at_a_lane_border(ctx, oracle, ref, gap):
    """(c), and (d) the largest gap mirror_ok admits: hits of one to three bases (3, 6, 9 against a gap of 7) in the last row of the
    first lane, across the border and in the first row of the second lane — every other cell of these reads is below one gap, where K
    lies above 1.0."""
    reads = [hit_read(ref, i, 2000 + 811 * (3 * i + k), front=front) for i in (1, 2, 3) for k, front in enumerate((17, 18, 19))]
    check(ctx, oracle, reads, ref, 0, 8, 19, match=3.0, mismatch=-3.0, gap=gap)


@pytest.mark.parametrize("scoring", [(1.0, -1.0, 1.0), (5.0, -4.0, 7.0)])
def test_scorings_unequal_pairs_and_a_lone_last_query(pgs, ctx, oracle, ref, scoring):
    """(d) the other two identity scorings, on (e) pairs of unequal length (padding rows in one half only) and an odd number of reads."""
    refa = np.frombuffer(ref, dtype=np.uint8)
    lens = (150, 145, 149, 146, 150, 147, 148)
    reads = [pgs.synth.read_from_ref(refa, 500 + k, m, sub_rate=0.03, indel_rate=0.01)[0].tobytes() for k, m in enumerate(lens)]
    check(ctx, oracle, reads, ref, 0, 8, 19, match=scoring[0], mismatch=scoring[1], gap=scoring[2])


@pytest.mark.parametrize("which", [0, 1])
def test_table_at_the_cap_on_a_20_letter_alphabet(pgs, ctx, oracle, which):
    """(d) a table with entries at and below the -1024 cap, with gap 3 and with gap 2040; (h) a 20-letter alphabet (21 reference codes,
    many distinct gap-folded entries per profile plane)."""
    sc = si.capped_table_scorings(pgs)[which]
    refa = pgs.synth.protein(4711, N)
    assert sc.smax(0) * LEN + sc.smax(0) <= 1024
    reads = [pgs.synth.read_from_ref(refa, 900 + k, m, sub_rate=0.05, indel_rate=0.01)[0].tobytes() for k, m in enumerate((150, 150, 148, 146, 150))]
    # a neighbour pair that scores at the cap, inside an otherwise exact read
    a = sc.alpha
    capped = [(a[j], a[j + 1]) for j in range(len(a) - 1) if sc.lut[a[j], a[j + 1]] <= -1024.0]
    q = bytearray(refa[3000:3000 + LEN].tobytes())
    for p in range(10, LEN, 10):
        hit = [c for c, d in capped if d == q[p]]
        if hit:
            q[p] = hit[0]
    assert any(sc.lut[c, d] <= -1024.0 for c, d in zip(q, refa[3000:3000 + LEN]))
    reads.append(bytes(q))
    check(ctx, oracle, reads, refa.tobytes(), 0, 8, 19, **sc.kw())
