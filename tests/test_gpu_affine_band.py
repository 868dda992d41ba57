"""Banded lists of (query, window) pairs under affine gaps on the device (mi355_sw_affine_pairs_run_band / _trace_band) against
tests/affine_band_ref.py applied to the slice y[left:right] with the pair's band.  Every case runs through the run and the trace
call, on the default dispatch (sw_affine_band_kernel) and under option no_affine_band (the exact kernel under a band): all must
equal the checker field for field, every emitted cell must lie in the band, and the path must show which kernel ran.  Shapes are the
smallest at which the band kernel can go wrong: every instance at the edges of its band widths, rows 1, 2 and 512, one column, gaps that
cross lane boundaries along the row (E) and down the columns (F), paths that run along either edge of the band, clipped and missing bands,
ties between lanes, rows and columns.  Planted features are first shown to matter by the checkers alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import affine_band_ref as br, affine_ref, score_instances as si

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_KERNEL_H = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "sw_affine_band_kernel.h")
FIELDS = ("score", "end_x", "end_y")
TRACE_FIELDS = FIELDS + ("begin_x", "begin_y", "pos", "cons_x", "cons_y", "cigar")
DEFAULT = dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0)


def compiled_R():
    with open(BAND_KERNEL_H) as f:
        m = re.search(r"constexpr\s+int\s+kBandR\[\]\s*=\s*\{([^}]*)\}", f.read())
    return tuple(int(v) for v in m.group(1).split(","))


BAND_R = compiled_R()
WMAX = 16 * BAND_R[-1]


def instance_of(W):
    return next((r for r in BAND_R if 16 * r >= W), 0)


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def effective(xs, pairs, k):
    q, left, right, lo, hi = pairs[k]
    return br.effective_band(len(xs[q]), right - left, lo, hi)


def expected(xs, y, pairs, sc=DEFAULT):
    """The checker's result of every pair (q, left, right, band_lo, band_hi): a list of dicts."""
    return [br.trace(xs[q], y[left:right], lo, hi, **sc) for q, left, right, lo, hi in pairs]


def band_tags(path):
    return sorted(t for t in path if t.startswith("affine_band["))


def call(ctx, pairs, sc=DEFAULT, trace=False, off=0):
    q, left, right, lo, hi = ([p[k] for p in pairs] for k in range(5))
    ctx.set_option("no_affine_band", off)
    try:
        got = (ctx.affine_pairs_trace if trace else ctx.affine_pairs_run)(q, left, right, band_lo=lo, band_hi=hi, **sc)
        return got, ctx.last_path()
    finally:
        ctx.set_option("no_affine_band", 0)


def same(got, exp, fields):
    for f in fields:
        a, b = [v for v in got[f]], [e[f] for e in exp]
        assert len(a) == len(b) and all(x == z for x, z in zip(a, b)), (f, [(k, x, z) for k, (x, z) in enumerate(zip(a, b)) if x != z][:5])


def check(ctx, xs, y, pairs, sc=DEFAULT, exp=None, upload=True, tags=None):
    """Run and trace, default dispatch and no_affine_band: all equal the checker; the emitted cells lie in the band; the paths name the
    kernels.  tags: the affine_band[..] tags the default dispatch must show (None: those of the pairs' effective widths up to WMAX)."""
    if upload:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
    exp = expected(xs, y, pairs, sc) if exp is None else exp
    kinds = []                                                        # per pair: "zero", "full", R of the band kernel, or "exact"
    for k, (q, left, right, lo, hi) in enumerate(pairs):
        m, n = len(xs[q]), right - left
        lo_e, hi_e = br.effective_band(m, n, lo, hi)
        if m < 1 or n < 1 or lo_e > hi_e:
            kinds.append("zero")
        elif lo_e == 1 - m and hi_e == n - 1:
            kinds.append("full")
        else:
            W = hi_e - lo_e + 1
            kinds.append(instance_of(W) if W <= WMAX and m <= 512 else "exact")
    want = sorted("affine_band[R=%d]" % r for r in set(k for k in kinds if isinstance(k, int))) if tags is None else sorted(tags)
    for trace in (False, True):
        for off in (0, 1):
            got, path = call(ctx, pairs, sc, trace, off)
            same(got, exp, TRACE_FIELDS if trace else FIELDS)
            if off == 0:
                assert band_tags(path) == want, (path, want)
                assert ("affine_exact_band" in path) == ("exact" in kinds), path
            else:
                assert not band_tags(path), path
                assert ("affine_exact_band" in path) == any(k == "exact" or isinstance(k, int) for k in kinds), path
            assert ("affine_exact" in path or any(t.startswith("affine_pair[") for t in path)) == ("full" in kinds), path
            if trace:
                for k, (q, left, right, lo, hi) in enumerate(pairs):
                    cells = br.cells_of(got["cons_x"][k], got["cons_y"][k], int(got["end_x"][k]), int(got["end_y"][k]))
                    assert all(lo <= j - i <= hi and i >= 1 and j >= 1 for i, j in cells), (k, pairs[k])
                    assert br.rescore(got["cons_x"][k], got["cons_y"][k], **sc) == got["score"][k], k
    return exp


def dna(pgs, seed, n):
    return pgs.synth.dna(seed, n).tobytes()


def read_of(pgs, y, seed, at, m):
    """m letters of y from `at` on with three substitutions, and from 40 letters on one letter dropped and one inserted 8 further."""
    x = np.frombuffer(y[at:at + m], dtype=np.uint8).copy()
    r = pgs.synth.splitmix64(seed, 8)
    if m >= 12:
        for k in range(3):
            x[int(r[k] % np.uint64(m))] = b"ACGT"[int(r[3 + k] % np.uint64(4))]
    if m >= 40:
        cut = 5 + int(r[6] % np.uint64(m - 20))
        x = np.concatenate([x[:cut], x[cut + 1:cut + 9], np.frombuffer(b"T", dtype=np.uint8), x[cut + 9:]])
    assert len(x) == m
    return x.tobytes()


# ---- every compiled instance at the edges of its widths, rows 1, 2, 512, one column ------------------------------------------------------
def test_instances_cover_256_diagonals():
    assert list(BAND_R) == sorted(set(BAND_R)) and WMAX >= 256 and 16 * BAND_R[0] <= 32 and BAND_R[-1] <= 32


@pytest.mark.parametrize("R", BAND_R)
def test_every_instance(ctx, pgs, R):
    y = dna(pgs, 9100 + R, 1800)
    wmin = 1 if R == BAND_R[0] else 16 * BAND_R[BAND_R.index(R) - 1] + 1
    lens = [1, 2, 150, 512]
    at = [400, 420, 450, 500]
    flank = 300
    xs = [read_of(pgs, y, 9200 + 10 * R + k, at[k], m) for k, m in enumerate(lens)]
    pairs = []
    for W in sorted(set((16 * R, 16 * R - 1, wmin))):
        if W < 1:
            continue
        for k, m in enumerate(lens):
            lo = flank - W // 2                                         # the read's own diagonal is `flank`
            pairs.append((k, at[k] - flank, at[k] + m + flank, lo, lo + W - 1))
    pairs.append((2, at[2] + 70, at[2] + 71, -70 - 16 * R // 2, -70 - 16 * R // 2 + 16 * R - 1))   # one column, met by row 71 on diagonal -70
    for k in range(len(pairs)):
        lo_e, hi_e = effective(xs, pairs, k)
        assert instance_of(hi_e - lo_e + 1) == R or k == len(pairs) - 1, (k, lo_e, hi_e)
    exp = check(ctx, xs, y, pairs, tags=None)
    by = {(p[0], p[4] - p[3] + 1): e for p, e in zip(pairs[:-1], exp)}
    if R >= 2:
        assert by[(3, 16 * R)]["score"] > 3 * 512 * 0.8 and by[(2, 16 * R)]["score"] > 3 * 150 * 0.8     # the planted reads, with their gaps
    assert exp[-1]["score"] == 3 and exp[-1]["end_y"] == 1
    # what the run call reports of the kernel
    sub = [p for p in pairs[:-1] if p[4] - p[3] + 1 == 16 * R]
    got, path = call(ctx, sub)
    assert band_tags(path) == ["affine_band[R=%d]" % R], path
    ki = ctx.last_kernel()
    assert ki["name"] == "sw_affine_band_kernel<R=%d>" % R and ki["dtype"] == "f32" and ki["rows_per_lane"] == R, ki
    assert ki["cells"] == sum(len(xs[p[0]]) * 16 * R for p in sub) and ki["valu_ops_per_cell"] > 12
    t = ctx.last_timings()
    assert t["score_us"] > 0 and t["score_launches"] == 1 and t["cells"] == ki["cells"]


def test_width_one_allows_no_gap(ctx, pgs):
    y = dna(pgs, 9301, 600)
    x = read_of(pgs, y, 9302, 200, 150)                                # one letter dropped, one inserted: two gaps off the diagonal
    pairs = [(0, 150, 450, 50, 50), (0, 150, 450, 49, 49), (0, 150, 450, 51, 51), (0, 150, 450, 49, 51)]
    exp = check(ctx, [x], y, pairs)
    assert all("-" not in e["cons_x"] + e["cons_y"] for e in exp[:3]) and "-" in exp[3]["cons_x"] + exp[3]["cons_y"]
    assert exp[3]["score"] > max(e["score"] for e in exp[:3]) > 0


# ---- a band that binds ----------------------------------------------------------------------------------------------------------------
def binding_case(pgs, seed, g=20, la=60):
    a, b, ins = dna(pgs, seed, la), dna(pgs, seed + 1, la), dna(pgs, seed + 2, g)
    left, right = dna(pgs, seed + 3, 40), dna(pgs, seed + 4, 40)
    return a, b, ins, left, right


def test_a_band_that_binds_and_its_mirror(ctx, pgs):
    a, b, ins, fl, fr = binding_case(pgs, 9401)
    # 0: the insert in y (a gap of 20 columns), 1: the insert in x (a gap of 20 rows); w = 5 around the diagonal of A
    xs = [a + b, a + ins + b]
    y = fl + a + ins + b + fr + fl + a + b + fr
    h = len(fl + a + ins + b + fr)
    w0, w1 = (0, h), (h, len(y))
    pairs = [(0, *w0, 40 - 5, 40 + 5), (1, *w1, 40 - 5, 40 + 5)]
    for q, left, right, lo, hi in pairs:
        full = affine_ref.locate(xs[q], y[left:right])[0]
        assert full == 3 * 120 - (5 + 19)                               # the checkers alone: unbanded, the gap is bridged
    exp = check(ctx, xs, y, pairs)
    assert [e["score"] for e in exp] == [180.0, 180.0]                  # banded: the better of A and B alone
    # the device's own two numbers, side by side
    got = ctx.affine_pairs_run([0, 1], [w0[0], w1[0]], [w0[1], w1[1]], **DEFAULT)
    assert got["score"].tolist() == [336.0, 336.0]
    got = ctx.affine_pairs_run([0, 1], [w0[0], w1[0]], [w0[1], w1[1]], band_lo=35, band_hi=45, **DEFAULT)
    assert got["score"].tolist() == [180.0, 180.0]
    # a band that holds both diagonals bridges the gap again
    exp = check(ctx, xs, y, [(0, *w0, 35, 65), (1, *w1, 15, 45)], upload=False)
    assert [e["score"] for e in exp] == [336.0, 336.0]


# ---- E across lanes (a row gap longer than 2 R columns), F across lanes (a column gap of more than 2 R rows), edge-running paths -------------
@pytest.mark.parametrize("R", BAND_R)
def test_gaps_across_lanes_and_along_the_edges(ctx, pgs, R):
    g = 2 * R + 3
    la = 40 + 2 * g                                                     # the flanks outscore the gap: 3 la > 5 + (g - 1)
    a, b, ins, fl, fr = binding_case(pgs, 9500 + 10 * R, g, la)
    xs = [a + b, a + ins + b]
    y = fl + a + ins + b + fr + fl + a + b + fr
    h, h2 = len(fl + a + ins + b + fr), len(y)
    W = 16 * R
    c = 40
    pairs = [
        (0, 0, h, c - 2, c - 2 + W - 1),          # E: the gap of g columns crosses at least two lane boundaries in one step
        (0, 0, h, c + g - W + 1, c + g),          # ... and then runs along hi_e exactly
        (0, 0, h, c, c + g),                      # both edges at once
        (0, 0, h, c, c + g - 1),                  # one diagonal short: the band binds
        (1, h, h2, c - g - 2, c - g - 2 + W - 1),   # F: the gap of g rows runs down across diagonals and lanes
        (1, h, h2, c - g, c - g + W - 1),      # ... and then along lo_e exactly
        (1, h, h2, c - g, c),
        (1, h, h2, c - g + 1, c),              # one diagonal short
    ]
    exp = check(ctx, xs, y, pairs)
    whole = 3.0 * 2 * la - (5 + g - 1)
    got = [e["score"] for e in exp]
    assert [got[k] for k in (0, 1, 2, 4, 5, 6)] == [whole] * 6
    assert 3.0 * la <= got[3] < whole and 3.0 * la <= got[7] < whole    # one diagonal short: about one flank (plus what a shorter gap buys)
    assert "%dD" % g in exp[1]["cigar"] and "%dI" % g in exp[5]["cigar"]


# ---- band edges and clipping ---------------------------------------------------------------------------------------------------------------
def test_band_edges_and_clipping(ctx, pgs):
    y = dna(pgs, 9601, 900)
    xs = [read_of(pgs, y, 9602, 300, 150), read_of(pgs, y, 9603, 310, 60)]
    m, left, right = 150, 250, 520                                      # n = 270, the read's diagonal is 50
    n = right - left
    pairs = [
        (0, left, right, -10 ** 6, 60),           # lo < 1 - m, hi inside
        (0, left, right, 40, 10 ** 6),            # hi > n - 1, lo inside
        (0, left, right, 1 - m, n - 1),           # exactly the matrix: the unbanded pair
        (0, left, right, -10 ** 12, 10 ** 12),    # both outside: the unbanded pair
        (0, left, right, n, n + 50),              # misses the matrix on the right
        (0, left, right, -m - 50, -m),            # ... and on the left
        (0, left, right, n - 1, n - 1),           # one corner cell: (1, n)
        (0, left, right, 1 - m, 1 - m),           # the other corner: (m, 1)
        (0, left, right, -(2 ** 62), 1 - m),      # clipped to that corner
        (1, 300, 400, 5, 15),
    ]
    exp = check(ctx, xs, y, pairs)
    assert exp[0]["score"] == exp[1]["score"] == exp[2]["score"] == exp[3]["score"] > 3 * 150 * 0.8
    assert exp[4]["score"] == exp[5]["score"] == 0
    x0, ys = xs[0], y[left:right]
    assert exp[6]["score"] == (3 if x0[0] == ys[-1] else 0) and exp[7]["score"] == (3 if x0[-1] == ys[0] else 0)
    # the covering bands: the unbanded path and its bytes
    q, lf, rt = [0, 0], [left, left], [right, right]
    plain = ctx.affine_pairs_trace(q, lf, rt, **DEFAULT)
    plain_path = ctx.last_path()
    got, path = call(ctx, pairs[2:4], trace=True)
    assert path == plain_path and any(t.startswith("affine_pair[") for t in path) and not band_tags(path), (path, plain_path)
    for f in TRACE_FIELDS:
        assert list(got[f]) == list(plain[f]), f
    # only misses: zeros, and no kernel at all
    got, path = call(ctx, pairs[4:6])
    assert not got["score"].any() and not got["end_x"].any() and not got["end_y"].any() and not path


# ---- ties -------------------------------------------------------------------------------------------------------------------------------
def test_ties(ctx, pgs):
    u, v = b"ACCAG", b"GACAC"
    x3 = u + v + b"N" * 22                                              # rows 6..10 match in columns 1..5 (diagonal -5), rows 1..5 in
    y3 = v + b"T" * 8 + u                                               # columns 14..18 (diagonal 13): the later row, the smaller column
    homo = b"A" * 40
    y = y3 + b"C" + b"A" * 100 + b"C"
    a = len(y3) + 1
    xs = [x3, homo]
    pairs = [(0, 0, 18, -5, 13), (0, 0, 18, -6, 26), (0, 0, 18, -4, 13),
             (1, a, a + 100, 0, 10), (1, a, a + 100, -5, 40), (1, a, a + 20, -25, 10), (1, a, a + 20, -20, -3)]
    H = br.matrices(x3, y3, -5, 13, **DEFAULT)[0]
    assert H.max() == 15 and H[10, 5] == 15 and H[5, 18] == 15           # the checker alone: the tie exists, in different lanes and rows
    exp = check(ctx, xs, y, pairs)
    ends = [(e["score"], e["end_x"], e["end_y"]) for e in exp]
    assert ends[0] == (15, 10, 5) and ends[1] == (15, 10, 5)            # the smaller column wins, though its row comes later
    # the same tie inside ONE lane, which only the lane's own compare across steps settles: diagonals -5 and 6 are registers 0 and 11
    # of lane 0 on the two widest instances; row 5 reaches 15 in column 11 first, row 10 reaches it later in column 5
    y4 = v + b"T" + u + b"T" * 260
    H = br.matrices(x3, y4, -5, 250, **DEFAULT)[0]
    assert H.max() == 15 and H[5, 11] == 15 and H[10, 5] == 15
    wide = [(0, 0, len(y4), -5, -5 + 16 * r - 1) for r in BAND_R[-2:]]
    assert all(instance_of(effective(xs, wide, k)[1] + 5 + 1) == r and r >= 12 for k, r in enumerate(BAND_R[-2:]))
    exp4 = check(ctx, xs, y4, wide)
    assert [(e["score"], e["end_x"], e["end_y"]) for e in exp4] == [(15, 10, 5)] * 2
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    assert ends[2] == (15, 5, 18)                                       # with diagonal -5 out of the band the other one is left
    assert ends[3] == (120, 40, 40) and ends[4] == (120, 40, 40)        # columns 40..50 tie in row 40: the smallest column
    assert ends[5] == (60, 20, 20)                                      # rows 20..40 tie in column 20: the smallest row
    assert ends[6] == (60, 23, 20)                                      # diagonals -20 .. -3: column 20 from row 23 on


# ---- one mixed call ---------------------------------------------------------------------------------------------------------------------------
def test_one_mixed_call_keeps_the_order(ctx, pgs):
    y = dna(pgs, 9701, 3000)
    lens = [150, 37, 512, 1, 513, 90, 0]
    at = [400, 700, 1000, 1700, 1800, 2500, 0]
    xs = [read_of(pgs, y, 9710 + k, at[k], m) if m else b"" for k, m in enumerate(lens)]
    pairs = []
    widths = sorted(set([1, 17] + [16 * r - (r % 2) for r in BAND_R] + [WMAX + 1, WMAX + 144]))   # every instance, and two widths beyond the last
    for k, W in enumerate(widths):
        q = (0, 1, 2, 5)[k % 4]
        fl = 100 + 37 * (k % 3) + (200 if W > 256 else 0)
        pairs.append((q, at[q] - fl, at[q] + lens[q] + fl, fl - W // 2, fl - W // 2 + W - 1))
        if k % 3 == 0:
            pairs.append((q, at[q] - fl, at[q] + lens[q] + fl, -10 ** 9, 10 ** 9))      # full cover
        if k % 4 == 1:
            pairs.append((q, at[q] - fl, at[q] + lens[q] + fl, 5000, 6000))             # zeros
    pairs.append((4, at[4] - 50, at[4] + 513 + 50, 40, 60))                # 513 rows: the exact kernel under a band
    pairs.append((6, 0, 100, -5, 5))                                       # an empty query
    pairs.append((3, at[3] - 5, at[3] + 6, 5, 5))
    pairs.append((0, at[0] - 100, at[0] + 250, 90, 99))                    # query 0 again, a band beside its diagonal
    pairs.append((0, at[0] - 100, at[0] + 250, 95, 110))
    exp = check(ctx, xs, y, pairs)
    assert len(set(e["score"] for e in exp)) > 8 and exp[-1]["score"] > exp[-2]["score"]
    _, path = call(ctx, pairs)
    assert band_tags(path) == sorted("affine_band[R=%d]" % r for r in BAND_R) and "affine_exact_band" in path
    assert any(t.startswith("affine_pair[") for t in path), path


def test_one_call_takes_all_five_routes(ctx, pgs):
    """Zeros, the pair kernel, the band kernel, the exact kernel and the exact kernel under a band in one list, interleaved; the pair
    stage's table is built for 150 rows and the band stage's for 37."""
    y = dna(pgs, 9751, 3000)
    lens = [150, 37, 513, 0]
    at = [400, 900, 1500, 0]
    xs = [read_of(pgs, y, 9760 + k, at[k], m) if m else b"" for k, m in enumerate(lens)]
    cover = (-10 ** 9, 10 ** 9)
    w513 = (at[2] - 50, at[2] + 513 + 50)                                 # the read's own diagonal is 50
    first = (0, at[0] - 100, at[0] + 250, *cover)                         # 150 rows, full cover: the pair kernel, R = 10
    pairs = [
        first,
        (2, *w513, 40, 60),                                               # 513 rows under a band: the exact kernel's BAND instance
        (1, at[1] - 60, at[1] + 37 + 60, 52, 68),                         # 37 rows, 17 diagonals around its own (60): the band kernel
        (0, at[0] - 100, at[0] + 250, 5000, 6000),                        # the band misses the matrix
        (2, *w513, *cover),                                               # 513 rows, full cover: the exact kernel
        (3, 0, 100, -5, 5),                                               # an empty query
        first,
    ]
    assert instance_of(17) == BAND_R[1] and effective(xs, pairs, 2) == (52, 68)
    exp = expected(xs, y, pairs)
    # the checkers alone: the reads are found, the covering bands are the unbanded pairs, and the band of pair 1 binds (the read's
    # dropped letter moves it to diagonal 51 and its inserted one back: both inside; the band that lacks diagonal 50 loses the head)
    assert exp[0]["score"] > 3 * 150 * 0.8 and exp[2]["score"] > 3 * 37 * 0.7 and exp[4]["score"] > 3 * 513 * 0.8
    assert exp[0]["score"] == affine_ref.locate(xs[0], y[first[1]:first[2]])[0] and exp[4]["score"] == affine_ref.locate(xs[2], y[w513[0]:w513[1]])[0]
    assert exp[1]["score"] == exp[4]["score"] and "D" in exp[1]["cigar"] and "I" in exp[1]["cigar"]
    assert 0 < br.trace(xs[2], y[w513[0]:w513[1]], 51, 60, **DEFAULT)["score"] < exp[1]["score"]
    assert exp[3]["score"] == exp[5]["score"] == 0 and exp[0] == exp[6]
    check(ctx, xs, y, pairs, exp=exp)
    for off in (0, 1):
        got, path = call(ctx, pairs, trace=True, off=off)
        for f in TRACE_FIELDS:
            assert got[f][0] == got[f][-1], (off, f)
        if off == 0:
            assert [t for t in path if t.startswith("affine_pair[")] == ["affine_pair[R=10]"], path
            assert band_tags(path) == ["affine_band[R=%d]" % BAND_R[1]], path
            assert "affine_exact" in path and "affine_exact_band" in path, path


# ---- tables -------------------------------------------------------------------------------------------------------------------------------
def test_a_25_by_21_table_and_a_table_beyond_32_kib(ctx, pgs):
    lut = pgs.synth.make_lut(4242, 1.0)
    sc = dict(match=3.0, mismatch=-3.0, gap_open=11.0, gap_extend=1.0, lut=lut)
    y = si.letters(pgs, 9801, 900, si.AA20).copy()
    q = [si.letters(pgs, 9802 + k, 120, si.AA20).copy() for k in range(2)]
    ins = si.letters(pgs, 9810, 4, si.AA20)
    y[200:324] = np.concatenate([q[0][:50], ins, q[0][50:]])            # a gap of 4 columns
    y[500:617] = np.concatenate([q[1][:70], q[1][73:]])                 # a gap of 3 rows
    xs, yb = [v.tobytes() for v in q], y.tobytes()
    pairs = [(0, 150, 400, 40, 60), (0, 150, 400, 50, 53), (1, 450, 700, 40, 60), (1, 450, 700, 48, 50), (1, 450, 700, 20, 280)]
    exp = check(ctx, xs, yb, pairs, sc=sc)
    assert exp[0]["score"] > exp[1]["score"] > 0 and exp[2]["score"] > exp[3]["score"] > 0
    assert "4D" in exp[0]["cigar"] and "3I" in exp[2]["cigar"]
    # every byte its own class against a reference of 40 letters: 41 x 257 entries, beyond 32 KiB — every banded pair on the exact kernel
    rng = np.random.default_rng(9820)
    big = rng.integers(-4, 0, (256, 256)).astype(np.float32)           # (random rows: pairwise different on the reference's letters)
    big[np.arange(256), np.arange(256)] = 5.0
    alpha = np.arange(40, 80, dtype=np.uint8)
    y2 = alpha[rng.integers(0, 40, 600)]
    x2 = np.concatenate([y2[200:260], y2[263:320]])
    ctx.set_reference(y2.tobytes())
    ctx.batch_upload([x2.tobytes()])
    sc2 = dict(match=3.0, mismatch=-3.0, gap_open=6.0, gap_extend=1.0, lut=big)
    pairs2 = [(0, 150, 400, 45, 60), (0, 150, 400, 50, 52)]
    exp2 = expected([x2.tobytes()], y2.tobytes(), pairs2, sc2)
    for trace in (False, True):
        got, path = call(ctx, pairs2, sc2, trace)
        same(got, exp2, TRACE_FIELDS if trace else FIELDS)
        assert "affine_exact_band" in path and not band_tags(path), path
    assert exp2[0]["score"] == 5 * 117 - (6 + 2) and exp2[1]["score"] == 5 * 60


# ---- the float32 bound from both sides ---------------------------------------------------------------------------------------------------------
def test_bound_from_both_sides(ctx, pgs):
    y = bytearray(dna(pgs, 9901, 1200))
    x = dna(pgs, 9902, 511)
    y[300:811] = x
    y = bytes(y)
    ctx.set_reference(y)
    ctx.batch_upload([x])
    pairs = [(0, 250, 900, 40, 60)]
    for sc, kernel in ((dict(match=511.0, mismatch=-300.0, gap_open=700.0, gap_extend=3.0), True),
                       (dict(match=512.0, mismatch=-300.0, gap_open=700.0, gap_extend=3.0), False),
                       (dict(match=3.0, mismatch=-3.0, gap_open=float(2 ** 18), gap_extend=1.0), False),
                       (dict(match=3.0, mismatch=-3.0, gap_open=float(2 ** 18 - 1), gap_extend=float(2 ** 18 - 1)), True)):
        got, path = call(ctx, pairs, sc)
        assert (len(band_tags(path)) > 0) == kernel and ("affine_exact_band" in path) == (not kernel), (sc, path)
        same(got, expected([x], y, pairs, sc), FIELDS)
        assert got["score"][0] == sc["match"] * 511


# ---- end-to-end mode with bands, argument errors ----------------------------------------------------------------------------------------------
def test_end_to_end_with_bands_is_refused_and_errors_leave_the_context_usable(ctx, pgs):
    y = dna(pgs, 9951, 2000)
    xs = [read_of(pgs, y, 9960 + k, 400 * k + 100, 150) for k in range(4)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    pairs = [(k, 400 * k + 50, 400 * k + 320, 40, 60) for k in range(4)]
    exp = expected(xs, y, pairs)
    q, left, right, lo, hi = ([p[k] for p in pairs] for k in range(5))

    def still_fine():
        got, path = call(ctx, pairs)
        same(got, exp, FIELDS)
        assert band_tags(path)

    for fn in (ctx.affine_pairs_run, ctx.affine_pairs_trace):
        with pytest.raises(pgs.MI355Error) as e:
            fn(q, left, right, mode="end_to_end", band_lo=lo, band_hi=hi, **DEFAULT)
        assert e.value.code == ENOTSUP and "end-to-end" in str(e.value)
        still_fine()
        with pytest.raises(pgs.MI355Error) as e:
            fn(q, left, right, band_lo=[40, 40, 40, 40], band_hi=[60, 39, 60, 60], **DEFAULT)
        assert e.value.code == EINVAL
        with pytest.raises(pgs.MI355Error) as e:                        # an argument error of the _mode call comes first
            fn(q, left, [r + 5000 for r in right], mode="end_to_end", band_lo=lo, band_hi=hi, **DEFAULT)
        assert e.value.code == EINVAL
    still_fine()
    L = ctx._L
    p, keep = pgs.capi.make_affine_params()
    n = 4
    i64, i32 = C.c_int64 * n, C.c_int32 * n
    sc, ex, ey = (C.c_float * n)(7, 7, 7, 7), i64(7, 7, 7, 7), i64(7, 7, 7, 7)
    args = (C.c_size_t(n), i32(*q), i64(*left), i64(*right))
    for blo, bhi in ((i64(*lo), None), (None, i64(*hi))):               # exactly one of the two NULL
        assert L.mi355_sw_affine_pairs_run_band(ctx._ctx, C.c_int(0), *args, blo, bhi, C.byref(p), sc, ex, ey) == EINVAL
    assert list(sc) == [7] * 4 and list(ex) == [7] * 4 and list(ey) == [7] * 4
    # both NULL: the _mode call itself, same path and bytes
    assert L.mi355_sw_affine_pairs_run_band(ctx._ctx, C.c_int(0), *args, None, None, C.byref(p), sc, ex, ey) == 0
    path = ctx.last_path()
    plain = ctx.affine_pairs_run(q, left, right, **DEFAULT)
    assert path == ctx.last_path() and list(sc) == plain["score"].tolist() and list(ey) == plain["end_y"].tolist()
    still_fine()


def test_a_banded_pair_beyond_both_kernels_is_refused(ctx, pgs):
    y = dna(pgs, 9971, 120_000)
    xs = [dna(pgs, 9972, 600), read_of(pgs, y, 9973, 100, 100)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    for fn in (ctx.affine_pairs_run, ctx.affine_pairs_trace):
        with pytest.raises(pgs.MI355Error) as e:                        # 600 rows: not the band kernel's; 600 x 120 000 cells: not the exact kernel's
            fn([1, 0], [0, 0], [300, 120_000], band_lo=[-5, 0], band_hi=[5, 50], **DEFAULT)
        assert e.value.code == ENOTSUP and "2^26" in str(e.value) and "banded pair 1" in str(e.value)
    exp = check(ctx, xs, y, [(1, 50, 300, 40, 60), (0, 0, 700, -20, 20)], upload=False)   # the context goes on working
    assert exp[0]["score"] > 200


def test_through_the_python_aligner(ctx, pgs):
    y = dna(pgs, 9981, 800)
    xs = [read_of(pgs, y, 9982, 200, 150), read_of(pgs, y, 9983, 400, 80)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    pairs = [(0, 150, 420, 40, 60), (1, 350, 530, 45, 55)]
    exp = expected(xs, y, pairs)
    q, left, right = ([p[k] for p in pairs] for k in range(3))
    got = pgs.AffineSWAligner.align_pairs(q, left, right, context=ctx, traceback=True, band=([40, 45], [60, 55]))
    same(got, exp, TRACE_FIELDS)
    got = pgs.AffineSWAligner.align_pairs(q, left, right, context=ctx, band=(45, 55))
    same(got, expected(xs, y, [(0, 150, 420, 45, 55), (1, 350, 530, 45, 55)]), FIELDS)
