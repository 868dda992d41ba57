"""Lists of (query, window) pairs under affine gaps on the device (mi355_sw_affine_pairs_run / _trace) against tests/affine_ref.py and
tests/affine_trace_ref.py applied to the slice y[left:right].  Every case runs twice, on the default dispatch (sw_affine_pair_kernel)
and under option no_affine_pairs (the exact kernel): both must equal the checker, hence each other, field for field, and the path must
show which kernel ran.  Planted features are first shown to matter by the checker alone.  Expected values are computed once per
module."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import affine_ref, affine_trace_ref, score_instances as si

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_KERNEL_H = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "sw_affine_pair_kernel.h")
FIELDS = ("score", "end_x", "end_y")
TRACE_FIELDS = FIELDS + ("begin_x", "begin_y", "pos", "cons_x", "cons_y", "cigar")


def compiled_R():
    with open(PAIR_KERNEL_H) as f:
        m = re.search(r"constexpr\s+int\s+kPairR\[\]\s*=\s*\{([^}]*)\}", f.read())
    return tuple(int(v) for v in m.group(1).split(","))


PAIR_R = compiled_R()


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


class Scoring:
    def __init__(self, name, match=3, mismatch=-3, gap_open=5, gap_extend=1, lut=None, alpha=b"ACGT"):
        self.name, self.match, self.mismatch, self.open, self.ext, self.lut, self.alpha = name, match, mismatch, gap_open, gap_extend, lut, alpha

    def kw(self):
        return dict(match=float(self.match), mismatch=float(self.mismatch), gap_open=float(self.open), gap_extend=float(self.ext), lut=self.lut)

    def ref_args(self, gap=None):
        go, ge = (self.open, self.ext) if gap is None else (gap, gap)
        return (self.match, self.mismatch, go, ge, self.lut)


DEFAULT = Scoring("3/-3/5/1")


def expected(xs, y, pairs, sc):
    """dict of arrays score, end_x, end_y: the checker on every pair's slice, pairs of one window in one sweep."""
    n = len(pairs)
    out = dict(score=np.zeros(n, dtype=np.float32), end_x=np.zeros(n, dtype=np.int64), end_y=np.zeros(n, dtype=np.int64))
    by_window = {}
    for k, (q, lo, hi) in enumerate(pairs):
        by_window.setdefault((lo, hi), []).append(k)
    for (lo, hi), ks in by_window.items():
        s, i, j = affine_ref.locate_batch([xs[pairs[k][0]] for k in ks], y[lo:hi], *sc.ref_args())
        for t, k in enumerate(ks):
            out["score"][k], out["end_x"][k], out["end_y"][k] = s[t], i[t], j[t]
    return out


def pair_tags(path):
    return [t for t in path if t.startswith("affine_pair[")]


def run_both(ctx, pairs, sc, trace=False):
    """{0: (result, path) on the default dispatch, 1: under no_affine_pairs} of the resident batch and reference."""
    q, lo, hi = ([p[k] for p in pairs] for k in range(3))
    out = {}
    for off in (0, 1):
        ctx.set_option("no_affine_pairs", off)
        try:
            got = (ctx.affine_pairs_trace if trace else ctx.affine_pairs_run)(q, lo, hi, **sc.kw())
            out[off] = (got, ctx.last_path())
        finally:
            ctx.set_option("no_affine_pairs", 0)
    return out


def same(got, exp, fields=FIELDS):
    for f in fields:
        a, b = got[f], exp[f]
        ok = np.array_equal(a, b) if isinstance(a, np.ndarray) else list(a) == list(b)
        assert ok, (f, [(k, x, z) for k, (x, z) in enumerate(zip(a, b)) if x != z][:5])


def check_both(ctx, xs, y, pairs, sc=DEFAULT, exp=None, upload=True):
    """Both dispatches equal the checker and each other; the paths name the kernel that ran.  Returns the expectation."""
    if upload:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
    exp = expected(xs, y, pairs, sc) if exp is None else exp
    out = run_both(ctx, pairs, sc)
    for off in (0, 1):
        same(out[off][0], exp)
    same(out[0][0], out[1][0])
    work = any(len(xs[q]) and hi > lo for q, lo, hi in pairs)
    p0, p1 = out[0][1], out[1][1]
    assert (len(pair_tags(p0)) > 0) == work and "affine_exact" not in p0, p0
    assert ("affine_exact" in p1) == work and not pair_tags(p1), p1
    return exp


def read_of(pgs, y, seed, at, m):
    """m letters of y from `at` on with a few substitutions, one letter dropped and one inserted where there is room."""
    x = np.frombuffer(y[at:at + m], dtype=np.uint8).copy()
    r = pgs.synth.splitmix64(seed, 8)
    if m >= 12:
        for k in range(3):
            x[int(r[k] % np.uint64(m))] = b"ACGT"[int(r[3 + k] % np.uint64(4))]
    if m >= 40:
        cut = 5 + int(r[6] % np.uint64(m - 20))
        x = np.concatenate([x[:cut], x[cut + 1:cut + 9], np.frombuffer(b"T", dtype=np.uint8), x[cut + 9:]])
    assert x.dtype == np.uint8 and len(x) == m
    return x.tobytes()


# ---- every compiled instance ------------------------------------------------------------------------------------------------------
def test_instances_cover_512_rows_and_a_150_row_read():
    assert 1 <= len(PAIR_R) <= 8 and list(PAIR_R) == sorted(set(PAIR_R)) and PAIR_R[-1] == 32
    assert min(16 * r for r in PAIR_R if 16 * r >= 150) - 150 <= 10


@pytest.mark.parametrize("R", PAIR_R)
def test_every_instance(ctx, pgs, R):
    y = pgs.synth.dna(7100 + R, 1400).tobytes()
    lens = [1, R, R + 1, 16 * R - 1, 16 * R]
    xs = [read_of(pgs, y, 7200 + 10 * R + k, 300 + 11 * k, m) for k, m in enumerate(lens)]
    pairs = [(k, max(0, 300 + 11 * k - 30), 300 + 11 * k + m + 30) for k, m in enumerate(lens)]
    exp = check_both(ctx, xs, y, pairs)
    assert exp["score"][4] > 3 * 16 * R * 0.7                         # the planted read is found, not background
    ctx.set_option("no_affine_pairs", 0)
    ctx.affine_pairs_run([3, 4], [pairs[3][1], pairs[4][1]], [pairs[3][2], pairs[4][2]], **DEFAULT.kw())
    assert "affine_pair[R=%d]" % R in ctx.last_path(), ctx.last_path()
    ki = ctx.last_kernel()
    assert ki["name"] == "sw_affine_pair_kernel<R=%d>" % R and ki["dtype"] == "f32" and ki["rows_per_lane"] == R, ki
    assert ki["cells"] == sum(len(xs[k]) * (pairs[k][2] - pairs[k][1]) for k in (3, 4)) and ki["valu_ops_per_cell"] > 9
    t = ctx.last_timings()
    assert t["score_us"] > 0 and t["score_launches"] == 1 and t["cells"] == ki["cells"]


# ---- window lengths: skew, segment refill, history ---------------------------------------------------------------------------------
WINDOWS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 1000]


def test_window_lengths(ctx, pgs):
    y = pgs.synth.dna(7301, 1500).tobytes()
    xs = [read_of(pgs, y, 7302, 105, 150), b"", read_of(pgs, y, 7303, 160, 37)]
    pairs = [(q, 100, 100 + w) for w in WINDOWS for q in (0, 1, 2)]
    exp = check_both(ctx, xs, y, pairs)
    assert all(exp["score"][k] == 0 for k, (q, lo, hi) in enumerate(pairs) if q == 1 or hi == lo)
    assert exp["score"][pairs.index((0, 100, 300))] > 300              # the read lies in the 200-column window
    # nothing but empty problems: zeros, and no kernel at all
    for off in (0, 1):
        ctx.set_option("no_affine_pairs", off)
        got = ctx.affine_pairs_run([1, 0], [5, 7], [50, 7])
        ctx.set_option("no_affine_pairs", 0)
        assert not got["score"].any() and not got["end_x"].any() and not got["end_y"].any() and not ctx.last_path()


# ---- batch sizes: idle slots, a last partial workgroup, short and long streams in one wavefront ------------------------------------
_batch = {}


def batch_case(pgs):
    if not _batch:
        y = pgs.synth.dna(7401, 4000).tobytes()
        wins = [(500, 1500), (812, 832), (2100, 3100), (2590, 2610)]      # 1 000 and 20 columns, interleaved
        at = [900, 815, 2500, 2592]
        xs = [read_of(pgs, y, 7410 + k, at[k % 4] + (k // 4) % 40, 100 + (k * 7) % 61) for k in range(300)]
        pairs = [(k, *wins[k % 4]) for k in range(300)]
        _batch.update(y=y, xs=xs, pairs=pairs, exp=expected(xs, y, pairs, DEFAULT))
    return _batch


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 300])
def test_batch_sizes(ctx, pgs, n):
    b = batch_case(pgs)
    exp = {f: b["exp"][f][:n] for f in FIELDS}
    check_both(ctx, b["xs"], b["y"], b["pairs"][:n], exp=exp)
    assert b["exp"]["score"][0] > 200 and 0 < b["exp"]["score"][1] <= 60


# ---- independence of the pairs -----------------------------------------------------------------------------------------------------
def test_windows_cut_copies_at_both_edges(ctx, pgs):
    y = bytearray(pgs.synth.dna(7501, 3000).tobytes())
    x = pgs.synth.dna(7502, 150).tobytes()
    lo, hi = 1000, 1400
    y[lo - 60:lo + 90] = x                                             # a perfect copy across the left edge ...
    y[hi - 80:hi + 70] = x                                             # ... and one across the right edge
    y = bytes(y)
    whole = affine_ref.locate(x, y)
    exp = check_both(ctx, [x], y, [(0, lo, hi)])
    assert whole[0] == 450 and exp["score"][0] == 3 * 90 and exp["end_y"][0] == 90, (whole, exp)


def test_reference_ends_shared_query_and_overlaps(ctx, pgs):
    y = bytearray(pgs.synth.dna(7601, 2000).tobytes())
    xs = [pgs.synth.dna(7602 + k, m).tobytes() for k, m in enumerate((150, 90, 33))]
    y[:90] = xs[1]                                                     # begins in column 0
    y[2000 - 33:] = xs[2]                                              # ends in the last column
    y[700:850] = xs[0]
    y = bytes(y)
    pairs = [(1, 0, 200), (2, 1800, 2000), (1, 0, 2000 - 1), (2, 0, 2000)]
    pairs += [(0, 500 + 7 * k, 760 + 9 * k) for k in range(40)]          # one query in 40 overlapping windows
    exp = check_both(ctx, xs, y, pairs)
    assert exp["score"][0] == 270 and exp["end_y"][0] == 90 and exp["score"][1] == 99 and exp["end_y"][1] == 200
    assert len(set(exp["score"][4:].tolist())) > 3                     # the windows cut the copy at different columns


# ---- planted gaps -------------------------------------------------------------------------------------------------------------------
_gaps = {}


def gap_case(pgs, sc=DEFAULT):
    """150-row queries (10 rows per lane).  0: 3 window letters inserted in the middle of the copy (a gap of 3 columns, inside one
    lane's rows); 1: rows 11..13, the first of the second lane, have no column (a gap of 3 rows handed across the lane boundary);
    2: 70 window letters inserted, longer than a segment, where the flanks outscore the gap; 3: unrelated."""
    if sc.name not in _gaps:
        al = sc.alpha
        y = si.letters(pgs, 7701, 2400, al).copy()
        q = [si.letters(pgs, 7710 + k, 150, al).copy() for k in range(4)]
        ins = lambda k, cnt: si.letters(pgs, 7750 + k, cnt, al)
        R = min(r for r in PAIR_R if 16 * r >= 150)
        h = 7 * R + R // 2                                              # inside lane 7's rows
        p0 = np.concatenate([q[0][:h], ins(0, 3), q[0][h:]])
        p1 = np.concatenate([q[1][:R], q[1][R + 3:]])
        p2 = np.concatenate([q[2][:h], ins(2, 70), q[2][h:]])
        at = [200, 700, 1200]
        for a, p in zip(at, (p0, p1, p2)):
            y[a:a + len(p)] = p
        pairs = [(0, 150, 420), (1, 640, 900), (2, 1150, 1500), (3, 1150, 1500), (0, 640, 900)]
        xs, y = [v.tobytes() for v in q], y.tobytes()
        exp = expected(xs, y, pairs, sc)
        faults = []
        for k in (0, 1, 2):
            _, lo, hi = pairs[k]
            lin = [affine_ref.locate(xs[k], y[lo:hi], *sc.ref_args(g))[0] for g in (sc.open, sc.ext)]
            if exp["score"][k] in lin:
                faults.append("pair %d: affine %g, linear %s: the gap does not matter" % (k, exp["score"][k], lin))
        _gaps[sc.name] = dict(xs=xs, y=y, pairs=pairs, exp=exp, faults=faults)
    return _gaps[sc.name]


def test_planted_gaps(ctx, pgs):
    g = gap_case(pgs)
    assert not g["faults"], g["faults"]
    assert g["exp"]["score"][2] == 3 * 150 - 5 - 69                   # the 70-column gap is bridged
    check_both(ctx, g["xs"], g["y"], g["pairs"], exp=g["exp"])


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def tie_cases(pgs):
    x = pgs.synth.dna(7801, 150).tobytes()
    y1 = pgs.synth.dna(7802, 30).tobytes() + x + pgs.synth.dna(7803, 41).tobytes() + x + pgs.synth.dna(7804, 30).tobytes()
    homo = [b"A" * 40, b"A" * 100, b"A" * 20]
    # the same value twice in ONE lane's rows: rows 6..10 match in columns 1..5, rows 1..5 in columns 14..18 (a later column, a
    # smaller row); 'N' matches nothing
    u, v = b"ACCAG", b"GACAC"
    x3 = u + v + b"N" * 140
    y3 = v + b"T" * 8 + u
    return x, y1, homo, x3, y3


def test_ties(ctx, pgs):
    x, y1, homo, x3, y3 = tie_cases(pgs)
    H = affine_trace_ref.matrices(x3, y3, 3, -3, 5, 1)[0]
    assert H.max() == 15 and H[10, 5] == 15 and H[5, 18] == 15        # the checker alone: the tie exists
    y = y1 + b"C" + homo[1] + b"C" + y3
    a = len(y1) + 1
    b = a + 100 + 1
    xs = [x, homo[0], x3, homo[0][:30]]
    pairs = [(0, 0, len(y1)), (1, a, a + 100), (1, a, a + 20), (2, b, b + 18), (3, a, a + 100), (3, a + 3, a + 20)]
    exp = check_both(ctx, xs, y, pairs)
    assert (exp["score"][0], exp["end_x"][0], exp["end_y"][0]) == (450, 150, 180)      # two copies: the first column
    assert (exp["score"][1], exp["end_x"][1], exp["end_y"][1]) == (120, 40, 40)        # smallest column ...
    assert (exp["score"][2], exp["end_x"][2], exp["end_y"][2]) == (60, 20, 20)         # ... then smallest row, rows 20..40 of 5 lanes tie
    assert (exp["score"][3], exp["end_x"][3], exp["end_y"][3]) == (15, 10, 5)          # smaller column over smaller row in a lane


# ---- scorings -----------------------------------------------------------------------------------------------------------------------
def _scorings(pgs):
    asym = np.full((256, 256), -4.0, dtype=np.float32)
    for c in b"ACGT":
        asym[c, c] = 5.0
    asym[ord("A"), ord("C")], asym[ord("C"), ord("A")], asym[ord("G"), ord("T")], asym[ord("T"), ord("G")] = -1.0, -6.0, 2.0, -3.0
    return [DEFAULT, Scoring("1/-1/4/2", 1, -1, 4, 2), Scoring("10/-2/12/1", 10, -2, 12, 1), Scoring("3/-3/2/2", 3, -3, 2, 2),
            Scoring("lut/aa20/11/1", gap_open=11, gap_extend=1, lut=pgs.synth.make_lut(4242, 1.0), alpha=si.AA20),
            Scoring("lut/asym/6/1", gap_open=6, gap_extend=1, lut=asym)]


@pytest.mark.parametrize("which", range(6))
def test_scorings(ctx, pgs, oracle, which):
    sc = _scorings(pgs)[which]
    g = gap_case(pgs, sc)
    exp = check_both(ctx, g["xs"], g["y"], g["pairs"], sc=sc, exp=g["exp"])
    assert exp["score"][0] > exp["score"][4] > 0
    if sc.open == sc.ext:                                              # the linear model: the reference's oracle on the slice
        for k, (q, lo, hi) in enumerate(g["pairs"]):
            o = oracle.locate(g["xs"][q], g["y"][lo:hi], 0, match=3.0, mismatch=-3.0, gap=2.0)
            assert (float(o[0]), int(o[1]), int(o[2])) == (float(exp["score"][k]), int(exp["end_x"][k]), int(exp["end_y"][k]))


# ---- the 2^18 bound from both sides --------------------------------------------------------------------------------------------------
def test_bound_from_both_sides(ctx, pgs):
    y = bytearray(pgs.synth.dna(7901, 1200).tobytes())
    xs = [pgs.synth.dna(7902, 511).tobytes(), pgs.synth.dna(7903, 511).tobytes()]
    y[300:811] = xs[0]
    y = bytes(y)
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    pairs = [(0, 250, 900), (1, 0, 600)]
    q, lo, hi = ([p[k] for p in pairs] for k in range(3))
    for sc, kernel in ((Scoring("511", 511, -300, 700, 3), True), (Scoring("512", 512, -300, 700, 3), False),
                       (Scoring("open", 3, -3, 2 ** 18, 1), False), (Scoring("open-1", 3, -3, 2 ** 18 - 1, 1), True)):
        try:
            got = ctx.affine_pairs_run(q, lo, hi, **sc.kw())
        except pgs.MI355Error as e:
            assert e.code == ENOTSUP and not kernel, sc.name
            continue
        path = ctx.last_path()
        assert (len(pair_tags(path)) > 0) == kernel and ("affine_exact" in path) == (not kernel), (sc.name, path)
        exp = expected(xs, y, pairs, sc)
        same(got, exp)
        assert exp["score"][0] == sc.match * 511


# ---- mixed dispatch, and the pair neither kernel takes -------------------------------------------------------------------------------
_mixed = {}


def mixed_case(pgs):
    if not _mixed:
        y = bytearray(pgs.synth.dna(8001, 2500).tobytes())
        xs = [pgs.synth.dna(8002 + k, m).tobytes() for k, m in enumerate((513, 150, 512, 20))]
        y[100:613] = xs[0]
        y[1000:1512] = xs[2][:200] + xs[2][203:] + b"ACG"
        y = bytes(y)
        pairs = [(1, 0, 700), (0, 50, 700), (2, 900, 1600), (0, 900, 1600), (3, 0, 2500), (1, 2000, 2500)]
        _mixed.update(xs=xs, y=y, pairs=pairs, exp=expected(xs, y, pairs, DEFAULT))
    return _mixed


def test_mixed_dispatch_keeps_the_order(ctx, pgs):
    m = mixed_case(pgs)
    ctx.set_reference(m["y"])
    ctx.batch_upload(m["xs"])
    out = run_both(ctx, m["pairs"], DEFAULT)
    for off in (0, 1):
        same(out[off][0], m["exp"])
    assert pair_tags(out[0][1]) and "affine_exact" in out[0][1], out[0][1]
    assert not pair_tags(out[1][1]) and "affine_exact" in out[1][1], out[1][1]
    assert m["exp"]["score"][1] == 3 * 513 and len(set(m["exp"]["score"].tolist())) == 6


def test_a_pair_beyond_both_kernels_is_refused(ctx, pgs):
    y = pgs.synth.dna(8105, 120_000).tobytes()
    xs = [pgs.synth.dna(8106, 600).tobytes(), pgs.synth.dna(8107, 100).tobytes()]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    for call in (ctx.affine_pairs_run, ctx.affine_pairs_trace):
        with pytest.raises(pgs.MI355Error) as e:
            call([1, 0], [0, 0], [300, 120_000])
        assert e.value.code == ENOTSUP and "2^26" in str(e.value)
    exp = check_both(ctx, xs, y, [(1, 0, 300), (1, 100, 700)], upload=False)   # the context goes on working
    assert exp["score"][0] > 0


# ---- traceback ----------------------------------------------------------------------------------------------------------------------
def trace_expected(xs, y, pairs, sc):
    rows = [affine_trace_ref.trace(xs[q], y[lo:hi], *sc.ref_args()) for q, lo, hi in pairs]
    return {f: (np.array([r[f] for r in rows]) if f not in ("cons_x", "cons_y", "cigar") else [r[f] for r in rows]) for f in TRACE_FIELDS}


def check_trace(ctx, pgs, xs, y, pairs, sc=DEFAULT, sample=()):
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    exp = trace_expected(xs, y, pairs, sc)
    out = run_both(ctx, pairs, sc, trace=True)
    for off in (0, 1):
        same(out[off][0], exp, TRACE_FIELDS)
        assert "affine_trace" in out[off][1]
    got = out[0][0]
    for k in range(len(pairs)):
        assert affine_trace_ref.rescore(got["cons_x"][k], got["cons_y"][k], *sc.ref_args()) == got["score"][k], k
    again = ctx.affine_pairs_trace(*([p[k] for p in pairs] for k in range(3)), **sc.kw())   # the scratch is reused
    same(again, got, TRACE_FIELDS)
    assert ctx.last_timings()["trace_us"] > 0
    for k in sample:
        q, lo, hi = pairs[k]
        one = ctx.affine_align_trace(xs[q], y[lo:hi], **sc.kw())
        for f in TRACE_FIELDS:
            assert one[f] == got[f][k], (k, f, one[f], got[f][k])
    return got


def test_trace_gaps(ctx, pgs):
    g = gap_case(pgs)
    got = check_trace(ctx, pgs, g["xs"], g["y"], g["pairs"], sample=(0, 1, 4))
    assert "3D" in got["cigar"][0] and "3I" in got["cigar"][1] and "70D" in got["cigar"][2], got["cigar"][:3]


def test_trace_ties(ctx, pgs):
    x, y1, homo, x3, y3 = tie_cases(pgs)
    y = y1 + b"C" + homo[1] + b"C" + y3
    a = len(y1) + 1
    b = a + 100 + 1
    got = check_trace(ctx, pgs, [x, homo[0], x3], y, [(0, 0, len(y1)), (1, a, a + 100), (1, a, a + 20), (2, b, b + 18)], sample=(0, 3))
    assert got["cigar"][0] == "150M" and got["begin_y"][0] == 31 and got["cigar"][3] == "5M"


def test_trace_table_and_mixed_dispatch(ctx, pgs):
    sc = _scorings(pgs)[4]
    g = gap_case(pgs, sc)
    check_trace(ctx, pgs, g["xs"], g["y"], g["pairs"], sc=sc, sample=(1,))
    m = mixed_case(pgs)
    got = check_trace(ctx, pgs, m["xs"], m["y"], m["pairs"], sample=(1, 2))
    assert got["cigar"][1] == "513M" and "3I" in got["cigar"][2], got["cigar"]


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, pgs):
    y = pgs.synth.dna(8201, 3000).tobytes()
    xs = [read_of(pgs, y, 8210 + k, 400 * k + 100, 150) for k in range(4)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    pairs = [(k, 400 * k + 50, 400 * k + 320) for k in range(4)]
    exp = expected(xs, y, pairs, DEFAULT)
    base = affine_ref.locate_batch(xs, y)
    L = ctx._L
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    sc, ex, ey = (C.c_float * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()

    def still_fine():
        same(ctx.affine_pairs_run(*([t[k] for t in pairs] for k in range(3))), exp)
        assert pair_tags(ctx.last_path())
        got = ctx.affine_batch_run()
        assert np.array_equal(got["score"], base[0]) and np.array_equal(got["end_x"], base[1]) and np.array_equal(got["end_y"], base[2])

    def run(q=qa, lo=la, hi=ra, params=C.byref(p), s=sc, x=ex, yv=ey, count=n):
        return L.mi355_sw_affine_pairs_run(ctx._ctx, C.c_size_t(count), q, lo, hi, params, s, x, yv)

    def trace(q=qa, lo=la, hi=ra, params=C.byref(p), outs=res, count=n):
        return L.mi355_sw_affine_pairs_trace(ctx._ctx, C.c_size_t(count), q, lo, hi, params, outs)

    for bad in (dict(q=None), dict(lo=None), dict(hi=None), dict(params=None), dict(s=None), dict(x=None), dict(yv=None)):
        assert run(**bad) == EINVAL, bad
    for bad in (dict(q=None), dict(lo=None), dict(hi=None), dict(params=None), dict(outs=None)):
        assert trace(**bad) == EINVAL, bad
    still_fine()
    for q, lo, hi in (((0, -1), (0, 10), (100, 200)), ((0, 4), (0, 10), (100, 200)), ((0, 1), (-1, 10), (100, 200)),
                      ((0, 1), (0, 300), (100, 200)), ((0, 1), (0, 10), (100, 3001))):
        args = dict(q=(C.c_int32 * n)(*q), lo=(C.c_int64 * n)(*lo), hi=(C.c_int64 * n)(*hi))
        assert run(**args) == EINVAL and trace(**args) == EINVAL, (q, lo, hi)
        assert len(L.mi355_sw_last_error(ctx._ctx)) > 0
    assert list(sc) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7]
    still_fine()
    # npairs == 0: 0, and nothing is written (not even through NULL arrays)
    assert run(count=0) == 0 and run(q=None, lo=None, hi=None, s=None, x=None, yv=None, count=0) == 0 and trace(outs=None, count=0) == 0
    assert list(sc) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7]
    got = ctx.affine_pairs_run([], [], [])
    assert len(got["score"]) == 0
    for kw in (dict(gap_open=1.0, gap_extend=2.0), dict(gap_open=3.0, gap_extend=0.0), dict(match=float("nan"))):
        for call in (ctx.affine_pairs_run, ctx.affine_pairs_trace):
            with pytest.raises(pgs.MI355Error) as e:
                call([0], [0], [100], **kw)
            assert e.value.code == EINVAL
    with pytest.raises(pgs.MI355Error) as e:
        ctx.affine_pairs_run([0], [0], [100], match=3.5)
    assert e.value.code == ENOTSUP and "integer" in str(e.value)
    with pytest.raises(ValueError):
        ctx.affine_pairs_run([0, 1], [0], [100])
    still_fine()
