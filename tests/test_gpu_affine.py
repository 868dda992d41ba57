"""Affine-gap score and end cell on the device (mi355_sw_affine_*) against tests/affine_ref.py, the checker that
tests/test_affine_ref.py pins to the reference's oracle: whole problems on the exact kernel, every tile shape of the sweep kernel
on inputs whose planted gaps lie where a tile kernel goes wrong, scorings up to the float16 bound, the linear special case against
the oracle and the linear engine, option no_affine_sweep, and the error codes.  Expected values are computed once per module."""
import numpy as np
import pytest

from tests import affine_ref, score_instances as si

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
A = "ACGGTCATGCTA"
B = "GTACCTGAATCG"
KNOWN = [(A + B, "CCCC" + A + "TTT" + B + "CCCC", (24, 31)), (A + "GGG" + B, "CCCC" + A + B + "CCCC", (27, 28))]
KNOWN_SCORES = {(5, 1): 65, (5, 5): 57, (1, 1): 69, (2, 2): 66, (7, 2): 61}


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


SWEEP = Scoring("3/-3/4/1", 3, -3, 4, 1)
CL = 256                                                            # option `chunk`: the tile length of the sweep cases


class Case:
    """One (reference, batch, ranges) of a tile shape (SL, R); L / l = the longest / shortest query length of the shape's bucket.

    Ranges (tiles of CL columns, at least four each; no start is a multiple of 4): 0 and 1 are adjacent, 2 ends at the reference's
    last column.  Queries, in upload order; sorted by length the pairs are (1, 0) (2, 3) (4 alone): l and L in one pair, and the
    last workgroup has no second query.
      0  L, copy in range 0 with 3 reference letters inserted across the boundary of tiles 1 and 2 (a gap of 3 columns: E)
      1  l, exact copy ending in range 2's last column
      2  L, copy in range 1 with 3 of its letters missing in the reference, right below a row boundary between two lanes
         (a gap of 3 rows that F carries from one lane to the next)
      3  L, unrelated
      4  L, copy in range 0 with 70 reference letters inserted (a gap longer than a 64-step segment) where the flanks outscore
         it; an exact copy otherwise
    """

    def __init__(self, pgs, shape, sc, seed=0):
        lens, slot = si.shape_lengths(shape)
        self.shape, self.sc, self.slot = shape, sc, slot
        L, l = lens[-1], lens[0]
        SL, R = shape
        self.L, self.l = L, l
        base = 7000003 * (SL * 100 + R) + 101 * seed
        off4 = lambda v: v + (v % 4 == 0)
        w0 = off4(max(1100, 2 * CL + 2 * L + 130) + 1) - 1          # range 0 = [1, 1 + w0): range 1 starts off a multiple of 4
        w1 = max(1100, L + 300)
        r0 = (1, 1 + w0)
        r1 = (r0[1], r0[1] + w1)
        s2 = off4(r1[1] + 37)
        n = s2 + max(1100, l + 600)
        self.ranges = [r0, r1, (s2, n)]
        assert all(b - a >= max(1024, 4 * CL) and a % 4 for a, b in self.ranges)
        ref = si.letters(pgs, base + 1, n, sc.alpha).copy()
        q = [si.letters(pgs, base + 10 + k, m, sc.alpha).copy() for k, m in enumerate((L, l, L, L, L))]
        ins = lambda k, cnt: si.letters(pgs, base + 50 + k, cnt, sc.alpha)
        h = L // 2
        bnd = r0[0] + 2 * CL                                       # first column of tile 2 of range 0
        at0 = bnd - 1 - h
        p0 = np.concatenate([q[0][:h], ins(0, 3), q[0][h:]])       # inserted letters at columns bnd - 1 .. bnd + 1
        ref[at0:at0 + len(p0)] = p0
        self.gap70 = sc.lut is None and sc.match * h > sc.open + 69 * sc.ext + 30
        p4 = np.concatenate([q[4][:h], ins(4, 70), q[4][h:]]) if self.gap70 else q[4]
        at4 = at0 + len(p0) + 20
        ref[at4:at4 + len(p4)] = p4
        assert at0 >= r0[0] and at4 + len(p4) <= r0[1]
        rb = R * -(-8 // R)                                        # a lane boundary with at least 8 rows above it
        p2 = np.concatenate([q[2][:rb], q[2][rb + 3:]])
        at2 = r1[0] + 150
        ref[at2:at2 + len(p2)] = p2
        ref[n - l:] = q[1]
        self.ref = ref.tobytes()
        self.queries = [v.tobytes() for v in q]
        self.gapped = [(0, 0), (2, 1)] + ([(4, 0)] if self.gap70 else [])   # (query, range) of the planted gaps
        self.expected = None

    def compute(self):
        """Per-range maxima [3, nq], (score, end_x, end_y)[nq] over the whole reference, and what the planted gaps must show."""
        if self.expected is None:
            a = self.sc.ref_args()
            mx = np.array([affine_ref.locate_batch(self.queries, self.ref[lo:hi], *a)[0] for lo, hi in self.ranges])
            whole = affine_ref.locate_batch(self.queries, self.ref, *a)
            faults = []
            for k, r in self.gapped:
                lo, hi = self.ranges[r]
                lin = [affine_ref.locate(self.queries[k], self.ref[lo:hi], *self.sc.ref_args(g))[0] for g in (self.sc.open, self.sc.ext)]
                if mx[r, k] == lin[0] or mx[r, k] == lin[1]:
                    faults.append("query %d in range %d: affine %g, linear %g at open, %g at extend: the gap does not matter" % (k, r, mx[r, k], lin[0], lin[1]))
            self.expected = (mx, whole, faults)
        return self.expected


_cases = {}


def case_of(pgs, shape, sc=SWEEP):
    key = (shape, sc.name)
    if key not in _cases:
        _cases[key] = Case(pgs, shape, sc)
    return _cases[key]


def run_case(ctx, c, extra_options=()):
    """(per-range maxima, batch result, paths of both calls) of case c on the device, every option reset afterwards."""
    opts = [("chunk", CL)] + ([("slot", c.slot)] if c.slot else []) + [(o, 1) for o in extra_options]
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        ctx.set_reference(c.ref)
        ctx.batch_upload(c.queries)
        mx = ctx.affine_score_ranges(c.ranges, **c.sc.kw())
        p1 = ctx.last_path()
        got = ctx.affine_batch_run(**c.sc.kw())
        p2 = ctx.last_path()
    finally:
        for k, _ in opts:
            ctx.set_option(k, 0)
    return mx, got, p1, p2


def check_case(c, mx, got):
    emx, (es, ei, ej), faults = c.compute()
    assert not faults, faults
    assert np.array_equal(mx.astype(np.float64), emx), (c.shape, mx.tolist(), emx.tolist())
    assert np.array_equal(got["score"].astype(np.float64), es), (c.shape, got["score"].tolist(), es.tolist())
    assert np.array_equal(got["end_x"], ei) and np.array_equal(got["end_y"], ej), (c.shape, got["end_x"].tolist(), ei.tolist(), got["end_y"].tolist(), ej.tolist())


SWEEP_SHAPES = [(16, r) for r in si.R16] + [(8, r) for r in si.R8]


# ---- whole problems: the exact kernel ---------------------------------------------------------------------------------------------
def test_known_answers(ctx):
    for x, y, end in KNOWN:
        for (go, ge), score in KNOWN_SCORES.items():
            r = ctx.affine_align(x, y, gap_open=go, gap_extend=ge)
            assert (r["score"], r["end_x"], r["end_y"]) == (float(score), end[0], end[1]), (x, go, ge, r)
            assert "affine_exact" in ctx.last_path()


def test_small_pairs_exact(ctx):
    scorings = [(3, -3, 5, 1), (1, -1, 4, 2), (2, 0, 3, 1), (10, -2, 12, 1), (5, -4, 9, 7), (3, -3, 2, 2), (1, -1, 4, 4)]
    rng = np.random.default_rng(4711)
    bad = []
    for k in range(200):
        alpha = np.frombuffer(b"ACGT" if k % 2 == 0 else b"AC", dtype=np.uint8)
        m, n = int(rng.integers(1, 41)), int(rng.integers(1, 121))
        x = alpha[rng.integers(0, len(alpha), m)].tobytes()
        y = bytearray(alpha[rng.integers(0, len(alpha), n)].tobytes())
        if k % 3 == 0 and n >= m + 2 and m >= 8:
            at = int(rng.integers(0, n - m - 1))
            y[at:at + m + 2] = x[:m // 2] + alpha[rng.integers(0, len(alpha), 2)].tobytes() + x[m // 2:]
        ma, mi, go, ge = scorings[k % len(scorings)]
        exp = affine_ref.locate(x, bytes(y), ma, mi, go, ge)
        r = ctx.affine_align(x, bytes(y), match=ma, mismatch=mi, gap_open=go, gap_extend=ge)
        if (r["score"], r["end_x"], r["end_y"]) != exp:
            bad.append((k, r, exp))
    assert not bad, bad[:5]


def test_degenerate_inputs(ctx):
    assert ctx.affine_align("", "ACGT") == dict(score=0.0, end_x=0, end_y=0)
    assert ctx.affine_align("ACGT", "") == dict(score=0.0, end_x=0, end_y=0)
    assert ctx.affine_align("AAAA", "CCCCCCC") == dict(score=0.0, end_x=0, end_y=0)           # nothing matches
    x, y = "ACGTTGCAGGTCA" * 3, "TTGCAGG"                                                    # query longer than the reference
    r = ctx.affine_align(x, y)
    assert (r["score"], r["end_x"], r["end_y"]) == affine_ref.locate(x, y) and r["score"] == 21.0


# ---- the sweep kernel, every tile shape -------------------------------------------------------------------------------------------
def test_shape_lists_are_those_of_the_host():
    h = si.lists_in_header()
    assert h["kR16"] == si.R16 and h["kR8"] == si.R8 and len(SWEEP_SHAPES) == 17


@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "SL%d_R%d" % s)
def test_sweep_shape(ctx, pgs, shape):
    c = case_of(pgs, shape)
    assert not c.compute()[2], c.compute()[2]                      # the planted gaps matter, by the checker alone
    mx, got, p1, p2 = run_case(ctx, c)
    check_case(c, mx, got)
    tag = "affine[cell=f16,SL=%d,R=%d]" % shape
    assert tag in p1 and tag in p2, (p1, p2)
    assert "affine_exact" in p2 and "affine_exact" not in p1       # the end cells come from the exact kernel behind the sweep


# ---- scorings ---------------------------------------------------------------------------------------------------------------------
def _scorings(pgs):
    return [Scoring("3/-3/5/1", 3, -3, 5, 1), Scoring("2/0/3/1", 2, 0, 3, 1), Scoring("10/-2/12/1", 10, -2, 12, 1),
            Scoring("1/-1/4/2", 1, -1, 4, 2),
            Scoring("lut/aa20/11/1", gap_open=11, gap_extend=1, lut=pgs.synth.make_lut(4242, 1.0), alpha=si.AA20)]


@pytest.mark.parametrize("shape", [(8, 19), (16, 10)], ids=lambda s: "SL%d_R%d" % s)
@pytest.mark.parametrize("which", range(5))
def test_scorings(ctx, pgs, shape, which):
    sc = _scorings(pgs)[which]
    c = case_of(pgs, shape, sc)
    mx, got, p1, p2 = run_case(ctx, c)
    check_case(c, mx, got)
    assert "affine[cell=f16,SL=%d,R=%d]" % shape in p1


def _bound_case(pgs, m):
    ref = pgs.synth.dna(900 + m, 1500).copy()
    qs = [pgs.synth.dna(910 + m + k, m).copy() for k in range(3)]
    ref[200:200 + m] = qs[0]                                        # the perfect score 8 m
    ref[700:700 + m // 2] = qs[1][:m // 2]
    ref[700 + m // 2 + 2:702 + m] = qs[1][m // 2:]
    return ref.tobytes(), [q.tobytes() for q in qs]


def test_float16_bound_from_both_sides(ctx, pgs):
    kw = dict(match=8.0, mismatch=-5.0, gap_open=6.0, gap_extend=2.0)
    ref, qs = _bound_case(pgs, 254)                                 # smax * (maxlen + 1) = 8 * 255 = 2040: the sweep, exact
    ctx.set_reference(ref)
    ctx.batch_upload(qs)
    got = ctx.affine_batch_run(**kw)
    assert any(t.startswith("affine[") for t in ctx.last_path())
    es, ei, ej = affine_ref.locate_batch(qs, ref, 8, -5, 6, 2)
    assert es[0] == 8 * 254
    assert np.array_equal(got["score"], es) and np.array_equal(got["end_x"], ei) and np.array_equal(got["end_y"], ej)
    ref, qs = _bound_case(pgs, 255)                                 # one past it: exact, or refused
    ctx.set_reference(ref)
    ctx.batch_upload(qs)
    try:
        got = ctx.affine_batch_run(**kw)
    except pgs.MI355Error as e:
        assert e.code == ENOTSUP
    else:
        es, ei, ej = affine_ref.locate_batch(qs, ref, 8, -5, 6, 2)
        assert np.array_equal(got["score"], es) and np.array_equal(got["end_x"], ei) and np.array_equal(got["end_y"], ej)


# ---- gap_open == gap_extend: the reference's linear model -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 1024, 1025, 6007])
def test_linear_case_equals_oracle_and_linear_engine(ctx, pgs, oracle, n):
    ref = pgs.synth.dna(300 + n, n).copy()
    qs = [pgs.synth.read_from_ref(ref, 40 + k, 150, sub_rate=0.03, indel_rate=0.02)[0].tobytes() for k in range(6)]
    qs.append(pgs.synth.dna(77, 97).tobytes())
    tail = pgs.synth.dna(78, 120)
    ref[n - 120:] = tail                                            # an exact copy ending in the last column
    qs.append(tail.tobytes())
    ref = ref.tobytes()
    ctx.set_reference(ref)
    ctx.batch_upload(qs)
    for ma, mi, g in ((3, -3, 2), (1, -1, 4)):
        got = ctx.affine_batch_run(match=ma, mismatch=mi, gap_open=g, gap_extend=g)
        path = ctx.last_path()
        assert any(t.startswith("affine[") for t in path) == (n >= 1024), path
        lin = ctx.batch_run(match=ma, mismatch=mi, gap=g, flags=pgs.capi.SCORE_ONLY)
        for k, q in enumerate(qs):
            exp = oracle.locate(q, ref, 0, match=float(ma), mismatch=float(mi), gap=float(g))
            mine = (float(got["score"][k]), int(got["end_x"][k]), int(got["end_y"][k]))
            assert mine == (float(exp[0]), int(exp[1]), int(exp[2])), (n, k, mine, exp)
            assert mine == (lin[k]["score"], lin[k]["end_x"], lin[k]["end_y"]), (n, k, mine, lin[k])


# ---- option no_affine_sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 19), (16, 32)], ids=lambda s: "SL%d_R%d" % s)
def test_no_affine_sweep(ctx, pgs, shape):
    c = case_of(pgs, shape)
    mx, got, p1, p2 = run_case(ctx, c, extra_options=("no_affine_sweep",))
    check_case(c, mx, got)
    for p in (p1, p2):
        assert "affine_exact" in p and not any(t.startswith("affine[") for t in p), p


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, pgs, oracle):
    ref = pgs.synth.dna(5150, 3000)
    qs = [pgs.synth.read_from_ref(ref, 60 + k, 150)[0].tobytes() for k in range(4)]
    ref = ref.tobytes()
    ctx.set_reference(ref)
    ctx.batch_upload(qs)
    for kw in (dict(gap_open=1.0, gap_extend=2.0), dict(gap_open=3.0, gap_extend=0.0), dict(gap_open=float("nan"), gap_extend=1.0),
               dict(match=float("nan")), dict(gap_open=5.0, gap_extend=float("inf"))):
        for call in (lambda: ctx.affine_batch_run(**kw), lambda: ctx.affine_align(qs[0], ref, **kw),
                     lambda: ctx.affine_score_ranges([(0, 2000)], **kw)):
            with pytest.raises(pgs.MI355Error) as e:
                call()
            assert e.value.code == EINVAL, kw
    with pytest.raises(pgs.MI355Error) as e:
        ctx.affine_batch_run(match=3.5, mismatch=-2.25)
    assert e.value.code == ENOTSUP
    assert len(ctx._L.mi355_sw_last_error(ctx._ctx)) > 0 and "integer" in str(e.value)
    lin = ctx.batch_run(flags=pgs.capi.SCORE_ONLY)
    for k, q in enumerate(qs):
        exp = oracle.locate(q, ref, 0)
        assert (lin[k]["score"], lin[k]["end_x"], lin[k]["end_y"]) == (float(exp[0]), int(exp[1]), int(exp[2]))
    got = ctx.affine_batch_run()
    es, ei, ej = affine_ref.locate_batch(qs, ref)
    assert np.array_equal(got["score"], es) and np.array_equal(got["end_x"], ei) and np.array_equal(got["end_y"], ej)
