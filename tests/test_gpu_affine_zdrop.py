"""The banded extension under the z-drop stop rule on the device (mi355_sw_affine_extend_run_zdrop / _trace_zdrop) against
tests/affine_zdrop_ref.py applied to the letters x[q_lo:q_hi] and the slice y[left:right].  Every case runs through both dispatches —
the default one (sw_affine_band_extz_kernel where it admits the pair) and option no_affine_band (the exact path: the rows instance,
the rule on the host, the exact kernel under the band on the first rows_done rows) — and through both calls, run and trace: every
field, rows_done included, must equal the checker; the strings must be worth the traced score; every emitted cell must lie in the
band and in rows <= rows_done; the path must show which kernel ran.  Scores are integers: no tolerance.  What a case is built to show
(a stop at a given row, a tie, a detour that survives only with the diagonal term) is asserted on the checker's own values first.
Expected values are computed once per case."""
import numpy as np
import pytest

from tests import affine_extend_band_ref as br, affine_zdrop_ref as zr, score_instances as si
from tests.test_gpu_affine_extend_band import BAND_R, Pair, Scoring, band_of, call_args, columns, instance_of, same

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
NINF, INF = float("-inf"), float("inf")
RUN_FIELDS = ("score", "end_x", "end_y", "to_end_score", "to_end_y", "rows_done")
TRACE_FIELDS = RUN_FIELDS + ("pos", "cons_x", "cons_y", "cigar")
Z1 = Scoring("1/-4/7/1", 1, -4, 7, 1)
Z2 = Scoring("2/-6/10/2", 2, -6, 10, 2)
Z3 = Scoring("3/-9/12/2", 3, -9, 12, 2)
OTHER = {65: 67, 67: 71, 71: 84, 84: 65}                            # a letter that mismatches: A -> C -> G -> T -> A


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def junk(y, at, k):
    """k letters that mismatch y[at:at + k] position by position."""
    return bytes(OTHER[c] for c in y[at:at + k])


def falling(y, at, good, m):
    """A read of m rows: `good` letters of y from `at`, then letters that mismatch the diagonal."""
    return y[at:at + good] + junk(y, at + good, m - good)


def reference(x, y, p, sc, zdrop):
    """(the run call's fields, the trace call's fields) by the checker from ONE fill over the clipped window: rows <= rows_done of the
    full matrices are the matrices of the truncated pair (tests/test_affine_zdrop_ref.py pins that against zr.locate / zr.trace)."""
    xb, yb = br._b(x), br._b(y)
    if p.back:
        xb, yb = xb[::-1], yb[::-1]
    yb = yb[:br.clip(len(xb), len(yb), p.bhi)]
    m = len(xb)
    H, E, F, S = br.matrices(xb, yb, p.blo, p.bhi, **sc.kw())
    s = zr.stop_row(H, sc.ext, zdrop) if m else 0
    H, E, F, S = H[:s + 1], E[:s + 1], F[:s + 1], S[:s + 1]
    b, i, j = br.best(H)
    ts, tj = br.to_end(H) if s == m else (NINF, -1)
    run = dict(score=b, end_x=i, end_y=j, to_end_score=ts, to_end_y=tj, rows_done=s)
    if p.to_end and tj < 0:
        return run, dict(run, score=NINF, end_x=0, end_y=0, pos=0, cons_x="", cons_y="", cigar="")
    cs, ci, cj = (ts, s, tj) if p.to_end else (b, i, j)
    cx, cy = br.walk(xb[:s], yb, H, E, F, S, ci, cj, sc.open)
    tr = dict(run, score=cs, end_x=ci, end_y=cj, pos=1 if cj > 0 else 0, cons_x=cx, cons_y=cy,
              cigar=br.cigar(cx[::-1], cy[::-1]) if p.back else br.cigar(cx, cy))
    return run, tr


def expected(xs, y, pairs, sc, zdrop, definition=8):
    both = [reference(p.letters(xs), y[p.lo:p.hi], p, sc, zdrop) for p in pairs]
    for p, (run, tr) in list(zip(pairs, both))[:definition]:          # the first pairs also by the definition itself, two fills each
        x, w = p.letters(xs), y[p.lo:p.hi]
        assert zr.locate(x, w, p.blo, p.bhi, zdrop, bool(p.back), **sc.kw()) == run
        assert zr.trace(x, w, p.blo, p.bhi, zdrop, bool(p.back), bool(p.to_end), **sc.kw()) == tr
    return columns([b[0] for b in both], RUN_FIELDS), columns([b[1] for b in both], TRACE_FIELDS)


def check(ctx, xs, y, pairs, zdrop, sc=Z1, exp=None, upload=True, kernels="band", options=("no_affine_band",)):
    """The default dispatch and one per option, both calls: equal to the checker field for field; the paths name the kernels.  kernels:
    what the pairs of the default dispatch run on — "band", "exact", "both" or "none" (host-filled pairs only).  exp: the
    checker's values where the test computed them first (expected()).  Returns (run, trace) of the checker."""
    exp = expected(xs, y, pairs, sc, zdrop) if exp is None else exp
    q, lo, hi, kw, te = call_args(pairs)
    if upload:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
    for option in (None,) + tuple(options):
        if option:
            ctx.set_option(option, 1)
        try:
            got = ctx.affine_extend_zdrop_run(q, lo, hi, zdrop=zdrop, **kw, **sc.kw())
            p_run, c_run = ctx.last_path(), ctx.last_counters()
            traced = ctx.affine_extend_zdrop_trace(q, lo, hi, to_end=te, zdrop=zdrop, **kw, **sc.kw())
            p_trace = ctx.last_path()
        finally:
            if option:
                ctx.set_option(option, 0)
        same(got, exp[0], RUN_FIELDS)
        same(traced, exp[1], TRACE_FIELDS)
        ms = np.array([len(p.letters(xs)) for p in pairs])
        assert c_run["zdrop_stopped"] == int((exp[0]["rows_done"] < ms).sum())
        for k, p in enumerate(pairs):
            if traced["score"][k] == NINF:
                continue
            assert br.rescore(traced["cons_x"][k], traced["cons_y"][k], **sc.kw()) == traced["score"][k], k
            cells = br.path_cells(traced["cons_x"][k], traced["cons_y"][k], int(traced["end_x"][k]), int(traced["end_y"][k]))
            assert all(br.in_band(i, j, p.blo, p.bhi) and i <= traced["rows_done"][k] for i, j in cells), k
        on_band = option is None and kernels in ("band", "both")
        on_exact = kernels != "none" and (option is not None or kernels in ("exact", "both"))
        for path in (p_run, p_trace):
            tags = [t for t in path if t.startswith("affine_band")]
            assert all(t.startswith("affine_band_extz[R=") for t in tags), path
            assert (len(tags) > 0) == on_band, (option, path)
            assert ("affine_exact_band_rows" in path) == on_exact and ("affine_exact_band" in path) == on_exact, (option, path)
            assert not any(t.startswith("affine_pair") or t == "affine_exact" for t in path), path   # every pair is a banded pair
    return exp


# ---- every compiled instance at its widest band and at the narrowest it serves: reads of 40 rows -----------------------------------------
@pytest.mark.parametrize("R", BAND_R)
def test_every_instance(ctx, pgs, R):
    y = pgs.synth.dna(15100 + R, 1200).tobytes()
    a = 300
    xs = [y[a:a + 40], falling(y, a, 22, 40), falling(y, a, 9, 40)]
    pairs = []
    for W in (16 * R, 16 * (R - 1) + 1):
        lo, hi = band_of(40, W)
        assert instance_of(W) == R
        pairs += [Pair(k, a, a + 40 + hi + 5, lo, hi, to_end=(k + W) % 2) for k in range(3)]
    exp = check(ctx, xs, y, pairs, 3.0)
    assert list(exp[0]["rows_done"]) == [40, 23, 10] * 2 and list(exp[0]["score"]) == [40, 22, 9] * 2
    lo, hi = band_of(40, 16 * R)
    ctx.affine_extend_zdrop_run([0], [a], [a + 40 + hi + 5], band_lo=lo, band_hi=hi, zdrop=3.0, **Z1.kw())
    assert ctx.last_path() == ["affine_band_extz[R=%d]" % R], ctx.last_path()
    ki = ctx.last_kernel()
    assert ki["name"] == "sw_affine_band_extz_kernel<R=%d>" % R and ki["dtype"] == "f32" and ki["rows_per_lane"] == R, ki
    ext = 15.0 + ((R + 1) // 2 + 33.0) / R                             # the extension instance's count: the rule costs more
    assert ki["cells"] == 40 * 16 * R and ext + 3 < ki["valu_ops_per_cell"] < ext + 6 + 60.0 / R


# ---- where the stop falls -----------------------------------------------------------------------------------------------------------------------
def test_stop_rows_and_the_tie(ctx, pgs):
    """zdrop 3 under 1/-4/7/1: the first letter that mismatches drops the row maximum by 4 and stops; zdrop 4 is the tie B - r - d e ==
    zdrop, which does not stop: the next row (6 by the gap, 8 by the diagonal) does."""
    y = pgs.synth.dna(15201, 800).tobytes()
    a, m = 100, 40
    xs = [falling(y, a, 0, m), falling(y, a, m - 2, m), falling(y, a, m - 1, m), falling(y, a, 17, m), y[a:a + m]]
    pairs = [Pair(k, a, a + m + 18, -8, 8, to_end=k % 2) for k in range(5)] + [Pair(k, a, a + m + 18, -8, 8, to_end=1 - k % 2) for k in range(5)]
    exp = check(ctx, xs, y, pairs, 3.0)
    assert list(exp[0]["rows_done"][:5]) == [1, m - 1, m, 18, m]        # row 1, row m - 1, a drop at row m alone: not tested
    assert exp[0]["to_end_score"][2] == m - 1 - 4 and exp[0]["to_end_y"][2] == m and exp[0]["to_end_score"][1] == NINF
    assert list(exp[0]["score"][:5]) == [0, m - 2, m - 1, 17, m]
    tie = check(ctx, xs, y, pairs, 4.0, upload=False)
    assert list(tie[0]["rows_done"][:5]) == [2, m, m, 19, m]
    half = check(ctx, xs, y, pairs, 3.5, upload=False)                  # the drop is an integer: 3.5 is 3
    assert list(half[0]["rows_done"]) == list(exp[0]["rows_done"])


def test_the_diagonal_term(ctx, pgs):
    """Three letters inserted (the row maximum moves left of the best's diagonal) and three columns skipped (right of it): without the
    term d e the detour's rows drop by more than zdrop, with it they do not — asserted on the checker by running its rule with e = 0."""
    y = pgs.synth.dna(15301, 800).tobytes()
    a = 100
    xs = [y[a:a + 20] + junk(y, a + 20, 3) + y[a + 20:a + 60], y[a:a + 20] + y[a + 23:a + 63]]
    pairs = [Pair(0, a, a + 90, -8, 8, 0, 63), Pair(1, a, a + 90, -8, 8, 0, 60, to_end=1), Pair(0, a + 5, a + 90, -8, 8, 5, 63, to_end=1)]
    for p in pairs[:2]:
        H = br.matrices(p.letters(xs), y[p.lo:p.hi], p.blo, p.bhi, **Z1.kw())[0]
        assert zr.stop_row(H, 1.0, 5.0) == len(p.letters(xs)) and 20 < zr.stop_row(H, 0.0, 5.0) < 26
    exp = check(ctx, xs, y, pairs, 5.0)
    assert list(exp[0]["rows_done"]) == [63, 60, 58] and exp[1]["cigar"][0] == "20M3I40M" and "3D" in exp[1]["cigar"][1]
    assert list(exp[1]["score"]) == [60 - 9, 60 - 9, 55 - 9]         # one gap of three letters: 7 + 2
    # a smaller zdrop and both detours stop
    less = check(ctx, xs, y, pairs[:2], 3.0, upload=False)
    assert list(less[0]["rows_done"]) == [21, 21]


def test_windows_that_end_early(ctx, pgs):
    """A window that ends inside the band's reach while the read falls: the columns beyond n are padding, and the F chain down column
    n + 1 must not be taken for a row maximum.  A window that ends before the read does: the first row without an in-band real
    column stops, whatever zdrop."""
    y = pgs.synth.dna(15401, 800).tobytes()
    a = 100
    xs = [falling(y, a, 24, 60), y[a:a + 60]]
    pairs = [Pair(0, a, a + 26, -8, 8), Pair(0, a, a + 26, -8, 8, to_end=1), Pair(0, a, a + 24, -12, 3),
             Pair(1, a, a + 20, -4, 8), Pair(1, a, a + 20, -4, 8, to_end=1), Pair(1, a, a + 20, 0, 8), Pair(1, a, a + 59, -8, 8, to_end=1)]
    exp = check(ctx, xs, y, pairs, 20.0)
    assert 25 < exp[0]["rows_done"][0] < 60 and exp[0]["score"][0] == 24
    assert list(exp[0]["rows_done"][3:]) == [25, 25, 21, 60]            # rows i with i + band_lo > n have no real column
    big = check(ctx, xs, y, pairs[3:], float(2 ** 20), upload=False)
    assert list(big[0]["rows_done"]) == [25, 25, 21, 60]


def test_empty_windows_and_empty_reads(ctx, pgs):
    y = pgs.synth.dna(15501, 400).tobytes()
    xs = [y[50:58], y[50:90]]
    pairs = [Pair(0, 50, 50, -8, 3, 0, 8), Pair(0, 50, 50, -8, 3, 0, 8, to_end=1), Pair(0, 50, 50, -3, 3, 0, 8, to_end=1),
             Pair(0, 60, 70, -3, 3, 4, 4), Pair(0, 50, 50, -8, 3, 2, 3, to_end=1)]
    exp = check(ctx, xs, y, pairs, 6.0, kernels="none")                 # o - e = 6 does not exceed zdrop: only the band stops
    assert list(exp[0]["rows_done"]) == [8, 8, 4, 0, 1] and exp[0]["to_end_score"][0] == -14 and exp[0]["to_end_score"][2] == NINF
    exp = check(ctx, xs, y, pairs, 5.0, kernels="none", upload=False)
    assert list(exp[0]["rows_done"]) == [1, 1, 1, 0, 1] and exp[0]["to_end_score"][0] == NINF and exp[0]["to_end_score"][4] == -7
    check(ctx, xs, y, pairs + [Pair(1, 50, 100, -8, 8, 0, 40)], 5.0, upload=False)


# ---- four slots of one wavefront ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ((0, 1, 2), (2, 0, 1)))
def test_four_slots_of_a_wavefront(ctx, pgs, order):
    """Rows 5 and 60, never, and an idle slot: the wavefront runs on for its live slot, the stopped ones keep their results."""
    y = pgs.synth.dna(15601, 800).tobytes()
    a, m = 100, 150
    reads = [falling(y, a, 4, m), falling(y, a, 59, m), y[a:a + m]]
    xs = [reads[k] for k in order]
    pairs = [Pair(k, a, a + m + 18, -8, 8, to_end=k % 2) for k in range(3)]
    exp = check(ctx, xs, y, pairs, 3.0)
    assert list(exp[0]["rows_done"]) == [(5, 60, 150)[k] for k in order]
    ctx.affine_extend_zdrop_run(*call_args(pairs)[:3], band_lo=-8, band_hi=8, zdrop=3.0, **Z1.kw())
    assert ctx.last_timings()["score_launches"] == 1 and ctx.last_counters()["zdrop_rows_run"] == 150


def test_a_stopped_slot_ignores_what_later_rows_would_give(ctx, pgs):
    """30 matching letters, 15 that mismatch, 100 matching: the full matrix's best extension jumps the junk, the stopped one must not."""
    y = pgs.synth.dna(15702, 800).tobytes()
    a = 100
    xs = [y[a:a + 30] + junk(y, a + 30, 15) + y[a + 45:a + 145], y[a:a + 145]]
    pairs = [Pair(0, a, a + 170, -8, 8), Pair(0, a, a + 170, -8, 8, to_end=1), Pair(1, a, a + 170, -8, 8), Pair(0, a, a + 170, -16, 16)]
    # on the checker first: the full matrix's best and the truncated one differ
    full = br.locate(xs[0], y[a:a + 170], -8, 8, **Z1.kw())
    exp = expected(xs, y, pairs, Z1, 20.0)
    assert full["score"] > 60 and full["end_x"] == 145 and exp[0]["score"][0] == 30 and exp[0]["end_x"][0] == 30
    assert 30 < exp[0]["rows_done"][0] < 60 and 30 < exp[0]["rows_done"][3] < 70 and exp[0]["rows_done"][2] == 145
    assert exp[0]["to_end_score"][0] == NINF and (exp[1]["score"][1], exp[1]["cons_x"][1], exp[1]["end_x"][1]) == (NINF, "", 0)
    # the device must then return the truncated one
    check(ctx, xs, y, pairs, 20.0, exp=exp)


# ---- directions ---------------------------------------------------------------------------------------------------------------------------------
def test_backward_pairs_and_sub_ranges(ctx, pgs):
    y = pgs.synth.dna(15801, 2000).tobytes()
    x = junk(y, 400, 40) + y[440:560] + junk(y, 560, 40)              # letters 40..160 of the read lie at 440..560
    xs = [x, y[900:1000]]
    # a seed at read offset 90..110: to the right of it and to the left of it, each runs into junk 50 letters on
    pairs = [Pair(0, 510, 640, -12, 12, 110, 200), Pair(0, 370, 490, -12, 12, 0, 90, back=1),
             Pair(0, 510, 640, -12, 12, 110, 200, to_end=1), Pair(0, 370, 490, -12, 12, 0, 90, back=1, to_end=1),
             Pair(1, 905, 1100, -3, 9, 5, 100), Pair(1, 700, 995, -3, 9, 0, 95, back=1, to_end=1)]
    exp = check(ctx, xs, y, pairs, 20.0)
    assert list(exp[0]["score"]) == [50, 50, 50, 50, 95, 95] and all(50 < s < 90 for s in exp[0]["rows_done"][:4])
    assert exp[1]["cigar"][0] == "50M" and exp[1]["cigar"][1] == "50M" and exp[1]["score"][2] == NINF and exp[1]["score"][5] == 95


# ---- identity -----------------------------------------------------------------------------------------------------------------------------------
def test_an_infinite_zdrop_is_the_banded_call(ctx, pgs):
    y = pgs.synth.dna(15901, 1200).tobytes()
    xs = [falling(y, 300, 60, 150), y[300:340], falling(y, 300, 5, 40)]
    q, lo, hi, back = [0, 1, 2, 0, 1], [300, 300, 300, 300, 700], [480, 360, 360, 300, 760], [0, 0, 0, 0, 1]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    for blo, bhi in ((-8, 8), ([-150, -40, -40, -150, -40], [180, 60, 60, 0, 60])):      # banded pairs; bands that cover the matrix
        want = ctx.affine_extend_trace(q, lo, hi, backward=back, to_end=[0, 1, 1, 1, 0], band_lo=blo, band_hi=bhi, **Z1.kw())
        p_want = ctx.last_path()
        got = ctx.affine_extend_zdrop_trace(q, lo, hi, backward=back, to_end=[0, 1, 1, 1, 0], band_lo=blo, band_hi=bhi, zdrop=INF, **Z1.kw())
        assert ctx.last_path() == p_want and not any("extz" in t or "rows" in t for t in p_want)
        assert list(got.pop("rows_done")) == [150, 40, 40, 150, 40]
        for f in want:
            assert (got[f].tobytes() == want[f].tobytes()) if isinstance(want[f], np.ndarray) else got[f] == want[f], f
        want = ctx.affine_extend_run(q, lo, hi, backward=back, band_lo=blo, band_hi=bhi, **Z1.kw())
        p_want = ctx.last_path()
        got = ctx.affine_extend_zdrop_run(q, lo, hi, backward=back, band_lo=blo, band_hi=bhi, zdrop=INF, **Z1.kw())
        assert ctx.last_path() == p_want and list(got.pop("rows_done")) == [150, 40, 40, 150, 40]
        assert sorted(got) == sorted(want) and all(got[f].tobytes() == want[f].tobytes() for f in want)
    # with a finite zdrop the covering bands stay bands; the aligner class's front end reaches the same entry points
    pairs = [Pair(0, 300, 480, -150, 180), Pair(1, 300, 360, -40, 60, to_end=1)]
    check(ctx, xs, y, pairs, 20.0, upload=False, kernels="both")        # 331 diagonals: the exact path; 101: the band kernel
    ctx.affine_extend_zdrop_run([1], [300], [360], band_lo=-40, band_hi=60, zdrop=20.0, **Z1.kw())
    assert ctx.last_path() == ["affine_band_extz[R=7]"]
    for tb in (False, True):
        want = (ctx.affine_extend_zdrop_trace if tb else ctx.affine_extend_zdrop_run)([0, 2], [300, 300], [480, 360], band_lo=-8, band_hi=8, zdrop=20.0, **Z1.kw())
        got = pgs.AffineSWAligner.extend_pairs_zdrop([0, 2], [300, 300], [480, 360], band=(-8, 8), zdrop=20.0, context=ctx, traceback=tb,
                                                     match=1, mismatch=-4, gap_open=7, gap_extend=1)
        assert sorted(got) == sorted(want) and all(list(got[f]) == list(want[f]) for f in want) and got["rows_done"][1] < 40
    with pytest.raises(ValueError):
        pgs.AffineSWAligner.extend_pairs_zdrop([0], [300], [480], zdrop=20.0, context=ctx)


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------------------
def test_exactness_bound_from_both_sides(ctx, pgs):
    """L24: the band kernel forms B - floor(zdrop), exact while zdrop < 2^24; at 2^24 the pairs take the exact path.  Only a row
    without a real column stops under such a zdrop."""
    y = pgs.synth.dna(16001, 800).tobytes()
    a = 100
    xs = [falling(y, a, 20, 60), y[a:a + 60]]
    pairs = [Pair(0, a, a + 80, -8, 8), Pair(1, a, a + 20, -4, 8, to_end=1), Pair(1, a, a + 80, -8, 8, to_end=1)]
    below, at = float(np.float32(2 ** 24 - 1)), float(2 ** 24)
    assert below == 2 ** 24 - 1
    exp = check(ctx, xs, y, pairs, below, kernels="band")
    assert list(exp[0]["rows_done"]) == [60, 25, 60]
    exp = check(ctx, xs, y, pairs, at, kernels="exact", upload=False)
    assert list(exp[0]["rows_done"]) == [60, 25, 60]


def test_pairs_beyond_the_band_kernel(ctx, pgs):
    y = pgs.synth.dna(16101, 2400).tobytes()
    a = 300
    xs = [falling(y, a, 350, 600), falling(y, a, 100, 400), falling(y, a, 30, 150)]
    wide = [Pair(1, a, a + 700, -128, 128), Pair(1, a, a + 700, -128, 128, to_end=1)]
    long_ = [Pair(0, a, a + 700, -8, 8), Pair(0, a, a + 700, -8, 8, to_end=1)]
    assert wide[0].effective(xs)[4] == 257
    exp = check(ctx, xs, y, wide + long_, 20.0, kernels="exact")
    assert 100 < exp[0]["rows_done"][0] < 400 and 350 < exp[0]["rows_done"][2] < 600
    check(ctx, xs, y, wide + long_ + [Pair(2, a, a + 200, -8, 8)], 20.0, kernels="both", options=("no_affine_band", "no_affine_pairs"), upload=False)


def test_errors_leave_the_context_usable(ctx, pgs):
    y = pgs.synth.dna(16201, 12_000).tobytes()
    xs = [y[100:4600], falling(y, 50, 30, 100)]
    good = [Pair(1, 50, 300, -8, 8), Pair(1, 50, 300, -8, 8, to_end=1)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    # 4500 rows: beyond the band kernel and beyond the rows instance of the exact kernel (4398 rows): refused, naming the bound
    for call in (ctx.affine_extend_zdrop_run, ctx.affine_extend_zdrop_trace):
        with pytest.raises(pgs.MI355Error) as e:
            call([1, 0], [50, 100], [300, 4700], band_lo=-8, band_hi=8, zdrop=20.0, **Z1.kw())
        assert e.value.code == ENOTSUP and "pair 1 " in str(e.value) and "4398 rows" in str(e.value) and "rows instance" in str(e.value)
        check(ctx, xs, y, good, 20.0, upload=False)
    # the same rows without the stop rule fit the exact kernel's 5600
    assert ctx.affine_extend_zdrop_run([0], [100], [4700], band_lo=-8, band_hi=8, zdrop=INF, **Z1.kw())["rows_done"][0] == 4500
    # the argument errors: no bands, a negative zdrop, a NaN — behind the band checks
    for kw, word in ((dict(zdrop=20.0), "required"), (dict(band_lo=-8, band_hi=8, zdrop=-1.0), "zdrop"),
                     (dict(band_lo=-8, band_hi=8, zdrop=float("nan")), "zdrop"), (dict(band_lo=1, band_hi=8, zdrop=-1.0), "anchor")):
        for call in (ctx.affine_extend_zdrop_run, ctx.affine_extend_zdrop_trace):
            with pytest.raises(pgs.MI355Error) as e:
                call([1], [50], [300], **kw)
            assert e.value.code == EINVAL and word in str(e.value), (kw, str(e.value))
    check(ctx, xs, y, good, 20.0, upload=False)


# ---- the early exit -----------------------------------------------------------------------------------------------------------------------------
def test_the_wavefronts_leave_early(ctx, pgs):
    """64 reads of 150 rows that all stop by row 12: 16 wavefronts, none runs beyond the last stop row of the list; with a zdrop that
    never fires every wavefront runs its 150 rows."""
    y = pgs.synth.dna(16301, 1200).tobytes()
    rng = np.random.default_rng(16302)
    a, m = 200, 150
    xs = [falling(y, a + 3 * k, int(rng.integers(0, 12)), m) for k in range(64)]
    pairs = [Pair(k, a + 3 * k, a + 3 * k + m + 18, -8, 8) for k in range(64)]
    exp = expected(xs, y, pairs, Z1, 3.0)
    top = int(exp[0]["rows_done"].max())
    assert top <= 12 and exp[0]["rows_done"].min() >= 1
    check(ctx, xs, y, pairs, 3.0, exp=exp)
    q, lo, hi, kw, _ = call_args(pairs)
    ctx.affine_extend_zdrop_run(q, lo, hi, zdrop=3.0, **kw, **Z1.kw())
    c = ctx.last_counters()
    assert c["zdrop_stopped"] == 64 and 16 <= c["zdrop_rows_run"] <= 16 * top
    never = ctx.affine_extend_zdrop_run(q, lo, hi, zdrop=float(2 ** 20), **kw, **Z1.kw())
    c = ctx.last_counters()
    assert c["zdrop_stopped"] == 0 and c["zdrop_rows_run"] >= 16 * m and list(never["rows_done"]) == [m] * 64


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------------------------
def fuzz_case(pgs, seed, alphabet, npairs, n_ref=6000):
    """Reads of 20..150 rows cut from the reference with 4 % substitutions, every second one's tail from a random point replaced by
    random letters; half widths 8 / 16 / 32, window m + w + 10, forward and backward."""
    rng = np.random.default_rng(seed)
    y = si.letters(pgs, seed, n_ref, alphabet).tobytes()
    alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    xs, pairs = [], []
    for k in range(npairs):
        m = int(rng.integers(20, 151))
        w = int(rng.choice((8, 16, 32)))
        n = m + w + 10
        at = int(rng.integers(n, n_ref - n))
        back = k % 4 >= 2
        x = np.frombuffer(y[at - m:at] if back else y[at:at + m], dtype=np.uint8).copy()
        flip = rng.random(m) < 0.04
        x[flip] = alpha[rng.integers(0, len(alpha), int(flip.sum()))]
        if k % 2:
            cut = int(rng.integers(0, m))
            tail = alpha[rng.integers(0, len(alpha), m - cut)]
            if back:
                x[:m - cut] = tail
            else:
                x[cut:] = tail
        xs.append(x.tobytes())
        pairs.append(Pair(k, at - n, at, -w, w, back=1, to_end=k % 3 == 0) if back else Pair(k, at, at + n, -w, w, to_end=k % 3 == 0))
    return xs, y, pairs


FUZZ = [(Z1, 20.0), (Z2, 40.0), (Z3, 60.0)]


@pytest.mark.parametrize("sc,zdrop", FUZZ, ids=[s.name for s, _ in FUZZ])
def test_fuzz(ctx, pgs, sc, zdrop):
    xs, y, pairs = fuzz_case(pgs, 16401, b"ACGT", 300)
    exp = check(ctx, xs, y, pairs, zdrop, sc)
    ms = np.array([len(x) for x in xs])
    stopped = int((exp[0]["rows_done"] < ms).sum())
    assert 60 <= stopped <= 240, stopped                                # at least a fifth stop and at least a fifth do not
    assert (exp[0]["score"] >= 20 * sc.match).sum() > 60


def test_fuzz_protein_table(ctx, pgs):
    a, b = np.arange(256)[:, None], np.arange(256)[None, :]           # 4..6 for a letter against itself, -1..-4 otherwise: random letters fall
    lut = np.where(a == b, 4 + a % 3, -(1 + (7 * a + 3 * b) % 4)).astype(np.float32)
    sc = Scoring("lut/aa20/11/1", gap_open=11, gap_extend=1, lut=lut)
    xs, y, pairs = fuzz_case(pgs, 16402, si.AA20, 80)
    exp = check(ctx, xs, y, pairs, 25.0, sc)
    ms = np.array([len(x) for x in xs])
    stopped = int((exp[0]["rows_done"] < ms).sum())
    assert 10 <= stopped <= 70, stopped
