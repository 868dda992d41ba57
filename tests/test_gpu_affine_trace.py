"""Affine-gap traceback on the device (mi355_sw_affine_align_trace / _batch_trace) against tests/affine_trace_ref.py, the
full-matrix checker that tests/test_affine_trace_ref.py pins: byte equality of score, end cell, pos and both reversed consensus
strings (and with them begin_x and the CIGAR string) on known answers, whole problems on the exact path, three tile shapes of the
sweep path with planted gaps, the edges of the L17 window, options and repeated calls, the linear special case,
table scoring and the error codes.  Expected values are computed once per module."""
import ctypes as C

import numpy as np
import pytest

from tests import affine_trace_ref as tr, score_instances as si
from tests import test_gpu_affine as ga

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
FIELDS = ("score", "end_x", "end_y", "pos", "cons_x", "cons_y", "begin_x", "begin_y", "cigar")
KNOWN_CIGAR = ("12M3D12M", "12M3I12M")
SCORINGS = [(3, -3, 5, 1), (2, -1, 3, 1), (1, -1, 2, 2), (5, -4, 10, 3)]
N = "N" * 138                                                      # a letter no reference here has
SEED1, SEED2 = "GTTGGTGTTTGG", "TGGTTTGTGGTG"

_expected = {}


def expected(key, xs, y, sc=(3, -3, 5, 1), lut=None):
    """Checker results of the batch `xs` against y, computed once per key."""
    if key not in _expected:
        _expected[key] = tr.trace_batch(xs, y, *sc, lut=lut)
    return _expected[key]


def kw(sc, lut=None):
    return dict(match=float(sc[0]), mismatch=float(sc[1]), gap_open=float(sc[2]), gap_extend=float(sc[3]), lut=lut)


def rows(got):
    """The dict of arrays and lists of affine_batch_trace as one dict per query."""
    n = len(got["cons_x"])
    return [{k: (got[k][q] if isinstance(got[k], list) else got[k][q].item()) for k in FIELDS} for q in range(n)]


def mismatches(got, exp):
    return [(q, k, g[k], e[k]) for q, (g, e) in enumerate(zip(got, exp)) for k in FIELDS if g[k] != e[k]]


def check(got, exp):
    assert len(got) == len(exp)
    bad = mismatches(got, exp)
    assert not bad, bad[:4]


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def swept(path, prefix="affine["):
    """Whether the list of tags of Context.last_path names an instance of the affine sweep kernel, "affine[cell=...]"."""
    return any(t.startswith(prefix) for t in path)


def batch_trace(ctx, xs, y, sc=(3, -3, 5, 1), lut=None):
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    return rows(ctx.affine_batch_trace(**kw(sc, lut)))


# ---- known answers ----------------------------------------------------------------------------------------------------------------
def test_known_answers_single_and_batch(ctx):
    for (x, y, end), cig in zip(ga.KNOWN, KNOWN_CIGAR):
        for (go, ge), score in ga.KNOWN_SCORES.items():
            sc = (3, -3, go, ge)
            exp = expected(("known", x, go, ge), [x], y, sc)[0]
            assert (exp["score"], exp["end_x"], exp["end_y"], exp["begin_x"], exp["pos"], exp["cigar"]) == (float(score), end[0], end[1], 1, 5, cig)
            one = ctx.affine_align_trace(x, y, **kw(sc))
            assert "affine_exact" in ctx.last_path() and "affine_trace" in ctx.last_path()
            check([one], [exp])
            check(batch_trace(ctx, [x, x[3:], x], y, sc), [exp, expected(("known3", x, go, ge), [x[3:]], y, sc)[0], exp])


# ---- whole problems on the exact path ---------------------------------------------------------------------------------------------
def _exact_batches():
    """Twelve (queries, reference, scoring): 300 pairs, m in [1, 40], n in [1, 200], alphabets of 2 and 4 letters, some with a
    planted copy carrying a 3-column insert or a 2-row one."""
    rng = np.random.default_rng(20240)
    out = []
    for b in range(12):
        alpha = np.frombuffer(b"ACGT" if b % 2 == 0 else b"AC", dtype=np.uint8)
        n = (1, 200, 2, 199)[b] if b < 4 else int(rng.integers(3, 201))
        y = bytearray(alpha[rng.integers(0, len(alpha), n)].tobytes())
        xs = []
        for k in range(25):
            m = (1, 40)[k] if k < 2 else int(rng.integers(1, 41))
            x = alpha[rng.integers(0, len(alpha), m)].tobytes()
            if k % 4 == 2 and m >= 8 and n >= m + 3:
                at = int(rng.integers(0, n - m - 2))
                y[at:at + m + 3] = x[:m // 2] + alpha[rng.integers(0, len(alpha), 3)].tobytes() + x[m // 2:]
            elif k % 4 == 3 and m >= 10 and n >= m:
                at = int(rng.integers(0, n - m + 3))
                y[at:at + m - 2] = x[:m // 2] + x[m // 2 + 2:]
            xs.append(x)
        out.append((xs, bytes(y), SCORINGS[(b // 2) % 4]))
    return out


@pytest.mark.parametrize("b", range(12))
def test_whole_problems_exact(ctx, b):
    xs, y, sc = _exact_batches()[b]
    exp = expected(("exact", b), xs, y, sc)
    got = batch_trace(ctx, xs, y, sc)
    path = ctx.last_path()
    assert "affine_exact" in path and not swept(path), path
    check(got, exp)
    for k in (0, 7, 19):                                           # and one by one
        check([ctx.affine_align_trace(xs[k], y, **kw(sc))], [exp[k]])


# ---- the sweep path: three tile shapes, planted gaps ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 2), (8, 19), (16, 32)], ids=lambda s: "SL%d_R%d" % s)
def test_sweep_shapes(ctx, pgs, shape):
    c = ga.Case(pgs, shape, ga.SWEEP)
    assert c.L == shape[0] * shape[1]
    sc = (ga.SWEEP.match, ga.SWEEP.mismatch, ga.SWEEP.open, ga.SWEEP.ext)
    exp = expected(("sweep", shape), c.queries, c.ref, sc)
    opts = [("chunk", ga.CL)] + ([("slot", c.slot)] if c.slot else [])
    for k, v in opts:
        ctx.set_option(k, v)
    try:
        got = batch_trace(ctx, c.queries, c.ref, sc)
        path = ctx.last_path()
    finally:
        for k, _ in opts:
            ctx.set_option(k, 0)
    assert "affine[cell=f16,SL=%d,R=%d]" % shape in path and "affine_trace" in path, path
    check(got, exp)
    assert "3D" in got[0]["cigar"] and "3I" in got[2]["cigar"], (got[0]["cigar"], got[2]["cigar"])
    if c.gap70:
        assert "70D" in got[4]["cigar"], got[4]["cigar"]


# ---- edges of the traceback window ------------------------------------------------------------------------------------------------
def _edge_a(pgs):
    ref = pgs.synth.dna(8101, 2048).copy()
    mid = pgs.synth.read_from_ref(ref[500:1500], 8102, 150, sub_rate=0.04, indel_rate=0.03)[0]
    xs = [ref[:150].tobytes(), ref[-150:].tobytes(), b"G", b"N" * 150, mid.tobytes()]
    return xs, ref.tobytes()


def _edge_b():
    rng = np.random.default_rng(8103)
    y = bytearray(np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, 2600)].tobytes())
    y[300:312] = SEED1.encode()
    y[2000:2012] = SEED2.encode()
    return [(N + SEED1).encode(), (N + SEED2).encode()], bytes(y)


def _edge_c():
    q = list("AC" * 75)
    q[40] = "A"; q[41] = "A"; q[97] = "C"
    del q[120:123]
    q2 = "CA" * 40 + "AC" * 35
    return ["".join(q).encode(), q2.encode(), b"AC" * 75], b"AC" * 700


def test_window_edges_copies_single_row_and_no_match(ctx, pgs):
    xs, y = _edge_a(pgs)
    exp = expected("edge_a", xs, y)
    got = batch_trace(ctx, xs, y)
    path = ctx.last_path()
    assert swept(path, "affine[cell=f16,") and "affine_trace" in path, path
    check(got, exp)
    assert got[0]["pos"] == 1 and got[0]["cigar"] == "150M" and got[0]["end_y"] == 150          # clamped at the first column
    assert got[1]["end_y"] == 2048 and got[1]["cigar"] == "150M" and got[1]["pos"] == 2048 - 149
    assert (got[2]["score"], got[2]["cigar"], got[2]["end_x"]) == (3.0, "1M", 1)
    assert (got[3]["score"], got[3]["pos"], got[3]["cons_x"], got[3]["cons_y"], got[3]["cigar"], got[3]["begin_x"]) == (0.0, 0, "", "", "", 0)


def test_window_edges_seed_only(ctx):
    xs, y = _edge_b()
    exp = expected("edge_b", xs, y)
    # W = 150 + (3 * 150 - 36) + 2 = 566: clamped for the seed near column 300, unclamped for the one near column 2000
    assert [(e["score"], e["end_x"], e["end_y"]) for e in exp] == [(36.0, 150, 312), (36.0, 150, 2012)]
    got = batch_trace(ctx, xs, y)
    check(got, exp)
    assert [g["cigar"] for g in got] == ["12M", "12M"] and [g["begin_x"] for g in got] == [139, 139]


def test_window_edges_periodic_reference(ctx):
    xs, y = _edge_c()
    check(batch_trace(ctx, xs, y), expected("edge_c", xs, y))
    sc = (1, -1, 2, 2)
    check(batch_trace(ctx, xs, y, sc), expected("edge_c2", xs, y, sc))


# ---- options and repeats ----------------------------------------------------------------------------------------------------------
def test_no_affine_sweep_repeats_and_score_call(ctx, pgs):
    xs, y = _edge_a(pgs)
    exp = expected("edge_a", xs, y)
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    first = ctx.affine_batch_trace()
    second = ctx.affine_batch_trace()                              # the same scratch again
    check(rows(first), exp)
    check(rows(second), exp)
    plain = ctx.affine_batch_run()
    for k in ("score", "end_x", "end_y"):
        assert np.array_equal(plain[k], first[k]), k
    ctx.set_option("no_affine_sweep", 1)
    try:
        third = ctx.affine_batch_trace()
        path = ctx.last_path()
    finally:
        ctx.set_option("no_affine_sweep", 0)
    assert not swept(path) and "affine_exact" in path and "affine_trace" in path, path
    check(rows(third), exp)
    assert ctx.last_timings()["trace_us"] > 0                      # mi355_sw_last_timings [2]: the trace kernel


# ---- gap_open == gap_extend: the linear model ---------------------------------------------------------------------------------------
def test_linear_special_case(ctx, pgs):
    xs, y = _edge_a(pgs)
    sc = (3, -3, 2, 2)
    exp = expected("edge_a_linear", xs, y, sc)
    got = batch_trace(ctx, xs, y, sc)
    check(got, exp)
    lin = ctx.batch_run(match=3.0, mismatch=-3.0, gap=2.0, flags=pgs.capi.SCORE_ONLY)
    for g, l in zip(got, lin):
        assert (g["score"], g["end_x"], g["end_y"]) == (l["score"], l["end_x"], l["end_y"])
        assert tr.rescore(g["cons_x"], g["cons_y"], *sc) == g["score"]


# ---- table scoring ----------------------------------------------------------------------------------------------------------------
def test_table_scoring_exact_path(ctx):
    rng = np.random.default_rng(8104)
    aa = np.frombuffer(si.AA20, dtype=np.uint8)
    t = rng.integers(-4, 3, (20, 20))
    t = np.triu(t) + np.triu(t, 1).T
    t[np.arange(20), np.arange(20)] = rng.integers(3, 9, 20)
    lut = np.full((256, 256), -4.0, dtype=np.float32)
    lut[np.ix_(aa, aa)] = t
    y = bytearray(aa[rng.integers(0, 20, 700)].tobytes())
    xs = [aa[rng.integers(0, 20, m)].tobytes() for m in (1, 17, 60, 144, 144, 90)]
    y[100:160] = xs[2]
    y[300:380] = xs[3][:80]
    y[384:448] = xs[3][80:]                                         # a 4-column gap
    y[500:530] = xs[5][:30]
    y[530:585] = xs[5][35:]                                         # a 5-row gap
    y = bytes(y)
    sc = (0, 0, 11, 1)
    exp = expected("table", xs, y, sc, lut)
    got = batch_trace(ctx, xs, y, sc, lut)
    path = ctx.last_path()
    assert "affine_exact" in path and not swept(path), path
    check(got, exp)
    assert "D" in got[3]["cigar"] and "I" in got[5]["cigar"]


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, pgs):
    xs, y = _edge_a(pgs)
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    for bad in (dict(gap_open=1.0, gap_extend=2.0), dict(gap_open=3.0, gap_extend=0.0), dict(match=float("nan"))):
        for call in (lambda: ctx.affine_batch_trace(**bad), lambda: ctx.affine_align_trace(xs[0], y, **bad)):
            with pytest.raises(pgs.MI355Error) as e:
                call()
            assert e.value.code == EINVAL, bad
    for call in (lambda: ctx.affine_batch_trace(match=3.5, mismatch=-2.25), lambda: ctx.affine_align_trace(xs[0], y, gap_open=5.5)):
        with pytest.raises(pgs.MI355Error) as e:
            call()
        assert e.value.code == ENOTSUP and "integer" in str(e.value)
    # outside both paths: more than 512 rows (no sweep) and more than 2^26 cells (no whole problem on the exact kernel)
    long_ref = pgs.synth.dna(8105, 120_000).tobytes()
    with pytest.raises(pgs.MI355Error) as e:
        ctx.affine_align_trace(pgs.synth.dna(8106, 600).tobytes(), long_ref)
    assert e.value.code == ENOTSUP
    # a NULL result
    p, _ = pgs.capi.make_affine_params()
    L = ctx._L
    assert L.mi355_sw_affine_align_trace(ctx._ctx, xs[0], C.c_size_t(len(xs[0])), y, C.c_size_t(len(y)), C.byref(p), None) == EINVAL
    assert L.mi355_sw_affine_batch_trace(ctx._ctx, C.byref(p), None) == EINVAL
    # the context still works
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    check(rows(ctx.affine_batch_trace()), expected("edge_a", xs, y))
