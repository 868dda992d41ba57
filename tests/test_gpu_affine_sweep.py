"""The affine sweep (sw_affine_kernel with affine_run / affine_sweep_launch) beyond its smallest configuration, on the inputs of
tests/affine_sweep_cases.py (what is planted where, and the two mutations they are built against, is said there; its conditions are
checked without a GPU by tests/test_affine_sweep_cases_ref.py): tiles in the second and third workgroup of a range, end cells at
every offset around a sub-chunk and a tile boundary, ties, buckets of one call that go different ways, and more ranges than a launch
group holds.  Every case goes through Context as tests/test_gpu_affine.py does, compares exactly with tests/affine_ref.py and
asserts the geometry it was built for: the instance tag in last_path() and chunk_len / sub_len of last_kernel()."""
import contextlib

import numpy as np
import pytest

from tests import affine_sweep_cases as sc, score_instances as si
from tests.test_gpu_affine import SWEEP, Scoring

pytestmark = pytest.mark.gpu

ids = lambda s: "SL%d_R%d" % s


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, **opts):
    """Context options set for the block and reset to 0 afterwards; a value of 0 / None is left out."""
    opts = {k: v for k, v in opts.items() if v}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            ctx.set_option(k, 0)


def tag_of(shape):
    return "affine[cell=f16,SL=%d,R=%d]" % shape


def sweep_tags(path):
    return [t for t in path if t.startswith("affine[")]


def geometry(ctx):
    k = ctx.last_kernel()
    return (k["lanes"], k["rows_per_lane"]), k["chunk_len"], k["sub_len"]


def triple(r):
    return (float(r["score"]), int(r["end_x"]), int(r["end_y"]))


def triples(got):
    return [(float(s), int(i), int(j)) for s, i, j in zip(got["score"], got["end_x"], got["end_y"])]


def expected_triples(exp):
    return [(float(s), int(i), int(j)) for s, i, j in zip(*exp)]


# ---- A: tiles beyond the first workgroup (cg >= 1) -----------------------------------------------------------------------------
def run_workgroup_case(ctx, c):
    with options(ctx, chunk=sc.CL, slot=c.slot):
        ctx.set_reference(c.ref)
        ctx.batch_upload(c.queries)
        mx = ctx.affine_score_ranges(c.ranges, **SWEEP.kw())
        p1, g1 = ctx.last_path(), geometry(ctx)
        got = ctx.affine_batch_run(**SWEEP.kw())
        p2, g2 = ctx.last_path(), geometry(ctx)
    return mx, got, (p1, g1), (p2, g2)


@pytest.mark.parametrize("shape", sc.WORKGROUP_SHAPES, ids=ids)
def test_tiles_beyond_the_first_workgroup(ctx, pgs, shape):
    c = sc.workgroup_case(pgs, shape)
    emx, whole = c.compute()
    mx, got, (p1, g1), (p2, g2) = run_workgroup_case(ctx, c)
    longest = max(b - a for a, b in c.ranges)
    cl, sl = c.geometry(longest)[:2]
    assert tag_of(shape) in p1 and tag_of(shape) in p2, (p1, p2)
    assert g1 == (shape, cl, sl) and g2 == (shape, cl, sl), (g1, g2)
    assert sc.tiles(longest, g1[1]) > 2 * sc.nslot(shape[0]) and sc.tiles(len(c.ref), g2[1]) > 2 * sc.nslot(shape[0])
    assert np.array_equal(mx.astype(np.float64), emx), (shape, mx.tolist(), emx.tolist())
    assert triples(got) == expected_triples(whole), (shape, triples(got), expected_triples(whole))


def test_tie_across_workgroups_in_a_batch(ctx, pgs):
    """Case A's query 4 on 16 x 2: equal maxima in the first and the third workgroup of the range; the first is the end cell."""
    c = sc.workgroup_case(pgs, sc.TIE_SHAPE)
    N = sc.nslot(sc.TIE_SHAPE[0])
    assert [sc.tile_of(e, sc.CL) // N for e in c.q4_ends] == [0, 2]
    mx, got, (p1, g1), _ = run_workgroup_case(ctx, c)
    assert g1[1:] == (sc.CL, sc.CL) and tag_of(sc.TIE_SHAPE) in p1
    assert mx[0, 4] == sc.MATCH * c.L and triples(got)[4] == (sc.MATCH * c.L, c.L, c.q4_end_whole) == expected_triples(c.compute()[1])[4]


# ---- B: the end column around every cut ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.CUT_SHAPES, ids=ids)
def test_end_cell_around_cuts_batch(ctx, pgs, shape):
    cl, sl = sc.BATCH_GEOMETRY
    bad = []
    with options(ctx, chunk=cl):
        for d in sc.CUT_OFFSETS:
            c = sc.cut_case(pgs, shape, d)
            ctx.set_reference(c.ref)
            ctx.batch_upload(c.queries)
            got = ctx.affine_batch_run(**SWEEP.kw())
            assert tag_of(shape) in ctx.last_path() and geometry(ctx) == (shape, cl, sl), (d, ctx.last_path(), geometry(ctx))
            exp = expected_triples(c.compute())
            bad += [(d, k, c.ends[k], g, e) for k, (g, e) in enumerate(zip(triples(got), exp)) if g != e]
    assert not bad, bad


@pytest.mark.parametrize("chunk", [sc.CL, None], ids=["chunk256", "chunk_as_picked"])
@pytest.mark.parametrize("shape", sc.CUT_SHAPES, ids=ids)
def test_end_cell_around_cuts_lone(ctx, pgs, shape, chunk):
    bad, picked = [], set()
    with options(ctx, chunk=chunk):
        for d in sc.CUT_OFFSETS:
            c = sc.cut_case(pgs, shape, d)
            exp = expected_triples(c.compute())
            for k, x in enumerate(c.queries):
                got = triple(ctx.affine_align(x, c.ref, **SWEEP.kw()))
                g = geometry(ctx)
                assert tag_of(shape) in ctx.last_path() and g[0] == shape and g[2] == sc.KSEG, (d, k, ctx.last_path(), g)
                if chunk:
                    assert g[1] == chunk, (d, k, g)
                picked.add(g[1])
                if got != exp[k]:
                    bad.append((d, k, c.ends[k], got, exp[k]))
    assert not bad, ("tile lengths of the calls: %s" % sorted(picked), bad)


# ---- C: ties -------------------------------------------------------------------------------------------------------------------
def test_ties_batch(ctx, pgs):
    c = sc.tie_case(pgs, "batch")
    cl, sl = c.geometry
    with options(ctx, chunk=cl):
        ctx.set_reference(c.ref)
        ctx.batch_upload(c.queries)
        got = ctx.affine_batch_run(**SWEEP.kw())
        assert tag_of(sc.TIE_SHAPE) in ctx.last_path() and geometry(ctx) == (sc.TIE_SHAPE, cl, sl), (ctx.last_path(), geometry(ctx))
    exp = expected_triples(c.compute())
    assert triples(got) == exp, [(n, g, e) for n, g, e in zip(c.names, triples(got), exp) if g != e]


def test_ties_lone(ctx, pgs):
    c = sc.tie_case(pgs, "lone")
    cl, sl = c.geometry
    exp = expected_triples(c.compute())
    bad = []
    with options(ctx, chunk=cl):
        for k, x in enumerate(c.queries):
            got = triple(ctx.affine_align(x, c.ref, **SWEEP.kw()))
            assert tag_of(sc.TIE_SHAPE) in ctx.last_path() and geometry(ctx) == (sc.TIE_SHAPE, cl, sl), (k, ctx.last_path(), geometry(ctx))
            if got != exp[k]:
                bad.append((c.names[k], got, exp[k]))
    assert sc.tiles(c.n, cl) > sc.nslot(sc.TIE_SHAPE[0])             # two workgroups
    assert not bad, bad


# ---- D: mixed dispatch in one call ---------------------------------------------------------------------------------------------
def run_mixed(ctx, ref, qs, scoring):
    """(batch result, path, geometry) and (maxima over the whole reference as one range, path) under option chunk = CL."""
    with options(ctx, chunk=sc.CL):
        ctx.set_reference(ref)
        ctx.batch_upload(qs)
        got = ctx.affine_batch_run(**scoring.kw())
        p1, g1 = ctx.last_path(), geometry(ctx)
        mx = ctx.affine_score_ranges([(0, len(ref))], **scoring.kw())
        p2 = ctx.last_path()
    return (got, p1, g1), (mx, p2)


def check_mixed(got, mx, exp):
    assert triples(got) == expected_triples(exp), (triples(got), expected_triples(exp))
    assert np.array_equal(mx.astype(np.float64)[0], exp[0]), (mx.tolist(), exp[0].tolist())


def test_float16_bound_per_bucket(ctx, pgs):
    ref, qs, exp = sc.bound_mix(pgs)
    ma, mi, go, ge, _ = sc.BOUND_SCORING
    (got, p1, g1), (mx, p2) = run_mixed(ctx, ref, qs, Scoring("8/-5/6/2", ma, mi, go, ge))
    fast, slow = si.pick_shape(100), si.pick_shape(300)
    for p in (p1, p2):
        assert sweep_tags(p) == [tag_of(fast)] and "affine_exact" in p, p     # the bucket of 300 rows is beyond the bound
    assert g1 == (fast, sc.CL, sc.sub_len(3, 100, sc.CL)) and tag_of(slow) not in p1
    check_mixed(got, mx, exp)


def test_long_and_empty_queries_beside_short_ones(ctx, pgs):
    ref, qs, exp = sc.long_and_empty(pgs)
    (got, p1, g1), (mx, p2) = run_mixed(ctx, ref, qs, SWEEP)
    fast = si.pick_shape(150)
    for p in (p1, p2):
        assert sweep_tags(p) == [tag_of(fast)] and "affine_exact" in p, p
    assert g1 == (fast, sc.CL, sc.sub_len(2, 150, sc.CL))
    assert triples(got)[2] == (0.0, 0, 0) and mx[0, 2] == 0.0
    check_mixed(got, mx, exp)


@pytest.mark.parametrize("gap_open", [2040, 2041])
def test_gap_open_across_the_float16_bound(ctx, pgs, gap_open):
    ref, qs, exp = sc.gap_open_bound(pgs, gap_open)
    (got, p1, g1), (mx, p2) = run_mixed(ctx, ref, qs, Scoring("3/-3/%d/1" % gap_open, 3, -3, gap_open, 1))
    for p in (p1, p2):
        assert sweep_tags(p) == ([tag_of(si.pick_shape(150))] if gap_open <= 2040 else []), (gap_open, p)
    if gap_open <= 2040:
        assert g1 == (si.pick_shape(150), sc.CL, sc.sub_len(3, 150, sc.CL))
    check_mixed(got, mx, exp)


# ---- E: more than 32 768 ranges ------------------------------------------------------------------------------------------------
def test_more_ranges_than_a_launch_group(ctx, pgs):
    c = sc.many_ranges(pgs)
    seven, every = c.compute()
    with options(ctx, chunk=sc.CL):
        ctx.set_reference(c.ref)
        ctx.batch_upload(c.queries)
        mx = ctx.affine_score_ranges(c.ranges, **SWEEP.kw())
        path, g = ctx.last_path(), geometry(ctx)
    assert tag_of((16, 2)) in path and g == ((16, 2), sc.CL, sc.sub_len(4, 32, sc.CL)), (path, g)
    assert mx.shape == every.shape == (sc.GROUP + 3, 4)
    wrong = np.flatnonzero((mx.astype(np.float64) != every).any(axis=1))
    assert wrong.size == 0, (wrong.size, wrong[:8].tolist(), mx[wrong[:8]].tolist(), every[wrong[:8]].tolist())
