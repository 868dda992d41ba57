"""Long database streams of the small-alignment batch cut into pieces (exact_full_device in csrc/host_batch.h; batch_wave_setup,
batch_seq_results, batch_window_setup in csrc/sw_batch_kernels.h; DESIGN.md §3.3 lemma L12): argmax cells around own-row boundaries,
lengths around the gate, ties across pieces and against whole sequences launched behind them, decision windows resumed inside a
piece, the longest chain L1 allows at zero rounding slack of the warm-up, pairs of pieces of different sequences in one slot of the
packed float16 pass, and the gates that turn pieces off.  Inputs, the restated piece table and the predicted counters:
tests/wave_pieces.py; their conditions, from the oracle alone: tests/test_wave_pieces_ref.py.

Every case runs under every route; every route asserts the same four things: all fields equal to the oracle's, bit for bit; the
devlist[...] tag the restated table predicts (no case passes on another kernel or with pieces silently off); counters left_window and
beyond_f16 equal to the module's prediction; and an ordinary align_batch on the same context afterwards still answers correctly."""
import numpy as np
import pytest

from tests import wave_pieces as wp

pytestmark = pytest.mark.gpu

FIELDS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
SCORE_FIELDS = ("score", "end_x", "end_y")
CASES = wp.all_cases()
# route -> (options, traceback, struct-of-arrays view); no_wave_window: the gate that takes pieces off with traceback (whole-problem decisions)
ROUTES = {"default": ((), True, False), "f32": (("no_wave_f16",), True, False), "score": ((), False, False),
          "scatter": (("no_devlist_by_id",), True, False), "nopieces": (("no_wave_pieces",), True, False),
          "nopieces_score": (("no_wave_pieces",), False, False), "nowindow": (("no_wave_window",), True, False),
          "view": ((), True, True)}


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


_expected, _piece_max = {}, {}


def expected(oracle, case):
    """The oracle's alignments of the case, computed once."""
    key = repr(case)
    if key not in _expected:
        m, x, g = case.scoring
        _expected[key] = [oracle.align(s, case.y, 0, m, x, g) for s in case.xs]
    return _expected[key]


def piece_max(oracle, case, t):
    """kk -> the oracle's maximum of problem kk of table t as a problem of its own, computed once per (sequence, rows)."""
    m, x, g = case.scoring

    def get(kk):
        p = t["problems"][kk]
        key = (repr(case), p["seq"], p["start"], p["rows"])
        if key not in _piece_max:
            _piece_max[key] = oracle.score_only(wp.piece_rows_of(t, case.xs[p["seq"]], kk), case.y, 0, m, x, g)
        return _piece_max[key]
    return get


def run(ctx, pgs, case, route):
    options, trace, view = ROUTES[route]
    m, x, g = case.scoring
    for o in options:
        ctx.set_option(o, 1)
    try:
        flags = 0 if trace else pgs.capi.SCORE_ONLY
        if view:
            ctx.set_reference(case.y)
            ctx.batch_upload(case.xs)
            arr = ctx.batch_run(semantics=0, match=m, mismatch=x, gap=g, flags=flags, raw=True)
            got = []
            for k in range(len(case.xs)):
                cx, cy = ctx.consensus(k)
                got.append(dict(score=float(arr["score"][k]), pos=int(arr["pos"][k]), end_x=int(arr["end_x"][k]), end_y=int(arr["end_y"][k]),
                                cons_x=cx, cons_y=cy))
        else:
            got = ctx.align_batch(case.xs, case.y, semantics=0, match=m, mismatch=x, gap=g, flags=flags)
        return got, ctx.last_path(), ctx.last_counters()
    finally:
        for o in options:
            ctx.set_option(o, None)


_after = {}


def still_answers(ctx, oracle):
    """An ordinary batch on the same context: the scratch the pieces used has not been left in a state that changes an answer."""
    if not _after:
        rng = np.random.default_rng(8999)
        y = wp.rand(rng, 144, wp.ALL_LETTERS)
        xs = [wp.rand(rng, n, wp.ALL_LETTERS) for n in (40, 200, 1500)] + [wp.rand(rng, 30, wp.ALL_LETTERS) + y[30:90] + wp.rand(rng, 50, wp.ALL_LETTERS)]
        _after.update(y=y, xs=xs, exp=[oracle.align(s, y, 0) for s in xs])
    got = ctx.align_batch(_after["xs"], _after["y"], semantics=0)
    bad = [(k, f, g[f], e[f]) for k, (g, e) in enumerate(zip(got, _after["exp"])) for f in FIELDS if g[f] != e[f]]
    assert not bad, ("afterwards", bad[:4])


def check(ctx, pgs, oracle, case, route):
    options, trace, view = ROUTES[route]
    exp = expected(oracle, case)
    t = case.table(trace=trace, options=options)
    left, beyond = wp.predict_counters(t, case.xs, case.y, exp, piece_max(oracle, case, t))
    got, path, cnt = run(ctx, pgs, case, route)
    print("%s %s: %s left_window %d (predicted %d) beyond_f16 %d (predicted %d)" % (case, route, t["tag"], cnt["left_window"], left, cnt["beyond_f16"], beyond))
    assert t["tag"] in path, (repr(case), route, t["tag"], path)
    keys = FIELDS if trace else SCORE_FIELDS
    bad = [(k, f, g[f], e[f]) for k, (g, e) in enumerate(zip(got, exp)) for f in keys if g[f] != e[f]]
    assert not bad, (repr(case), route, bad[:4])
    assert (cnt["left_window"], cnt["beyond_f16"]) == (left, beyond), (repr(case), route, cnt, left, beyond)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_pieces(ctx, pgs, oracle, case, route):
    check(ctx, pgs, oracle, case, route)
    still_answers(ctx, oracle)


def test_tables_differ_where_they_should():
    """The routes above are different launches: pieces on and off, float16 and float32 cells, windows and none (a table that predicted
    the same tag for all of them would assert nothing)."""
    c = next(c for c in CASES if c.name == "boundary" and c.ny == 144)
    tags = {r: c.table(trace=ROUTES[r][1], options=ROUTES[r][0])["tag"] for r in ROUTES}
    assert len({tags[r] for r in ("default", "f32", "score", "nopieces", "nopieces_score", "nowindow")}) == 6, tags
    assert "pieces=1" in tags["default"] and "pieces=0" in tags["nopieces"] and "pieces=0" in tags["nowindow"]
    assert all("pieces=0" in wp.boundary_case(*wp.GATE_OFF).table(trace=ROUTES[r][1], options=ROUTES[r][0])["tag"] for r in ROUTES)
