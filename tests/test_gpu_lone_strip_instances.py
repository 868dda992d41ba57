"""Raw maxima of the lone-query, twin and strip-mined sw_score_kernel instances, and of sw_long_kernel, against the oracle.

test_gpu_score_instances.py pins the two-query one-strip instances; this module pins the rest of kScoreInsts: the strip-mined tiles
(boundary rows in global memory, sub-chunk maxima folded over strips), the twin tiles (two tiles of ONE query in the halves of a
register), the one-query cells (kSemF32 / kSemF32U8 for a lone query) and, through align, the sampled lone-query instances.  As there,
Context.score_ranges returns the sweep's keys per (range, query) with no later correction; every case is built for ONE launch, checks
in Context.last_path() that this launch ran, and compares the whole array with oracle.score_only, exactly.  lone_strip_instances.py
holds the inputs (what is planted where, and why) and the host's choice restated.  test_every_planned_instance_ran, the last test,
compares what ran with the instances the header compiles beyond the other modules' (tests/test_lone_strip_instances_ref.py has the
partition)."""
import numpy as np
import pytest

import lone_strip_instances as ls
import score_instances as si
from score_instances import F32, U8SAT

KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
SEMS = ls.sems_in_header()

RAN = {}             # kScoreInsts tuple -> cases that ran on it
PLANNED = set()
RAN_LONG = set()     # (R, p32, groups > 1, sampled, unsat) of sw_long_kernel launches
_CASES = {}


def _cached(case, oracle, pool):
    case = _CASES.setdefault(case.key(), case)
    case.compute(oracle, pool)
    return case


def _context(pgs, options):
    c = pgs.Context(0)
    for o in options:
        c.set_option(o, True)
    return c


def _report(failures):
    assert not failures, "%d findings:\n%s" % (len(failures), "\n".join(failures[:60]))


def _tags(ctx):
    path = ctx.last_path()
    return si.parse_path(path), ls.parse_long(path)


def _check_launch(ctx, want, what, failures, sampled=0):
    """Every sweep of the call ran the launch the case was built for; returns the launch's tags, or None."""
    score, long_ = _tags(ctx)
    keys = {ls.tag_key(t) for t in score} | {ls.tag_key(t) for t in long_}
    if keys != {ls.tag_key(want)}:
        failures.append("%s: built for %s, ran %s" % (what, ls.tag_name(ls.tag_key(want)), ", ".join(ls.tag_name(k) for k in sorted(keys)) or "no sweep"))
        return None
    tags = long_ if want.get("long") else score
    if any(int(t.get("sampled", 0)) != sampled for t in tags):
        failures.append("%s: sampled != %d in %r" % (what, sampled, tags))
        return None
    if want.get("long") and not sampled and any(t["opt_margin"] != 0 for t in tags):
        failures.append("%s: score_ranges swept with an optimistic margin, its maxima are not raw: %r" % (what, tags))
        return None
    if want.get("long"):
        RAN_LONG.update((t["R"], t["p32"], int(t["groups"] > 1), t["sampled"], t["unsat"]) for t in tags)
    else:
        RAN.setdefault(ls.instance_of(ls.tag_key(want), sampled, SEMS), []).append(what)
    return tags


def _plan(want, sampled=0):
    if not want.get("long"):
        PLANNED.add(ls.instance_of(ls.tag_key(want), sampled, SEMS))


def _sweep(pgs, oracle, pool, ctx, make_case, first_chunk, want, what, failures, check_inputs=True):
    """score_ranges of the case built for the tile length the host chose, against the oracle on every (range, query)."""
    _plan(want)
    chunk = first_chunk
    for attempt in range(3):
        case = make_case(chunk)
        ctx.set_reference(case.ref)
        ctx.batch_upload(case.queries)
        got = ctx.score_ranges(case.ranges, semantics=case.sem, **case.sc.kw())
        ki = ctx.last_kernel()
        actual = int(ki["chunk_len"])
        if actual == chunk:
            break
        chunk = actual                                   # the ranges are cut relative to the tile length: build them for the real one
    else:
        failures.append("%s: the tile length did not settle (%d)" % (what, actual))
        return None
    case = _cached(case, oracle, pool)
    failures.extend("%s: geometry: %s" % (what, f) for f in case.geometry_faults())
    if check_inputs:
        failures.extend("%s: input: %s" % (what, f) for f in case.input_faults())
    if _check_launch(ctx, want, what, failures) is None:
        return None
    exp = case.expected
    assert got.shape == exp.shape
    for r, k in zip(*np.nonzero(got != exp)):
        failures.append("%s: tile length %d, range %s [%d, %d) (%d tiles) query %d (%d rows): kernel %g, oracle %g" % (
            what, chunk, case.names[r] if hasattr(case, "names") else case.NAMES[r], case.ranges[r][0], case.ranges[r][1], case.tiles(r), k,
            len(case.queries[k]), got[r, k], exp[r, k]))
    return case, ki


# ---- a lone query in one strip: twin tiles, one-query cells --------------------------------------------------------------------------
def _run_lone(pgs, oracle, pool, ctx, options, sem, failures, L, sc, expect, slot=0, chunk_opt=0, one_letter=False, one_tile=False,
              check_inputs=True):
    want = ls.predicted_lone(L, sem, sc, options, ls.ncodes(sc), 1024, slot)
    assert ls.matches(want, expect), (L, sc.name, options, want, expect)
    per_wg = (256 // want["SL"]) * (2 if want["twin"] or want["SL"] == 64 else 1)       # (64 lanes: twin or not, one input)
    what = "lone %d rows %s %s%s%s" % (L, "u8" if sem == U8SAT else "f32", sc.name, " one letter" if one_letter else "", " one tile" if one_tile else "")
    ctx.set_option("slot", slot)
    ctx.set_option("chunk", chunk_opt)
    try:
        make = lambda cl: ls.LoneCase(pgs, L, sem, sc, cl, per_wg, one_letter=one_letter, one_tile=one_tile)
        out = _sweep(pgs, oracle, pool, ctx, make, chunk_opt or max(128, si.pow2_at_least(L, 128)), want, what, failures, check_inputs)
    finally:
        ctx.set_option("chunk", 0)
        ctx.set_option("slot", 0)
    if out is not None:
        case, ki = out
        sub = ls.sub_len_of(sem, 1, L, want, case.chunk)
        if int(ki["sub_len"]) != sub:
            failures.append("%s: sub-chunks of %d columns, expected %d" % (what, int(ki["sub_len"]), sub))


@pytest.mark.gpu
@pytest.mark.parametrize("sem,name,options", ls.LONE_SHORT, ids=ls.route_ids(ls.LONE_SHORT))
def test_lone_short(pgs, oracle, sem, name, options):
    """One query of up to 512 rows: by default two of its TILES per packed float16 register on 16-lane tiles, with the code-pair profile
    (no_comb: without); no_twin: float32 cells on the 8- and 16-lane shape of its length; the uint8 engine the same, unsaturated, and
    under no_unsat its float32 cell.  A float-engine lone short query reports per 64-column sub-chunk."""
    failures = []
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for run in ls.lone_short_runs(sem, name, options):
                _run_lone(pgs, oracle, pool, ctx, options, sem, failures, **run)
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("sem,name,options,cell,twin,unsat", ls.LONE_WIDE, ids=ls.route_ids(ls.LONE_WIDE))
def test_lone_wide(pgs, oracle, sem, name, options, cell, twin, unsat):
    """One query of 513 .. 2048 rows on every kR64 shape: float32 cells (long_twin: two tiles per packed int16 register); the uint8
    engine unsaturated on float32 cells, and down its ladder of options to the saturating float32 cell."""
    failures = []
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for run in ls.lone_wide_runs(sem, name, options, cell, twin, unsat):
                _run_lone(pgs, oracle, pool, ctx, options, sem, failures, **run)
    finally:
        ctx.close()
    _report(failures)


# ---- strip-mined tiles ---------------------------------------------------------------------------------------------------------------------
def _run_strips(pgs, oracle, pool, ctx, options, sem, failures, shape, lens, sc, expect, strip_r=0, chunk_opt=0, check_inputs=True, min_subs=1, long_r=0):
    nmin = ls.strip_min_cols(sem, max(lens))
    want = ls.predicted_bucket(len(lens), max(lens), sem, sc, options, ls.ncodes(sc), nmin, 0, strip_r, long_r=long_r)
    what = "strips %r %r rows %s %s" % (shape, tuple(lens), "u8" if sem == U8SAT else "f32", sc.name)
    assert ls.matches(want, expect), (what, options, want, expect)
    if not want.get("long"):
        assert (want["SL"], want["R"], want["strips"]) == shape + (1,), (what, want)
        for m in lens:
            assert ls.bucket_shape(m, ls.ncodes(sc), set(options), 0, strip_r) == shape + (True,), (what, m)
    assert ls.fast_ok(max(lens), sem, sc, want, ls.ncodes(sc), nmin) and (want.get("long") or not ls.fast_ok(max(lens), sem, sc, want, ls.ncodes(sc), 4095)), what
    ctx.set_option("strip_r", strip_r)
    ctx.set_option("chunk", chunk_opt)
    try:
        make = lambda cl: ls.StripCase(pgs, shape, lens, sem, sc, cl)
        out = _sweep(pgs, oracle, pool, ctx, make, chunk_opt or 4096, want, what, failures, check_inputs)
    finally:
        ctx.set_option("strip_r", 0)
        ctx.set_option("chunk", 0)
    if out is not None and not want.get("long"):
        case, ki = out
        sub = ls.sub_len_of(sem, len(lens), max(lens), want, case.chunk)
        if int(ki["sub_len"]) != sub:
            failures.append("%s: sub-chunks of %d columns, expected %d" % (what, int(ki["sub_len"]), sub))
        if case.chunk // sub < min_subs:
            failures.append("%s: tiles of %d sub-chunks of %d columns, the case wants %d" % (what, case.chunk // sub, sub, min_subs))
        return case.chunk // sub
    return 0


@pytest.mark.gpu
@pytest.mark.parametrize("sem,name,options,cell,unsat", ls.BATCH_STRIPS, ids=ls.route_ids(ls.BATCH_STRIPS))
def test_batch_strips(pgs, oracle, sem, name, options, cell, unsat):
    """Three reads beyond 2048 rows (two strips, three with ONE row in the last, three full strips) on every kR64S shape, and beyond 512
    rows on a 20-letter alphabet on the kR16S shape."""
    failures = []
    subs = []                                                           # sub-chunks per tile of this variant's cases
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for run in ls.batch_strip_runs(sem, name, options, cell, unsat):
                subs.append(_run_strips(pgs, oracle, pool, ctx, options, sem, failures, **run))
    finally:
        ctx.close()
    if not failures:
        assert (64 if sem == F32 else 2) in subs, "no strip case of this variant had tiles of %d sub-chunks: %r" % (64 if sem == F32 else 2, subs)
    _report(failures)


@pytest.mark.gpu
def test_no_wide_strips(pgs, oracle):
    """Option no_wide sends DNA reads beyond 512 rows to the kR16S shape too."""
    failures = []
    ctx = _context(pgs, ("no_wide",))
    try:
        with si.make_pool() as pool:
            _run_strips(pgs, oracle, pool, ctx, ("no_wide",), F32, failures, (16, 32), ls.strip_lengths(16, 32), ls.strip_sc(F32),
                        dict(cell="i16", SL=16, R=32, strips=1))
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("sem,name,options,cell,twin,unsat", ls.LONE_STRIPS, ids=ls.route_ids(ls.LONE_STRIPS))
def test_lone_strips(pgs, oracle, sem, name, options, cell, twin, unsat):
    """One query beyond 2048 rows kept off sw_long_kernel, on every kR64S shape by its length alone; and (without twin tiles) one beyond
    512 rows on a 20-letter alphabet on the kR16S shape: float32 cells there, the uint8 engine's saturating float32 cell with no option."""
    failures = []
    with si.make_pool() as pool:
        for run in ls.lone_strip_runs(sem, name, options, cell, twin, unsat):
            run = dict(run)
            opts = run.pop("options", options)
            ctx = _context(pgs, opts)
            try:
                _run_strips(pgs, oracle, pool, ctx, opts, sem, failures, **run)
            finally:
                ctx.close()
    _report(failures)


# ---- sw_long_kernel: its per-range maxima are raw too -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_long_kernel(pgs, oracle):
    """A lone query beyond 2048 rows by default: sw_long_kernel<R, 1> with R = 20 / 24 / 32 by length and by long_r, float32 and float16
    profile, one and two workgroups per tile; the uint8 engine's unsaturated sweep on it.  (Its workgroups wait for each other: a test
    of its own.)"""
    failures = []
    with si.make_pool() as pool:
        for sem, options, ints, p32, groups in ls.LONG_VARIANTS:
            ctx = _context(pgs, options)
            try:
                for r, m, int_options, sc, check_inputs in ls.long_runs(sem, options, ints):
                    before = set(RAN_LONG)
                    RAN_LONG.clear()
                    for k, v in int_options:
                        ctx.set_option(k, v)
                    try:
                        _run_strips(pgs, oracle, pool, ctx, options, sem, failures, (64, r), (m,), sc,
                                    dict(long=1, unsat=int(sem == U8SAT), R=r), long_r=dict(int_options).get("long_r", 0), check_inputs=check_inputs)
                    finally:
                        for k, v in int_options:
                            ctx.set_option(k, 0)
                    ran = set(RAN_LONG)
                    RAN_LONG.update(before)
                    if ran and ran != {(r, p32, groups, 0, int(sem == U8SAT))}:
                        failures.append("long kernel %d rows %r %r: ran (R, p32, groups > 1, sampled, unsat) = %r, expected R=%d p32=%d groups>1=%d" % (
                            m, options, int_options, sorted(ran), r, p32, groups))
            finally:
                ctx.close()
    _report(failures)


# ---- the sampled lone-query instances ------------------------------------------------------------------------------------------------------
def _run_sampled(pgs, oracle, ctx, case, want, what, failures):
    """align of the case's query over its whole reference: sampled=1, every field the oracle's, no second sweep."""
    q, sc = case.queries[-1], case.sc
    _plan(want, 1)
    res = ctx.align(q, case.ref, semantics=case.sem, **sc.kw())
    counters = ctx.last_counters()
    if _check_launch(ctx, want, what, failures, sampled=1) is None:
        return
    if counters["whole_batch_again"] != 0 or counters["requeried"] != 0:
        failures.append("%s: fell back: whole_batch_again %d, requeried %d (candidates %d)" % (
            what, counters["whole_batch_again"], counters["requeried"], counters["candidates"]))
    exp = oracle.align(q, case.ref, case.sem, **sc.kw())
    for f in KEYS:
        if res[f] != exp[f]:
            failures.append("%s: %s %r, oracle %r" % (what, f, res[f], exp[f]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,options", ls.SAMPLED, ids=[v[0] for v in ls.SAMPLED])
def test_sampled_lone(pgs, oracle, name, options):
    """The MK = 4 float32 instances of a lone query (kR16M x 64 lanes in one strip; kR64S strips under no_long) and sw_long_kernel<R, 8>
    through align: sampled=1 in the path, results equal to the oracle's in every field, and no second sweep.  A lone query may have
    1088 candidate sub-chunks; these references hold fewer, so a sweep that under-reports fails instead of costing a second sweep."""
    failures = []
    ctx = _context(pgs, options)
    try:
        for kind, v, expect in ls.sampled_runs(name):
            if kind == "lone":
                rows, case = v, ls.LoneCase(pgs, v, F32, si.GAP_ABOVE_MATCH, si.pow2_at_least(v), 2)   # (a short F: the oracle's traceback pays per cell)
            else:
                rows = ls.natural_strip_length(v)
                case = ls.StripCase(pgs, (64, v), (rows,), F32, si.GAP_ABOVE_MATCH, 4096)
            sub = si.pow2_at_least(rows) if kind == "lone" else 64          # (strips: 1/64 of a tile of at least 4096 columns)
            assert -(-len(case.ref) // sub) < 1088, "the reference holds more sub-chunks than a lone query's candidate budget"
            want = ls.predicted_lone(rows, F32, case.sc, options, 5, len(case.ref), allow_sample=True)
            assert ls.matches(want, expect), (want, expect)
            _run_sampled(pgs, oracle, ctx, case, want, "sampled %s %d rows" % (name, rows), failures)
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("name,options", ls.SAMPLED_MIRROR, ids=[v[0] for v in ls.SAMPLED_MIRROR])
def test_sampled_mirrored_tall(pgs, oracle, name, options):
    """The MK = 4 mirrored instances on 16 x 24 and 16 x 32: mirror_ok admits reads of 384 and 512 rows only below match 3, so the sampled
    sweeps of test_gpu_score_instances.py (3 / -3 / 2) never reach them.  As there, through align_batch of that module's batch over its
    whole reference, at 1 / -1 / 4: sampled=1, results equal to the oracle's in every field, no second sweep; the reference holds fewer
    sub-chunks than a query's candidate budget."""
    failures = []
    sc = si.GAP_ABOVE_MATCH
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for shape in ls.SAMPLED_MIRROR_SHAPES:
                L = shape[0] * shape[1]
                want = ls.sampled_mirror_want(shape, options)
                assert ls.matches(want, dict(cell="f16", mirror=1, idiag=int(name == "f16m"))), want
                what = "sampled mirrored %r %s" % (shape, name)
                case = si.Case(pgs, shape, F32, sc, si.nominal_chunk(L, F32))
                assert -(-len(case.ref) // si.nominal_chunk(L, F32)) < 64 + 1024 // len(case.queries)
                exp = list(pool.map(lambda q: oracle.align(q, case.ref, F32, **sc.kw()), case.queries))
                _plan(want, 1)
                res = ctx.align_batch(case.queries, case.ref, semantics=F32, **sc.kw())
                counters = ctx.last_counters()
                if _check_launch(ctx, want, what, failures, sampled=1) is None:
                    continue
                if counters["whole_batch_again"] != 0 or counters["requeried"] != 0:
                    failures.append("%s: fell back: whole_batch_again %d, requeried %d (candidates %d)" % (
                        what, counters["whole_batch_again"], counters["requeried"], counters["candidates"]))
                for k, (got, e) in enumerate(zip(res, exp)):
                    for f in KEYS:
                        if got[f] != e[f]:
                            failures.append("%s: query %d (%s): %s %r, oracle %r" % (what, k, si.QUERY_NAMES[k], f, got[f], e[f]))
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
def test_every_planned_instance_ran():
    """Last: what ran equals what was planned, the plan is the one the CPU module partitions the header's table with, and every
    sw_long_kernel layout of the routes ran."""
    insts, _ = ls.instances_in_header()
    mine = {i for i in insts if ls.classify(i, SEMS) == "c"}
    missing = sorted(mine - set(RAN))
    assert not missing, "compiled, this module's, and never ran: %r" % missing
    assert set(RAN) == PLANNED, "ran and planned differ: %r" % sorted(set(RAN) ^ PLANNED)
    assert PLANNED == set(ls.plan()), "planned here and in lone_strip_instances.plan() differ: %r" % sorted(PLANNED ^ set(ls.plan()))
    for r in (20, 24, 32):
        for combo in ((r, 1, 0, 0, 0), (r, 0, 0, 0, 0), (r, 1, 1, 0, 0), (r, 1, 0, 0, 1)):
            assert combo in RAN_LONG, "sw_long_kernel (R, p32, groups > 1, sampled, unsat) = %r never ran: %r" % (combo, sorted(RAN_LONG))
        assert any(t[0] == r and t[3] == 1 for t in RAN_LONG), "sw_long_kernel<%d, 8> never ran" % r
    print("\n%d sw_score_kernel instances (%d of them this module's own), %d sw_long_kernel layouts" % (len(RAN), len(mine), len(RAN_LONG)))
