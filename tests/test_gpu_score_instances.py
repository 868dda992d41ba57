"""Raw maxima of every two-query sw_score_kernel instance against the oracle.

Context.score_ranges returns the kernel's keys per (range, query) with no later correction, so every tile's value is seen, not only
the winner's.  Each case here is built for ONE instance (cell, SL, R, mirror, idiag, unsat), checks in Context.last_path() that this
instance ran, and compares the whole [nranges, nq] array with oracle.score_only, exactly.  score_instances.py holds the inputs (what
is planted where, and why) and the host's choice of shape and cell restated from the same inequalities.

Shapes that pick_shape never selects on its own (they lose every tie against an 8-lane shape of the same height) and that are
reached with the context option slot=16:   16 lanes x 8 rows (ties with 8 x 16),   16 lanes x 16 rows (ties with 8 x 32).
Every other 8-lane, 16-lane and one-strip whole-wavefront shape is reached by query length alone.

The sampled instances (MK = 4) cannot be seen through score_ranges; test_sampled_instances runs them through align_batch and demands
exact results with no second sweep.  test_every_instance_ran, the last test, compares what ran with what was planned.
"""
import numpy as np
import pytest

import score_instances as si
from score_instances import F32, U8SAT

KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")

RAN = {}             # instance key -> cases that ran on it (score_ranges: MK = 1)
PLANNED = set()      # instance keys the cases were built for
RAN_SAMPLED = {}     # the same for the sampled sweeps of align_batch
PLANNED_SAMPLED = set()
_CASES = {}


def _case(pgs, oracle, pool, shape, sem, sc, chunk):
    c = si.Case(pgs, shape, sem, sc, chunk)
    c = _CASES.setdefault(c.key(), c)
    c.compute(oracle, pool)
    return c


def _context(pgs, options):
    c = pgs.Context(0)
    for o in options:
        c.set_option(o, True)
    return c


def _check_tags(tags, want, what, failures):
    """Every score launch of the call ran the instance the case was built for."""
    keys = {si.instance_key(t) for t in tags}
    if keys != {si.instance_key(want)}:
        failures.append("%s: built for %s, ran %s" % (what, si.instance_name(si.instance_key(want)),
                                                      ", ".join(si.instance_name(k) for k in sorted(keys)) or "no score kernel"))
        return False
    return True


def _run_case(pgs, oracle, pool, ctx, shape, sem, sc, want, failures, check_inputs=True):
    """One shape under one context: score_ranges against the oracle on every (range, query)."""
    lens, slot = si.shape_lengths(shape)
    assert lens, "no query length reaches shape %r" % (shape,)
    what = "%s %s %s" % (si.instance_name(si.instance_key(want)), "u8" if sem == U8SAT else "f32", sc.name)
    ctx.set_option("slot", slot)
    chunk = si.nominal_chunk(lens[-1], sem)
    for attempt in range(3):
        case = _case(pgs, oracle, pool, shape, sem, sc, chunk)
        ctx.set_reference(case.ref)
        ctx.batch_upload(case.queries)
        got = ctx.score_ranges(case.ranges, semantics=sem, **sc.kw())
        tags = si.parse_path(ctx.last_path())
        actual = int(ctx.last_kernel()["chunk_len"])
        if actual == chunk:
            break
        chunk = actual                                   # the ranges are cut relative to the tile length: build them for the real one
    else:
        failures.append("%s: the tile length did not settle (%d)" % (what, actual))
        return
    PLANNED.add(si.instance_key(want))
    if check_inputs:
        failures.extend("%s: input: %s" % (what, f) for f in case.input_faults())
    if not _check_tags(tags, want, what, failures):
        return
    RAN.setdefault(si.instance_key(want), []).append(what)
    exp = case.expected
    assert got.shape == exp.shape
    for r, k in zip(*np.nonzero(got != exp)):
        failures.append("%s: range %s [%d, %d) query %d (%s, %d rows, %s half): kernel %g, oracle %g" % (
            what, si.RANGE_NAMES[r], case.ranges[r][0], case.ranges[r][1], k, si.QUERY_NAMES[k], len(case.queries[k]),
            "odd / high" if case.half[k] else "even / low", got[r, k], exp[r, k]))


def _report(failures):
    assert not failures, "%d findings:\n%s" % (len(failures), "\n".join(failures[:60]))


# ---- CPU: the lists and the inputs -----------------------------------------------------------------------------------------------
def test_lists_match_host_score_h():
    """A shape added to the kernel's table without a case here fails on the CPU."""
    header = si.lists_in_header()
    for name, mine in si.LISTS.items():
        assert header.get(name) == mine, "%s: host_score.h has %r, the test iterates over %r" % (name, header.get(name), mine)
    for shape in si.SHAPES:
        lens, slot = si.shape_lengths(shape)
        assert lens and lens[-1] == shape[0] * shape[1] and len(lens) >= 2, shape
    assert sorted(s for s in si.SHAPES if si.shape_lengths(s)[1] == 16) == [(16, 8), (16, 16)]


def test_ranges_cover_the_cuts(pgs):
    """The cuts of every case's ranges are where Case says they are, at the nominal tile length and at another."""
    for shape in si.SHAPES:
        L = shape[0] * shape[1]
        for sem in (F32, U8SAT):
            for CL in (si.nominal_chunk(L, sem), 3 * 512):
                c = si.Case(pgs, shape, sem, si.DEFAULT, CL)
                A, B, C, D, E, F, G, H = c.ranges
                assert all(r[1] - r[0] >= 1024 and r[1] - r[0] > L + 1 for r in c.ranges)
                assert all(r[0] % 4 and r[0] % 64 for r in (A, B, C, E, F, G)) and H[0] % 64 == 0, c.ranges
                assert (A[1] - A[0]) % CL == 1 and (B[1] - B[0]) % CL == 0 and B[0] == A[1]
                assert C[1] - D[0] == 2 * L and G[1] == len(c.ref)
                assert (F[1] - F[0]) // CL > 256 // shape[0] or CL != si.nominal_chunk(L, sem), "F fits one workgroup's tiles"
                assert E[1] - E[0] == CL or CL < 1024 or CL <= L + 1
                assert len(c.queries) % 2 == 1 and len(c.queries) >= 5
                assert sorted(len(q) for q in c.queries)[2:4] == [c.l, c.L] and c.half[5] == 0 and c.half[0] == 1, "one pair holds l against L"


def test_inputs_hold_planted_hits(pgs, oracle):
    """Conditions on the inputs, from the oracle alone: every case holds a planted hit above 80 % of the perfect score and a range
    with only background for the same query, the hit across the cut A | B gives different partial scores in the two ranges, and the
    other planted hits are perfect.  (At the nominal tile length; the GPU cases check again at the one the host chose.)"""
    failures = []
    with si.make_pool() as pool:
        for shape in si.SHAPES:
            L = shape[0] * shape[1]
            todo = [(F32, si.DEFAULT), (U8SAT, si.DEFAULT if L <= 128 else si.U8_LOW_BACKGROUND)]
            if 100 <= L <= 160:                       # (shorter reads: a 26-letter table's background is too close)
                todo.append((F32, si.table_scorings(pgs)[4]))
            for sem, sc in todo:
                c = _case(pgs, oracle, pool, shape, sem, sc, si.nominal_chunk(L, sem))
                failures.extend("%r sem %d %s: %s" % (shape, sem, sc.name, f) for f in c.input_faults())
    _report(failures)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
ONE_TILE_SHAPES = ((8, 19), (16, 10), (16, 32))


def _variant_params():
    return [(sem, name, options) for sem in (F32, U8SAT) for name, options in si.variants(sem)]


@pytest.mark.gpu
@pytest.mark.parametrize("sem,name,options", _variant_params(), ids=lambda v: v if isinstance(v, str) else None)
def test_raw_maxima(pgs, oracle, sem, name, options):
    """Every shape under this cell variant at 3 / -3 / 2 (the uint8 engine's long reads also at 1 / -3 / 3, whose background stays
    below the cap)."""
    failures = []
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for vname, _, shape, want in si.plan(sem, si.DEFAULT):
                if vname != name:
                    continue
                L = shape[0] * shape[1]
                _run_case(pgs, oracle, pool, ctx, shape, sem, si.DEFAULT, want, failures, check_inputs=sem == F32 or L <= 128)
                if sem == U8SAT and L > 128:
                    sc = si.U8_LOW_BACKGROUND
                    _run_case(pgs, oracle, pool, ctx, shape, sem, sc, si.predicted(shape, L, sem, sc, options), failures)
                if shape in ONE_TILE_SHAPES:
                    # short reads get tiles of 256 columns, shorter than any range the score kernel takes: the tuning aid `chunk` makes
                    # range E one tile of 2048 columns (the whole-wavefront shapes have such a range at their own tile length)
                    ctx.set_option("chunk", 2048)
                    try:
                        _run_case(pgs, oracle, pool, ctx, shape, sem, si.DEFAULT, want, failures, check_inputs=False)
                    finally:
                        ctx.set_option("chunk", 0)
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("name,options", si.FLOAT_VARIANTS[:3], ids=lambda v: v if isinstance(v, str) else None)
def test_float16_scorings(pgs, oracle, name, options):
    """Mirrored and plain float16 shapes with a gap above the match, a zero mismatch, and a cheap gap with a long warm-up."""
    failures = []
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for sc in (si.GAP_ABOVE_MATCH, si.MISMATCH_ZERO, si.CHEAP_GAP):
                for vname, _, shape, want in si.plan(F32, sc):
                    if vname == name and want["cell"] == "f16":
                        _run_case(pgs, oracle, pool, ctx, shape, F32, sc, want, failures, check_inputs=False)
    finally:
        ctx.close()
    _report(failures)


TABLE_SHAPES = [(8, 13), (16, 10), (8, 19), (8, 26), (8, 32), (16, 20), (16, 24), (16, 32)]


def _profile_lds(nletters, shape):
    """launch_score's dynamic LDS of a one-strip two-query instance (profile_lds_bytes + the code windows)."""
    rp = (shape[1] + 3) // 4 * 4
    stride = rp + 4 if rp % 8 == 0 else rp
    return (nletters + 1) * 16 * stride * 4 + (256 // shape[0]) * 80


@pytest.mark.gpu
@pytest.mark.parametrize("name,options", si.FLOAT_VARIANTS, ids=lambda v: v if isinstance(v, str) else None)
def test_table_scoring(pgs, oracle, name, options):
    """An integer table (many distinct scores per profile, zeros, different scores in the two halves) on 20- and 26-letter alphabets
    with gaps 1, 3 and 11: two-query tiles of every float cell, the R = 26 / 32 profiles beyond 48 KiB of LDS."""
    failures = []
    big = 0
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for sc in si.table_scorings(pgs):
                for vname, _, shape, want in si.plan(F32, sc, TABLE_SHAPES):
                    if vname != name:
                        continue
                    big += _profile_lds(len(sc.alpha), shape) > 48 * 1024
                    _run_case(pgs, oracle, pool, ctx, shape, F32, sc, want, failures, check_inputs=sc.gap >= 3)
    finally:
        ctx.close()
    if name in ("f16m", "i16", "f32"):
        assert big >= 2, "no case of this variant needs more than 48 KiB of dynamic LDS"
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("name,options", si.FLOAT_VARIANTS[:3], ids=lambda v: v if isinstance(v, str) else None)
def test_table_at_the_cap(pgs, oracle, name, options):
    """Table entries of -1024, -1100 and -2048 (the cap of the mirrored profile entry) and the largest gap mirror_ok admits, 2040."""
    failures = []
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for sc in si.capped_table_scorings(pgs):
                for shape in ((8, 19), (16, 10)):
                    want = si.predicted(shape, shape[0] * shape[1], F32, sc, options)
                    assert want["cell"] == "f16" and want["mirror"] == (name != "f16"), want
                    _run_case(pgs, oracle, pool, ctx, shape, F32, sc, want, failures, check_inputs=False)
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("sem", [F32, U8SAT], ids=["f32", "u8"])
def test_mirror_bound_both_sides(pgs, oracle, sem):
    """Perfect-match reads with smax * maxlen + smax at 1024 and at the next value above it: mirrored cells at the bound, plain ones
    past it, exact answers on both sides (score_ranges against oracle.score_only, align_batch against oracle.align)."""
    failures = []
    ctx = _context(pgs, ("no_u8_early",) if sem == U8SAT else ())
    try:
        with si.make_pool() as pool:
            for match, length in si.MIRROR_BOUND:
                sc = si.Scoring("%d/%d/2 x %d rows" % (match, -match, length), match, -match, 2)
                shape = si.pick_bucket(length)
                want = si.predicted(shape, length, sem, sc, ())
                at_bound = match * length + match <= 1024
                assert want["cell"] == "f16" and want["mirror"] == int(at_bound), (want, match, length)
                what = "%s %s" % (si.instance_name(si.instance_key(want)), sc.name)
                ref = pgs.synth.dna(8800 + match + length, 6000)
                refb = ref.tobytes()
                ranges = [(1, 1500), (1400, 3100), (3001, 6000)]
                qs = [refb[at:at + length] for at in (3, 1500 - length, 1450, 3010, 6000 - length)]
                top = float(min(255, match * length) if sem == U8SAT else match * length)
                exp = np.array(list(pool.map(lambda rk: oracle.score_only(qs[rk[1]], refb[ranges[rk[0]][0]:ranges[rk[0]][1]], sem, **sc.kw()),
                                             [(r, k) for r in range(3) for k in range(5)]))).reshape(3, 5)
                assert (exp.max(axis=0) == top).all(), (what, exp)
                ctx.set_reference(refb)
                ctx.batch_upload(qs)
                got = ctx.score_ranges(ranges, semantics=sem, **sc.kw())
                PLANNED.add(si.instance_key(want))
                if _check_tags(si.parse_path(ctx.last_path()), want, what, failures):
                    RAN.setdefault(si.instance_key(want), []).append(what)
                for r, k in zip(*np.nonzero(got != exp)):
                    failures.append("%s: range %d query %d (%s half): kernel %g, oracle %g" % (what, r, k, "odd / high" if k % 2 else "even / low",
                                                                                                 got[r, k], exp[r, k]))
                if not (got.max(axis=0) == top).all():
                    failures.append("%s: top scores %r, not %g" % (what, got.max(axis=0).tolist(), top))
                res = ctx.align_batch(qs, refb, semantics=sem, **sc.kw())
                tags = si.parse_path(ctx.last_path())
                if not tags or any(t.get("mirror", 0) != int(at_bound) or t["cell"] != "f16" for t in tags):
                    failures.append("%s: align_batch ran %r" % (what, tags))
                for k, (g, e) in enumerate(zip(res, pool.map(lambda q: oracle.align(q, refb, sem, **sc.kw()), qs))):
                    if g["score"] != top:
                        failures.append("%s: align_batch query %d: score %g, not %g" % (what, k, g["score"], top))
                    for f in KEYS:
                        if g[f] != e[f]:
                            failures.append("%s: align_batch query %d: %s %r, oracle %r" % (what, k, f, g[f], e[f]))
    finally:
        ctx.close()
    _report(failures)


SAMPLED_VARIANTS = [(F32, "f16m", ()), (F32, "f16mf", ("no_f16m_int_diag",)), (F32, "f16", ("no_f16_mirror",)), (F32, "f32", ("force_f32",)),
                    (U8SAT, "unsat", ("no_u8_early",)), (U8SAT, "unsat_plain", ("no_u8_early", "no_f16_mirror"))]


@pytest.mark.gpu
@pytest.mark.parametrize("sem,name,options", SAMPLED_VARIANTS, ids=lambda v: v if isinstance(v, str) else None)
def test_sampled_instances(pgs, oracle, sem, name, options):
    """The MK = 4 instances (kR8M on 8-lane, kR16M on 16-lane and whole-wavefront tiles) through align_batch over one whole reference
    with a uniform background: sampled=1 in the path, exact results, and no second sweep.  Beyond float16's exact range the float
    engine's sampled sweep is the saturating one.  The zero-fall-back condition is on the inputs: a query may
    have 64 + 1024 / nq candidates, and these references hold fewer sub-chunks than that, so an honest sampled sweep cannot exceed it;
    one that under-reports fails here instead of costing a second sweep.  (The repeat-rich cases stay in the tests of the fall-backs.)"""
    failures = []
    ctx = _context(pgs, options)
    try:
        with si.make_pool() as pool:
            for shape in si.SAMPLED_SHAPES:
                L = shape[0] * shape[1]
                want = si.predicted(shape, L, sem, si.DEFAULT, options, allow_sat=True)
                key = si.instance_key(want)
                earlier = [v for v in SAMPLED_VARIANTS[:SAMPLED_VARIANTS.index((sem, name, options))] if v[0] == sem]
                if key in {si.instance_key(si.predicted(shape, L, sem, si.DEFAULT, o, allow_sat=True)) for _, _, o in earlier}:
                    continue                                   # (past the mirror bound the first variant already ran the plain cell)
                if want["cell"] == "f32" and shape[0] == 64:
                    continue                                   # (the host samples float32 batches on 8- and 16-lane tiles only)
                what = "sampled %s %s" % (si.instance_name(key), "u8" if sem == U8SAT else "f32")
                case = si.Case(pgs, shape, sem, si.DEFAULT, si.nominal_chunk(L, sem))
                nsub = -(-len(case.ref) // si.nominal_chunk(L, sem))
                assert nsub < 64 + 1024 // len(case.queries), "the reference holds more sub-chunks than a query's candidate budget"
                exp = list(pool.map(lambda q: oracle.align(q, case.ref, sem), case.queries))
                ctx.set_option("slot", case.slot)
                res = ctx.align_batch(case.queries, case.ref, semantics=sem)
                tags = si.parse_path(ctx.last_path())
                counters = ctx.last_counters()
                PLANNED_SAMPLED.add(key)
                if not _check_tags(tags, want, what, failures):
                    continue
                if any(t["sampled"] != 1 for t in tags):
                    failures.append("%s: not sampled: %r" % (what, tags))
                    continue
                RAN_SAMPLED.setdefault(key, []).append(what)
                if counters["whole_batch_again"] != 0 or counters["requeried"] != 0:
                    failures.append("%s: fell back: whole_batch_again %d, requeried %d (candidates %d)" % (
                        what, counters["whole_batch_again"], counters["requeried"], counters["candidates"]))
                for k, (g, e) in enumerate(zip(res, exp)):
                    for f in KEYS:
                        if g[f] != e[f]:
                            failures.append("%s: query %d (%s, %s half): %s %r, oracle %r" % (
                                what, k, si.QUERY_NAMES[k], "odd / high" if case.half[k] else "even / low", f, g[f], e[f]))
    finally:
        ctx.close()
    _report(failures)


@pytest.mark.gpu
def test_every_instance_ran():
    """Last: the union of the instances that ran equals the planned set — every 8-lane, 16-lane and one-strip whole-wavefront
    two-query shape under every cell the host can give it (shapes x cells minus what mirror_ok and the score bounds exclude, each
    exclusion computed by si.predicted from the host's inequality and the case's longest query)."""
    base = {si.instance_key(inst) for sem in (F32, U8SAT) for _, _, _, inst in si.plan(sem, si.DEFAULT)}
    for shape in si.SHAPES:                                     # the plan is not vacuous: these cells exist on every shape
        for cell, unsat in (("i16", 0), ("f32", 0), ("u8f16", 0), ("u8i16", 0), ("f16", 1)):
            assert any(k[0] == cell and k[1:3] == shape and k[5] == unsat for k in base), (shape, cell)
        if shape[0] != 64 and 3 * shape[0] * shape[1] + 3 <= 1024:
            assert (("f16",) + shape + (1, 1, 0)) in base and (("f16",) + shape + (1, 0, 0)) in base and (("f16",) + shape + (0, 0, 0)) in base
    missing = sorted(base - set(RAN))
    assert not missing, "planned at 3 / -3 / 2 but never ran: %s" % ", ".join(si.instance_name(k) for k in missing)
    assert set(RAN) == PLANNED, "ran and planned differ: %s" % ", ".join(si.instance_name(k) for k in sorted(set(RAN) ^ PLANNED))
    sampled = {(c, sl, r) for c, sl, r, _, _, _ in RAN_SAMPLED}
    for shape in si.SAMPLED_SHAPES:
        assert ("f16",) + shape in sampled and (shape[0] == 64 or ("f32",) + shape in sampled), shape
    assert set(RAN_SAMPLED) == PLANNED_SAMPLED, sorted(set(RAN_SAMPLED) ^ PLANNED_SAMPLED)
    print("\n%d score_ranges instances, %d sampled instances" % (len(RAN), len(RAN_SAMPLED)))
