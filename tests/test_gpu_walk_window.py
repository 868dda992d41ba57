"""Tracebacks whose greedy walk outgrows its first decision window: every route that answers a walk kernel's status 1
("window too small") — the solo kernel's decline, the widening loops of wave_trace (wave and strip decisions, one- and two-pass
walks) and of trace_located (sw_exact_kernel + sw_walk_kernel), the fall-back of the saved-state traceback — on inputs that force it
(tests/walk_window_cases.py; their classes come from the oracle alone, tests/test_walk_window_ref.py).  Everything goes through the
C-ABI and is bit-equal to the oracle; the counter walk_widened, the tags of mi355_sw_last_path and saved_fallbacks say that the
route under test really ran."""
import pytest

import walk_window_cases as wc

pytestmark = pytest.mark.gpu

KEYS = wc.KEYS


def _cmp(got, exp, what):
    for k in KEYS:
        assert got[k] == exp[k], "%s: %s differs: got %r expected %r" % (what, k, str(got[k])[:80], str(exp[k])[:80])


def _kw(sem, sc, lut=None):
    return dict(semantics=sem, match=sc[0], mismatch=sc[1], gap=sc[2], lut=lut)


def _walk_tags(path):
    return [t for t in path if t in ("walk_wave", "walk_long")]


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


@pytest.fixture
def options(ctx):
    """set(name) for the test's duration."""
    names = []

    def set_(name):
        ctx.set_option(name, True)
        names.append(name)
    yield set_
    for n in names:
        ctx.set_option(n, None)


_lone = {}


def _lone_expected(pgs, oracle, case):
    if case.name not in _lone:
        x, y = case.build(pgs)
        _lone[case.name] = (x, y, oracle.align(x, y, case.sem, *case.scoring))
    return _lone[case.name]


@pytest.mark.parametrize("case", wc.LONE, ids=repr)
def test_lone_read_solo_path_declines(pgs, oracle, ctx, options, case):
    """One read of 60 / 150 (sw_solo_kernel<3>) or 300 rows (<5>), runs that take 0 .. 3 widenings, both engines.
    Expected relation, from the code: the solo kernel runs on the FIRST window only (host_solo.h: budget = |x| / 8 + 64, never
    widened); its decline (kSoloWindow) sends the call to the general path, which starts again at that budget — so the solo round
    is no widening and walk_widened == rounds_needed exactly, with or without the solo kernel.  A forcing call therefore shows
    solo[ AND the general path's walk tag; a control shows solo[ alone.  Then the same with no_solo (the general
    path from the start: latency mode, strip decisions + sw_wave_walk_long_kernel) and with no_strip (wave decisions +
    sw_wave_walk_kernel<kWalkBoth>)."""
    x, y, exp = _lone_expected(pgs, oracle, case)
    kw = _kw(case.sem, case.scoring)
    smax, g = case.scoring[0], case.scoring[2]
    rounds = wc.rounds_needed(exp, case.m, smax, g)
    _cmp(ctx.align(x, y, **kw), exp, "%s" % case)
    path, cnt = ctx.last_path(), ctx.last_counters()
    print(case, "rounds", rounds, "walk_widened", cnt["walk_widened"], " ".join(path))
    assert any(t.startswith("solo[") for t in path), path
    if case.forcing:
        assert cnt["walk_widened"] == rounds == case.rounds, (cnt, rounds)
        assert len(_walk_tags(path)) == 1, path                                   # (a tag is noted once per call)
    elif case.rounds != "edge":
        assert cnt["walk_widened"] == 0 and not _walk_tags(path), (cnt, path)
    for opts, tag in ((("no_solo",), "walk_long"), (("no_solo", "no_strip"), "walk_wave")):
        for o in opts:
            ctx.set_option(o, True)
        try:
            _cmp(ctx.align(x, y, **kw), exp, "%s with %s" % (case, "+".join(opts)))
            path, cnt = ctx.last_path(), ctx.last_counters()
        finally:
            for o in opts:
                ctx.set_option(o, None)
        print(case, "+".join(opts), "walk_widened", cnt["walk_widened"], " ".join(path))
        assert not any(t.startswith("solo[") for t in path), path
        assert _walk_tags(path) and set(_walk_tags(path)) == {tag}, (opts, path)
        if case.forcing:
            assert cnt["walk_widened"] == rounds, (opts, cnt, rounds)
        elif case.rounds != "edge":
            assert cnt["walk_widened"] == 0, (opts, cnt)


@pytest.mark.parametrize("sem,sc", wc.SWEEP_ENGINES, ids=("f32", "u8"))
def test_boundary_sweep(pgs, oracle, ctx, options, sem, sc):
    """The read of 150 rows against runs of 222 .. 245: the host's first window stops holding the walk somewhere in between (the
    model: between 232 and 233).  Results at every K, on the default route and on the general path (no_solo).  The counter only
    at the two ends, where the model is 8 columns clear of zero — its + 2 / ceil terms are not restated to the column — and only
    on the general path, whose window is the model's: the solo kernel's window ends budget + need in front of the argmax's
    SUB-CHUNK, not of the argmax (sw_solo_kernel.h: wl = sub_lo - need_t), i.e. up to sub_len + 63 = 127 columns further left, so it
    holds every walk of this sweep (measured: no decline for any K here; the run of 400 of the lone cases is the first listed
    length it declines).  On the default route the call either stayed on the solo kernel or widened."""
    for route in ("default", "no_solo"):
        if route == "no_solo":
            options("no_solo")
        widened, walked = [], []
        for K in wc.SWEEP_K:
            x, y = wc.sweep_case(pgs, K)
            exp = oracle.align(x, y, sem, *sc)
            _cmp(ctx.align(x, y, **_kw(sem, sc)), exp, "sweep K=%d (%s)" % (K, route))
            widened.append(ctx.last_counters()["walk_widened"])
            walked.append(bool(_walk_tags(ctx.last_path())))
        print("sweep", route, sem, sc, dict(zip(wc.SWEEP_K, widened)))
        assert widened[0] == 0, (route, widened)
        if route == "no_solo":
            assert all(walked) and widened[-1] >= 1, (route, widened)
        else:
            assert widened[-1] >= 1 or not walked[-1], (route, widened, walked)


def _run_batch(pgs, oracle, ctx, name, tag, sem, sc, lut=None):
    reads, ref, starts, forcing_at = wc.batch(pgs, name)
    exp = wc.expected(oracle, (name, tag), reads, ref, sem, sc, lut)
    got = ctx.align_batch(reads, ref, **_kw(sem, sc, lut))
    path, cnt = ctx.last_path(), ctx.last_counters()
    print(name, tag, "walk_widened", cnt["walk_widened"], "saved_fallbacks", cnt["saved_fallbacks"], " ".join(path)[:600])
    assert len(got) == len(reads)
    for i, (a, e) in enumerate(zip(got, exp)):
        _cmp(a, e, "%s (%s) read %d%s" % (name, tag, i, " (forcing)" if i in forcing_at else ""))
    rounds = sum(wc.rounds_needed(exp[i], len(reads[i]), sc[0], sc[2]) for i in forcing_at)
    return path, cnt, rounds


def test_batch_of_200_reads_mixes_finished_and_widened_walks(pgs, oracle, ctx):
    """200 reads of 150 rows (run_wave + sw_wave_walk_kernel<kWalkBoth>: 65 .. 4096 walks take one pass), the reads that need 1, 2
    and 3 widenings at indices 0, 1, 100, 198, 199 and a control at 57, ordinary reads everywhere else: the walks that finish in
    round 0 keep their strings in that round's buffer while rounds 1 .. 3 run for the others.  Every read is compared."""
    path, cnt, rounds = _run_batch(pgs, oracle, ctx, "batch200", "default", wc.F32, wc.DEFAULT)
    assert rounds == 9
    assert cnt["walk_widened"] == rounds, cnt
    assert _walk_tags(path) == ["walk_wave"], path


def test_batch_of_9_reads_in_latency_mode(pgs, oracle, ctx):
    """The same reference with 9 reads (at most 64: strip decisions + sw_wave_walk_long_kernel, one wavefront per walk)."""
    path, cnt, rounds = _run_batch(pgs, oracle, ctx, "batch9", "default", wc.F32, wc.DEFAULT)
    assert cnt["walk_widened"] == rounds == 9, cnt
    assert _walk_tags(path) == ["walk_long"], path


def test_batch_beyond_4096_walks_takes_two_passes(pgs, oracle, ctx):
    """4100 reads of 40 rows, the forcing read (two widenings) at indices 0, 2048 and 4099.  From the code (host_wave.h): a group
    of more than 4096 walks is not one_pass, so round 0 runs sw_wave_walk_kernel<kWalkMeasure>, lays the strings out back to back
    — the three walks with status 1 get no room — and <kWalkWrite> skips them; all 4100 jobs fit one group (262144 jobs, 2 GiB of
    decisions).  Rounds 1 and 2 hold the three re-queued walks alone (latency mode does not apply: the mode is fixed per call)."""
    path, cnt, rounds = _run_batch(pgs, oracle, ctx, "batch4100", "default", wc.F32, wc.DEFAULT)
    assert rounds == 6
    assert cnt["walk_widened"] == rounds, cnt
    assert _walk_tags(path) == ["walk_wave"], path


@pytest.mark.parametrize("scoring", ("table", "mismatch0"))
def test_route_through_exact_and_walk_kernels(pgs, oracle, ctx, options, scoring):
    """Scorings the wave kernel does not take — a 256 x 256 table that IS 3 / -3 on ACGT (lut != NULL), and 2 / 0 / 1 (mismatch
    >= 0) — send short reads to trace_located's own loop: sw_exact_kernel windows + sw_walk_kernel, budget * 4 on status 1.
    Lone (the solo path needs wave scoring too: it does not take these) and the batch of 9."""
    sc = wc.DEFAULT if scoring == "table" else wc.MISMATCH_ZERO
    lut = wc.identity_lut(3.0, -3.0) if scoring == "table" else None
    for case in (c for c in wc.LONE if c.sem == wc.F32 and c.scoring == wc.DEFAULT and c.m == 150):
        x, y = case.build(pgs)
        exp = oracle.align(x, y, wc.F32, sc[0], sc[1], sc[2], lut)
        if scoring == "table":
            assert exp == _lone_expected(pgs, oracle, case)[2]
        rounds = wc.rounds_needed(exp, case.m, sc[0], sc[2])
        assert (rounds >= 1) == case.forcing
        _cmp(ctx.align(x, y, **_kw(wc.F32, sc, lut)), exp, "%s under %s" % (case, scoring))
        path, cnt = ctx.last_path(), ctx.last_counters()
        print(case, scoring, "rounds", rounds, "walk_widened", cnt["walk_widened"], " ".join(path))
        assert not _walk_tags(path) and not any(t.startswith("solo[") for t in path), path
        assert cnt["walk_widened"] == rounds, (case, cnt, rounds)
    tag = "lut" if scoring == "table" else "mismatch0"
    path, cnt, rounds = _run_batch(pgs, oracle, ctx, "batch9", tag, wc.F32, sc, lut)
    assert not _walk_tags(path), path
    assert rounds >= 1 and cnt["walk_widened"] == rounds, (cnt, rounds)


@pytest.mark.parametrize("k", (0, 1))
def test_long_query_lone(pgs, oracle, ctx, k):
    """700 and 1500 rows (beyond 512: strip decisions, sw_wave_walk_long_kernel), a run of rows + 600."""
    m, K, fl, fr = wc.LONG_LONE[k]
    x, y = wc.long_lone_case(pgs, k)
    exp = oracle.align(x, y, wc.F32, *wc.DEFAULT)
    _cmp(ctx.align(x, y), exp, "long lone m=%d" % m)
    path, cnt = ctx.last_path(), ctx.last_counters()
    print("long lone", m, "walk_widened", cnt["walk_widened"], " ".join(path))
    assert cnt["walk_widened"] >= 1, cnt
    assert _walk_tags(path) == ["walk_long"], path


def test_long_queries_beside_short_reads(pgs, oracle, ctx):
    """The two long reads at indices 1 and 5 of a batch with five ordinary reads of 150 rows: trace_located's second pass."""
    path, cnt, rounds = _run_batch(pgs, oracle, ctx, "batch_long", "default", wc.F32, wc.DEFAULT)
    assert cnt["walk_widened"] >= 2, cnt                                          # both long reads at least once
    assert "walk_long" in path, path


@pytest.mark.parametrize("k", (2, 3))
def test_lone_query_beyond_2048_rows_falls_back_from_saved_state(pgs, oracle, ctx, options, k):
    """2500 rows against a run of 3400.  The sweep is sw_long_kernel and saves its columns and strip rows (long[...saved=1...]);
    the locate step starts from them (saved_locate), the traceback from saved state is refused by the walk's checks — at these
    reference lengths the sweep's tiles are one sub-chunk long, so a cell of row ~2500 is never need(row) columns behind its
    tile's zero border (WaveWalk::zchunk) — the call counts a saved_fallback and goes to wave_trace's strip route, which the
    901 west steps outgrow.
    k = 3: the shortest reference with that tag — bucket_fast_ok (host_score.h) gives strip-mined queries to the score kernels
    from 4096 columns on.  There need(2500) = 6252 columns exceed the reference: the zero-border window starts at column 0, is
    not checked, and walk_widened stays 0 (by the window rule, not by measurement).
    k = 2: 8192 columns, 3400 of them in front of the run, so that the first zero-border window (376 + 6252 columns) is a
    true window: saved_fallbacks >= 1 AND walk_widened >= 1.  Then no_long_save: the same answer without saved state."""
    m, K, fl, fr = wc.LONG_LONE[k]
    x, y = wc.long_lone_case(pgs, k)
    assert m == 2500 and K == 3400 and len(y) == (8192 if k == 2 else 4096)
    exp = oracle.align(x, y, wc.F32, *wc.DEFAULT)
    _cmp(ctx.align(x, y), exp, "m=2500, %d columns" % len(y))
    path, cnt = ctx.last_path(), ctx.last_counters()
    print("beyond 2048 rows", len(y), cnt, " ".join(path))
    assert any(t.startswith("long[") and "saved=1" in t for t in path), path
    assert cnt["saved_fallbacks"] >= 1 and cnt["saved_traces"] == 0, cnt
    assert "walk_long" in path, path
    if k == 2:
        assert cnt["walk_widened"] >= 1, cnt
    else:
        assert cnt["walk_widened"] == 0, cnt
    options("no_long_save")
    _cmp(ctx.align(x, y), exp, "m=2500, %d columns, no_long_save" % len(y))
    path2, cnt2 = ctx.last_path(), ctx.last_counters()
    assert any(t.startswith("long[") and "saved=0" in t for t in path2), path2
    assert cnt2["saved_fallbacks"] == 0 and cnt2["walk_widened"] == cnt["walk_widened"], (cnt, cnt2)


@pytest.mark.parametrize("name", ("lone_k400", "lone_k600"))
def test_window_clamped_by_the_start_of_the_reference(pgs, oracle, ctx, options, name):
    """The reference BEGINS with the run: as soon as budget + need covers the columns in front of the end cell the window starts
    at column 0 (wl == 0, exact_from == 0: nothing to check) — at once for 400 letters, after one widening for 600 — although
    the model's slack is negative in that very round."""
    c = wc.clamped_case(pgs, name)
    exp = oracle.align(c["x"], c["y"], wc.F32, *wc.DEFAULT)
    for opts in ((), ("no_solo",), ("no_solo", "no_strip")):
        for o in opts:
            options(o)
        _cmp(ctx.align(c["x"], c["y"]), exp, "%s %s" % (name, "+".join(opts)))
        cnt = ctx.last_counters()
        print(name, opts, "walk_widened", cnt["walk_widened"], " ".join(ctx.last_path()))
        assert cnt["walk_widened"] == c["widenings"], (name, opts, cnt)


def test_window_clamped_by_a_piece_cut(pgs, oracle, ctx):
    """align_split: the run straddles the cut in front of piece 2 of 4, which wins (the piece before holds no end of the run);
    its walk ends at the piece's first column."""
    c = wc.clamped_case(pgs, "split")
    ranges = pgs.capi.make_string_range(wc.SPLIT_PIECES, len(c["x"]), wc.SPLIT_N, wc.SPLIT_RATIO)
    assert tuple(ranges[c["winner"]]) == c["range"], ranges
    exp = oracle.align_split(c["x"], c["y"], wc.SPLIT_PIECES, wc.SPLIT_RATIO, 0, 0)
    got = ctx.align_split(c["x"], c["y"], wc.SPLIT_PIECES, wc.SPLIT_RATIO, 0, 0)
    cnt = ctx.last_counters()
    print("split", "walk_widened", cnt["walk_widened"], " ".join(ctx.last_path()))
    for k in KEYS + ("piece",):
        assert got[k] == exp[k], ("align_split", k, str(got[k])[:80], str(exp[k])[:80])
    assert exp["piece"] == c["winner"] and exp["pos"] == c["range"][0] + 1
    assert cnt["walk_widened"] == c["widenings"], cnt


def test_window_clamped_by_a_range_start(pgs, oracle, ctx):
    """best_range + align_scored_range over a range that starts inside the run."""
    c = wc.clamped_case(pgs, "range")
    ctx.set_reference(c["y"])
    ctx.batch_upload([c["x"]])
    best, which, _ = ctx.best_range(c["ranges"])
    assert int(which[0]) == c["winner"] and best[0] == 450.0, (which, best)
    got = ctx.align_scored_range(c["winner"])
    cnt = ctx.last_counters()
    print("range", "walk_widened", cnt["walk_widened"], " ".join(ctx.last_path()))
    _cmp(got, oracle.align(c["x"], c["range_bytes"], wc.F32, *wc.DEFAULT), "align_scored_range")
    assert got["pos"] == 1
    assert cnt["walk_widened"] == c["widenings"], cnt


def test_context_stays_usable_after_three_rounds(pgs, oracle):
    """After a call that widened three times, an ordinary align and an ordinary align_batch on the same context: the oracle's
    answers, walk_widened back at 0."""
    case = next(c for c in wc.LONE if c.name == "f32-3_-3_2-m150-K1500")
    x, y, exp = _lone_expected(pgs, oracle, case)
    ref = pgs.synth.dna(7700, 20_000)
    reads = [wc.ordinary_read(pgs, ref, 7710 + k, 150)[0] for k in range(12)]
    refb = ref.tobytes()
    c = pgs.Context(0)
    try:
        _cmp(c.align(x, y), exp, "three rounds")
        assert c.last_counters()["walk_widened"] == 3
        _cmp(c.align(reads[0], refb), oracle.align(reads[0], refb, 0), "ordinary align afterwards")
        assert c.last_counters()["walk_widened"] == 0
        got = c.align_batch(reads, refb)
        assert c.last_counters()["walk_widened"] == 0
        for k, (a, q) in enumerate(zip(got, reads)):
            _cmp(a, oracle.align(q, refb, 0), "ordinary batch afterwards, read %d" % k)
        _cmp(c.align(x, y), exp, "three rounds again")
        assert c.last_counters()["walk_widened"] == 3
    finally:
        c.close()
