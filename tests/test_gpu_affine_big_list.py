"""Affine pair lists longer than one launch, on every exact stage (csrc/host_affine.h): lists of 88 001 small pairs built by
tests/affine_big_list_cases.py run through every affine list call — local, banded and end-to-end pairs, the anchored extension plain,
banded and under the z-drop, the global alignment with plain and banded pairs in one list — on both dispatches (the list kernels, and
the option that sends every pair to the exact kernels) and through both calls, run and trace.  Every field of every pair must equal
the family's checker (tests/affine_*_ref.py on the 256 dictionary entries, gathered by the list's index sequence): scores are integers,
so there is no tolerance.  Each test also asserts that the cut it is about HAPPENED: the path names the kernels, and the counters
exact_launches / trace_launches equal what the job counts of the checker's values give by ceiling division (at least 2).  Every checked
call follows the same call on the preceding list of the cases module, so a device slot that a launch skips or re-bases wrongly holds a
value that is wrong by construction.

Which site of csrc/host_affine.h each test covers:
  affine_exact_stage -> run_affine_exact (ExactJob)      test_family[local-exact], test_family[e2e-exact]
  affine_exact_stage -> run_affine_exact (ExactBandJob)  test_family[band-exact]
  affine_trace<BAND>                                     test_family[local-*], [e2e-*] (BAND = false), [band-*] (true); its byte budget:
                                                         test_byte_budget_of_a_traceback_group[pairs]
  affine_ext_exact_stage<BAND, GLOB>                     test_family[extend-exact] (false, false), [extend_band-exact], [zdrop-exact] (true, false),
                                                         [global-exact] (false, true), [global_band-exact] (true, true)
  affine_ext_trace<BAND> and its column-0 arena          test_family[extend-*], [global-*] (false), [extend_band-*], [zdrop-*], [global_band-*] (true);
                                                         its byte budget: test_byte_budget_of_a_traceback_group[extend], test_rows_stage_cut_at_the_word_bound
  affine_ext_rows_stage                                  test_family[zdrop-exact] (65 536 problems), test_rows_stage_cut_at_the_word_bound (2^24 words)
  affine_list_stage                                      test_family[*-list]: 88 001 pairs, one launch per instance R, outputs at NO * i0"""
import contextlib

import numpy as np
import pytest

from tests import affine_big_list_cases as bc
from tests.test_gpu_affine_extend_band import BAND_R, same
from tests.test_gpu_affine_pairs import PAIR_R

pytestmark = pytest.mark.gpu

# family -> (run call, trace call, the option that sends every pair to the exact kernels, the list kernels' tags: plain, banded)
CALLS = {
    "local": ("affine_pairs_run", "affine_pairs_trace", "no_affine_pairs", "affine_pair[R=%d]", None),
    "band": ("affine_pairs_run", "affine_pairs_trace", "no_affine_band", None, "affine_band[R=%d]"),
    "e2e": ("affine_pairs_run", "affine_pairs_trace", "no_affine_pairs", "affine_pair_e2e[R=%d]", None),
    "extend": ("affine_extend_run", "affine_extend_trace", "no_affine_pairs", "affine_pair_ext[R=%d]", None),
    "extend_band": ("affine_extend_run", "affine_extend_trace", "no_affine_band", None, "affine_band_ext[R=%d]"),
    "zdrop": ("affine_extend_zdrop_run", "affine_extend_zdrop_trace", "no_affine_band", None, "affine_band_extz[R=%d]"),
    "global": ("affine_global_run", "affine_global_trace", "no_affine_pairs", "affine_pair_glob[R=%d]", "affine_band_glob[R=%d]"),
    "global_band": ("affine_global_run", "affine_global_trace", "no_affine_pairs", "affine_pair_glob[R=%d]", "affine_band_glob[R=%d]"),
}
_resident = {}


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    _resident.clear()
    c.close()


def resident(ctx, name, y, xs):
    if _resident.get("name") != name:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
        _resident["name"] = name


@contextlib.contextmanager
def option(ctx, name):
    if name:
        ctx.set_option(name, 1)
    try:
        yield
    finally:
        if name:
            ctx.set_option(name, 0)


def listed(family, entries, idx):
    """The arguments of a list: those of the dictionary's entries, gathered by the list's index sequence."""
    q, lo, hi, kw, tkw = bc.call_args(family, entries)
    take = lambda v: np.asarray(v)[idx] if isinstance(v, list) else v
    return (take(q), take(lo), take(hi)), {k: take(v) for k, v in kw.items()}, {k: take(v) for k, v in tkw.items()}


def kernel_tags(path):
    return {t for t in path if t.startswith("affine") and t != "affine_trace"}


def expected_tags(family, exact):
    jobs = bc.stage_jobs(family)["exact"]
    if exact:
        names = dict(plain="affine_exact", band="affine_exact_band", rows="affine_exact_band_rows")
        return {names[s] for s, v in jobs.items() if v}
    plain, band = CALLS[family][3:]
    return {(band if geo == "band" else plain) % R for geo, R in bc.list_instances(family, PAIR_R, BAND_R)}


def differs(got, exp, fields, k):
    return any((got[f][k] != exp[f][k]) for f in fields)


@pytest.mark.parametrize("dispatch", ("list", "exact"))
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_family(ctx, family, dispatch):
    """88 001 pairs of one family on one dispatch, run and trace, each behind the same call on the preceding list."""
    exact = dispatch == "exact"
    run_name, trace_name, opt = CALLS[family][:3]
    run_f, trace_f = bc.FIELDS[family]
    es, (run_rec, tr_rec) = bc.entries(family), bc.records(family)
    idx, pidx = bc.seq(bc.N), bc.seq(bc.N, bc.STRIDE)
    jobs = bc.stage_jobs(family)
    assert min(bc.launches(jobs["exact"]), bc.launches(jobs["trace"])) >= 2 and max(jobs["exact"].values()) > bc.LAUNCH
    resident(ctx, "families", bc.reference(), bc.reads())
    (args, kw, tkw), (pargs, pkw, ptkw) = listed(family, es, idx), listed(family, es, pidx)
    exp, texp = bc.gather(run_rec, run_f, idx), bc.gather(tr_rec, trace_f, idx)
    with option(ctx, opt if exact else None):
        prev = getattr(ctx, run_name)(*pargs, **pkw, **bc.SC)
        got = getattr(ctx, run_name)(*args, **kw, **bc.SC)
        path, cnt, tim = ctx.last_path(), ctx.last_counters(), ctx.last_timings()
        same(got, exp, run_f)                                         # (before the trace calls: a wrong end cell fails their own check)
        tprev = getattr(ctx, trace_name)(*pargs, **pkw, **ptkw, **bc.SC)
        traced = getattr(ctx, trace_name)(*args, **kw, **tkw, **bc.SC)
        tpath, tcnt, ttim = ctx.last_path(), ctx.last_counters(), ctx.last_timings()
    same(traced, texp, trace_f)
    # the preceding calls really ran, and left something else in the slots
    same(prev, bc.gather(run_rec, run_f, pidx), run_f)
    k = bc.LAUNCH                                                     # the first problem of a second launch, where one list is one stage
    assert differs(prev, exp, run_f, k) and differs(tprev, texp, trace_f, k)
    for f in trace_f:
        assert tprev[f][k] == tr_rec[int(pidx[k])][f], f
    # the path: which kernels ran
    tags = expected_tags(family, exact)
    assert kernel_tags(path) == tags and kernel_tags(tpath) == tags, (path, tpath, tags)
    assert "affine_trace" in tpath and "affine_trace" not in path
    # the counters: the cut happened, as often as the job counts say
    n_trace = bc.launches(jobs["trace"])
    if exact:
        n_exact = bc.launches(jobs["exact"])
        assert n_exact >= 2 and n_trace >= 2
        assert cnt["exact_launches"] == n_exact and tcnt["exact_launches"] == n_exact, (cnt, tcnt, jobs)
        assert tim["score_launches"] == 0 and ttim["score_launches"] == 0
    else:
        assert cnt["exact_launches"] == 0 and tcnt["exact_launches"] == 0
        assert tim["score_launches"] == len(tags) and ttim["score_launches"] == len(tags), (tim, tags)
    assert cnt["trace_launches"] == 0 and tcnt["trace_launches"] == n_trace, (tcnt, jobs)
    if family == "zdrop":
        stopped = int((exp["rows_done"] < np.array([p.q_hi - p.q_lo for p in es])[idx]).sum())
        assert cnt["zdrop_stopped"] == stopped > bc.N // 9


def test_rows_stage_cut_at_the_word_bound(ctx):
    """56 001 reads of 150 rows under the z-drop and option no_affine_band: fewer than 65 536 problems, and the rows instance still
    takes two launches, because 55 924 problems fill its 2^24 row words.  A third of the reads stop early, so the second step (one
    launch) runs on rewritten m, n and bhi.  The traceback of this list needs about 1 GiB of device scratch: its decision bytes
    (some 46 KiB per pair) cut its pass into groups at the 2^30 byte budget, not at 65 536 problems."""
    es, (run_rec, tr_rec) = bc.word_entries(), bc.word_records()
    run_f, trace_f = bc.FIELDS["zdrop"]
    idx, pidx = bc.word_seq(bc.WORD_N), bc.word_seq(bc.WORD_N, bc.STRIDE)
    rows_launches = bc.rows_launches([bc.WORD_ROWS] * bc.WORD_N)
    assert rows_launches == 2 and bc.WORD_N < bc.LAUNCH
    resident(ctx, "word", bc.reference(), bc.word_reads())
    (args, kw, tkw), (pargs, pkw, ptkw) = listed("zdrop", es, idx), listed("zdrop", es, pidx)
    kw["zdrop"] = pkw["zdrop"] = bc.WORD_ZDROP
    exp, texp = bc.gather(run_rec, run_f, idx), bc.gather(tr_rec, trace_f, idx)
    sizes = [bc.dirs_bytes(int(i), int(j)) for i, j in zip(texp["end_x"], texp["end_y"]) if i >= 1 and j >= 1]
    groups = bc.trace_groups(sizes)
    assert len(groups) >= 2 and max(groups) < bc.LAUNCH              # cut by the bytes
    with option(ctx, "no_affine_band"):
        prev = ctx.affine_extend_zdrop_run(*pargs, **pkw, **bc.SC)
        got = ctx.affine_extend_zdrop_run(*args, **kw, **bc.SC)
        path, cnt = ctx.last_path(), ctx.last_counters()
        traced = ctx.affine_extend_zdrop_trace(*args, **kw, **tkw, **bc.SC)
        tpath, tcnt = ctx.last_path(), ctx.last_counters()
    same(got, exp, run_f)
    same(traced, texp, trace_f)
    same(prev, bc.gather(run_rec, run_f, pidx), run_f)
    assert differs(prev, exp, run_f, bc.WORD_PER_LAUNCH)               # the first problem of the second rows launch
    assert kernel_tags(path) == {"affine_exact_band_rows", "affine_exact_band"} == kernel_tags(tpath) and "affine_trace" in tpath
    # two launches of the rows instance and one of the second step
    assert cnt["exact_launches"] == rows_launches + 1 == 3 and tcnt["exact_launches"] == 3, (cnt, tcnt)
    assert cnt["trace_launches"] == 0 and tcnt["trace_launches"] == len(groups), (tcnt, groups)
    assert cnt["zdrop_stopped"] == int((exp["rows_done"] < bc.WORD_ROWS).sum()) and bc.WORD_N // 3 <= cnt["zdrop_stopped"] <= bc.WORD_N // 3 + 1


@pytest.mark.parametrize("family", ("pairs", "extend"))
def test_byte_budget_of_a_traceback_group(ctx, family):
    """22 pairs of about 5000 rows x 5000 columns: at (m + n + 1) min(m, n) + 16 decision bytes each 21 fit under 2^30 and the 22nd
    opens a second launch group.  This needs about 1 GiB of device scratch.  The answers are known by construction (a read cut
    from the reference with one substitution: score 3 (m - 1) - 3, CIGAR mM, the strings are the read and the window);
    tests/test_affine_big_list_ref.py runs the same constructor at 50 rows against the checkers."""
    y, xs, wins = bc.budget_case()
    rows = bc.budget_expected(y, xs, wins)
    sizes = [bc.dirs_bytes(len(x), hi - lo) for x, (lo, hi) in zip(xs, wins)]
    assert sum(sizes[:21]) <= bc.TRACE_BYTES < sum(sizes) and bc.trace_groups(sizes) == [21, 1]
    resident(ctx, "budget", y, xs)
    q, lo, hi = list(range(len(xs))), [w[0] for w in wins], [w[1] for w in wins]
    if family == "pairs":
        run_f, trace_f = bc.PAIRS_RUN, bc.PAIRS_TRACE
        got = ctx.affine_pairs_run(q, lo, hi, **bc.SC)
        cnt = ctx.last_counters()
        traced = ctx.affine_pairs_trace(q, lo, hi, **bc.SC)
    else:
        run_f, trace_f = bc.EXT_RUN, bc.EXT_TRACE
        got = ctx.affine_extend_run(q, lo, hi, **bc.SC)
        cnt = ctx.last_counters()
        traced = ctx.affine_extend_trace(q, lo, hi, **bc.SC)
    tpath, tcnt, ttim = ctx.last_path(), ctx.last_counters(), ctx.last_timings()
    same(got, bc.gather(rows, run_f, np.arange(len(xs))), run_f)
    same(traced, bc.gather(rows, trace_f, np.arange(len(xs))), trace_f)
    assert kernel_tags(tpath) == {"affine_exact"} and "affine_trace" in tpath
    assert cnt["exact_launches"] == 1 and cnt["trace_launches"] == 0
    assert tcnt["exact_launches"] == 1 and tcnt["trace_launches"] == 2, tcnt
    print("byte budget, %s: %d pairs, traceback %.1f ms in 2 groups, whole trace call %.1f ms on the device"
          % (family, len(xs), ttim["trace_us"] * 1e-3, ttim["total_us"] * 1e-3))
