"""The constructor of tests/affine_big_list_cases.py, pinned with the checkers alone (no GPU needed): the entries of every family are
pairwise distinct, any eight consecutive pairs of a list hold all eight classes, the list that precedes a checked one shifts every
class by four and never expects what the checked list expects (nor two empty results), every exact stage and every traceback pass
under test gets more than 65 536 jobs, and each class shows what it is built to show on the checker's own values.  Also: the header
names the two launch counters the GPU tests prove the cuts with."""
import os
import re

import numpy as np
import pytest

from tests import affine_big_list_cases as bc
from tests import affine_e2e_ref, affine_extend_ref, affine_trace_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_the_header_names_the_launch_counters(pgs):
    header, source, host = _read(ROOT, "include", "mi355_sw.h"), _read(CSRC, "mi355_sw.hip"), _read(CSRC, "host_affine.h")
    for counter in ("exact_launches", "trace_launches"):
        assert '"%s"' % counter in header and '"%s"' % counter in source
        assert '"%s"' % counter in _read(ROOT, "parallel-genomeseq_amd", "capi.py")
    at = header.index('"zdrop_rows_run"')
    assert at < header.index('"exact_launches"') < header.index('"trace_launches"') < header.index("mi355_sw_affine_extend_run_zdrop(", at)
    # every launch of an exact or a traceback kernel is counted, and the counters start where the z-drop counters do
    launches = re.findall(r"launch_dyn_lds\((?:&sw_affine_exact|affine_exact_instance)", host)
    assert len(launches) == 5 and host.count("ctx->exact_launches += 1;") == 3      # (three launch lines share one count in the ext stage)
    assert host.count("ctx->trace_launches += 1;") == 2 and len(re.findall(r"launch_dyn_lds\(&sw_affine_trace", host)) == 2
    reset = _read(CSRC, "host_pipeline.h")
    assert re.search(r"ctx->zdrop_stopped = 0; ctx->zdrop_rows_run = 0;\s*ctx->exact_launches = 0; ctx->trace_launches = 0;", reset)


def test_the_list_length():
    assert bc.N > bc.LAUNCH and all(bc.N % v for v in (16, 64, 256))
    assert bc.WORD_PER_LAUNCH == 55924 and bc.WORD_PER_LAUNCH < bc.WORD_N < bc.LAUNCH
    assert len(bc.reads()) <= 64 and all(12 <= len(x) <= 40 for x in bc.reads()) and len(bc.reference()) == bc.YLEN


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_entries_are_distinct_and_inside_the_reference(family):
    es = bc.entries(family)
    assert len(es) == bc.D and len({bc.key(p) for p in es}) == bc.D
    assert all(0 <= p.lo <= p.hi <= bc.YLEN for p in es)


def test_any_eight_consecutive_pairs_hold_all_classes():
    for shift in (0, bc.STRIDE):
        s = bc.seq(bc.N, shift)
        cls = s % 8
        windows = np.lib.stride_tricks.sliding_window_view(cls, 8)
        assert (np.sort(windows, axis=1) == np.arange(8)).all()
        assert len(set(s[:bc.D].tolist())) == bc.D                    # a list walks through the whole dictionary


def test_the_preceding_list_shifts_every_class_by_four():
    s, p = bc.seq(bc.N), bc.seq(bc.N, bc.STRIDE)
    assert ((p - s) % bc.D == bc.SHIFT).all() and ((p % 8) == (s % 8 + 4) % 8).all()


def _empty(rec):
    return all((v == "" or v == 0) for v in rec.values())


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_a_stale_result_is_wrong_by_construction(family):
    run, tr = bc.records(family)
    for d in range(bc.D):
        e = (d + bc.SHIFT) % bc.D
        assert run[d] != run[e] and tr[d] != tr[e], (family, d)
        assert not (_empty(run[d]) and _empty(run[e])) and not (_empty(tr[d]) and _empty(tr[e])), (family, d)
        if not family.startswith("global"):                           # what a skipped problem leaves in outs_f / outs_i: score and end cell
            assert (run[d]["score"], run[d]["end_x"], run[d]["end_y"]) != (run[e]["score"], run[e]["end_x"], run[e]["end_y"]), (family, d)


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_every_stage_gets_more_than_one_launch(family):
    for shift in (0, bc.STRIDE):
        jobs = bc.stage_jobs(family, bc.N, shift)
        main = "band" if family in ("band", "extend_band", "zdrop", "global_band") else "plain"
        assert jobs["exact"][main] > bc.LAUNCH and jobs["trace"][main] > bc.LAUNCH, jobs
        assert bc.launches(jobs["exact"]) >= 2 and bc.launches(jobs["trace"]) >= 2
    jobs = bc.stage_jobs(family)
    assert bc.dirs_upper(family) < bc.TRACE_BYTES                      # the byte budget of a traceback group cuts none of these lists
    tr = bc.records(family)[1]
    untraced = {d % 8 for d, p in enumerate(bc.entries(family)) if not bc.has_trace_job(family, p, tr[d])}
    assert len(untraced) <= 2, untraced
    if family == "zdrop":
        assert jobs["exact"]["rows"] == jobs["exact"]["band"] and bc.LAUNCH * 2 * 40 < bc.ROW_WORDS   # the word bound never cuts 40-row reads
    if family.startswith("global"):                                   # both kinds in one list; the other kind fits one launch
        other = "plain" if family == "global_band" else "band"
        assert 0 < jobs["exact"][other] <= bc.LAUNCH and 0 < jobs["trace"][other] <= bc.LAUNCH
    else:
        assert len(jobs["exact"]) == (2 if family == "zdrop" else 1) and len(jobs["trace"]) == 1


def _of(family, cls):
    es, (run, tr) = bc.entries(family), bc.records(family)
    ds = [d for d in range(bc.D) if bc.CLASSES[d % 8] == cls]
    return [(es[d], run[d], tr[d]) for d in ds]


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_each_class_shows_what_it_is_built_to_show(family):
    xs, y = bc.reads(), bc.reference()
    glob, ext, pairs = family.startswith("global"), family in ("extend", "extend_band", "zdrop"), family in ("local", "band", "e2e")
    for p, run, tr in _of(family, "zero"):
        assert _empty(run) and _empty(tr) and not bc.has_job(family, p)
    for p, run, tr in _of(family, "hit"):
        assert bc.has_job(family, p) and tr["score"] >= 3 * 29 - 3 - 8
        if not glob or p.hi - p.lo == 30:                             # (a longer window under the global model: a gap at the end)
            assert tr["cigar"] == "30M"
    for p, run, tr in _of(family, "ins"):
        assert "3I" in tr["cigar"] and (glob or "D" not in tr["cigar"]) and "-" in tr["cons_y"]   # (global: a longer window ends in a gap)
    for p, run, tr in _of(family, "del"):
        assert "3D" in tr["cigar"] and (glob or "I" not in tr["cigar"]) and "-" in tr["cons_x"]
    for p, run, tr in _of(family, "none"):
        if family in ("local", "band"):
            assert _empty(run) and _empty(tr) and bc.has_job(family, p)
        elif ext:
            assert run["score"] == 0 and run["to_end_y"] == 0 and p.to_end and tr["end_y"] == 0 and tr["end_x"] == p.q_hi - p.q_lo
            assert tr["cons_y"] == "-" * tr["end_x"] and not bc.has_trace_job(family, p, tr)     # the arena no kernel writes
        else:
            assert tr["score"] < 0 and bc.has_trace_job(family, p, tr)
    for p, run, tr in _of(family, "long"):
        assert len(xs[p.q]) == 40 and (not ext or p.to_end)
    for p, run, tr in _of(family, "edge"):
        if pairs:
            assert run["end_y"] == p.hi - p.lo                         # the hit ends in the window's last column
        else:
            assert p.back and (p.q_lo, p.q_hi) == (2, 30) and tr["score"] > 60 and (not ext or p.to_end)
    for p, run, tr in _of(family, "tie"):
        x, w = xs[p.q][:] if pairs else xs[p.q][p.q_lo:p.q_hi], y[p.lo:p.hi]
        if family == "local":
            H = affine_trace_ref.matrices(x, w, **bc.SC)[0]
            assert (H == H.max()).sum() >= 2 and H.max() == 36 and run["score"] == 36 and run["end_x"] == 12
            j = np.argwhere(H.T == H.max())[0]                        # the first maximum in column-major order
            assert (run["end_y"], run["end_x"]) == (int(j[0]), int(j[1]))
        elif family == "band":
            H = affine_trace_ref.matrices(x, w, **bc.SC)[0]           # (the two maxima lie on one diagonal, inside the band)
            assert (H == H.max()).sum() >= 2 and run["score"] == 36 and run["end_x"] == 12
        elif family == "e2e":
            H = affine_e2e_ref.matrices(x, w, **bc.SC)[0]
            row = H[len(x), 1:]
            assert (row == row.max()).sum() >= 2 and run["score"] == 36 and run["end_y"] == int(np.argmax(row)) + 1 and run["end_y"] < 100
        elif ext:
            H = affine_extend_ref.matrices(x, w, **bc.SC)[0]
            assert H[12, 12] == 36 and H[14, 14] == 36 and H.max() == 36 and (run["score"], run["end_x"], run["end_y"]) == (36, 12, 12)
        else:                                                         # global: the one pair of the other kind
            assert (p.blo is None) == (family == "global_band") and bc.has_job(family, p)
    if family == "zdrop":
        rows = np.array([r["rows_done"] for r in bc.records(family)[0]])
        ms = np.array([p.q_hi - p.q_lo for p in bc.entries(family)])
        stopped = {bc.CLASSES[d % 8] for d in np.nonzero(rows < ms)[0]}
        assert "tie" in stopped and "hit" not in stopped and "none" not in stopped, stopped


def test_the_word_bound_list():
    es, (run, tr) = bc.word_entries(), bc.word_records()
    assert len({bc.key(p) for p in es}) == bc.WORD_D and len(bc.word_reads()) <= 64
    rows = np.array([r["rows_done"] for r in run])
    assert ((rows < bc.WORD_ROWS) == (np.arange(bc.WORD_D) % 3 == 1)).all() and (rows[1::3] > 60).all()   # a third of the reads stop early
    assert all("3D" in t["cigar"] for t in tr[2::3])
    for d in range(bc.WORD_D):
        e = (d + bc.WORD_SHIFT) % bc.WORD_D
        assert run[d] != run[e] and tr[d] != tr[e]
    s = bc.word_seq(bc.WORD_N)
    assert len(set(s[:bc.WORD_D].tolist())) == bc.WORD_D and ((bc.word_seq(bc.WORD_N, bc.STRIDE) - s) % bc.WORD_D == (bc.WORD_A * bc.STRIDE) % bc.WORD_D).all()
    assert (bc.WORD_A * bc.STRIDE) % bc.WORD_D == bc.WORD_SHIFT
    # every pair is a job of the rows instance: fewer than 65 536 problems, and still two launches
    assert bc.rows_launches([bc.WORD_ROWS] * bc.WORD_N) == 2 and bc.rows_launches([40] * bc.LAUNCH) == 1
    assert bc.rows_launches([bc.WORD_ROWS] * bc.WORD_PER_LAUNCH) == 1 and bc.rows_launches([bc.WORD_ROWS] * (bc.WORD_PER_LAUNCH + 1)) == 2


def test_the_byte_budget_case():
    """The constructor at 50 rows against the checkers: 'by construction' is itself checked.  And the arithmetic of the group cut."""
    y, xs, wins = bc.budget_case(rows=50, pairs=bc.BUDGET_PAIRS)
    exp = bc.budget_expected(y, xs, wins)
    for x, (lo, hi), e in zip(xs, wins, exp):
        got = affine_trace_ref.trace(x, y[lo:hi], **bc.SC)
        assert {f: got[f] for f in bc.PAIRS_TRACE} == {f: e[f] for f in bc.PAIRS_TRACE}
        got = affine_extend_ref.trace(x, y[lo:hi], False, False, **bc.SC)
        assert {f: got[f] for f in bc.EXT_TRACE} == {f: e[f] for f in bc.EXT_TRACE}
    sizes = [bc.dirs_bytes(bc.BUDGET_ROWS + k, bc.BUDGET_ROWS + k) for k in range(bc.BUDGET_PAIRS)]
    assert sum(sizes[:21]) <= bc.TRACE_BYTES < sum(sizes) and bc.trace_groups(sizes) == [21, 1]
    assert bc.trace_groups([bc.dirs_bytes(30, 50)] * bc.N) == [bc.LAUNCH, bc.N - bc.LAUNCH]
