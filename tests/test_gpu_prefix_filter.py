"""The prefix-row filter in front of the full sweep of a short-read batch on the device: option prefix_min_cols
engages it on references of 200-300 k columns, every field of align_batch is compared with the oracle, with the filter and under
no_prefix, and the counters with the numpy emulation of the rule (tests/prefix_filter.py, checked against the oracle's full
matrices in tests/test_prefix_filter_ref.py): exact counts, not thresholds.

Two things the scoring 3 / -3 / 2 does not allow, and what stands in for them: a copy ONE score unit below another (scores differ by
3, 5 or 6: the second copy here lacks its last base, 3 units below; the one-unit case runs at 5 / -4 / 1 in its own test), and a
CERTIFIED end cell two sub-chunks right of its prefix (the insertion that takes costs more than the bound leaves: `insertion2` is an
offender here, as the emulation says; the certified case runs at 5 / -4 / 1 in test_end_cell_two_sub_chunks_right)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from prefix_filter import LANES, bound, emulate
from row_sampled_fold import SUB

pytestmark = pytest.mark.gpu

R = 19
P = LANES * R
M = 150
FIELDS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")


def _mutate(rng, x, lo, hi, k):
    x = bytearray(x)
    for at in rng.choice(np.arange(lo, hi), k, replace=False):
        x[at] = b"ACGT"[(b"ACGT".index(x[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(x)


def _main_batch(pgs):
    n = 250_000 + 123
    rng = np.random.default_rng(2026)
    y = bytearray(pgs.synth.dna(515, n).tobytes())
    at = lambda s, d: s * SUB + d
    copy = lambda o, m=M: bytes(y[o:o + m])
    reads, names = [], []

    def add(name, x):
        names.append(name); reads.append(x)
    add("exact", copy(at(40, 17)))
    add("exact2", copy(at(333, 200)))
    add("prefix_errors", _mutate(rng, copy(at(90, 60)), 0, P, 6))       # a low prefix value at the true locus
    add("prefix_errors2", _mutate(rng, copy(at(91, 60), 148), 0, P, 8))
    # prefix rows end in the last columns of sub-chunk c, the end cell behind an insertion of 24 / 150 columns in c + 1 / c + 2
    for name, c, ins in (("insertion1", 500, 24), ("insertion2", 600, 150)):
        cut = at(c + 1, -3)
        add(name, copy(cut - P - 2, P + 2) + copy(cut + ins, M - P - 2))
    two = copy(at(700, 5))
    y[at(800, 99):at(800, 99) + M] = two                                  # an equal copy further right: the first wins
    add("two_copies", two)
    three = copy(at(150, 31))
    y[at(120, 7):at(120, 7) + M - 1] = three[:M - 1]                      # a copy without its last base, 3 units below, further LEFT
    add("lower_copy_first", three)
    add("first_columns", copy(0))
    add("last_columns", copy(n - M))
    add("errors", pgs.synth.read_from_ref(np.frombuffer(bytes(y), dtype=np.uint8), 77, M, sub_rate=0.03, indel_rate=0.01)[0].tobytes())
    add("errors146", pgs.synth.read_from_ref(np.frombuffer(bytes(y), dtype=np.uint8), 78, 146, sub_rate=0.02, indel_rate=0.005)[0].tobytes())
    for k in range(3):
        add("random%d" % k, pgs.synth.dna(900 + k, M).tobytes())         # no hit: offenders
    add("short30", copy(at(10, 3), 30))                                 # P rows or fewer: other buckets, swept as ever
    add("short38", copy(at(11, 3), P))
    return names, reads, bytes(y)


@pytest.fixture(scope="module")
def main_case(pgs, oracle):
    names, reads, y = _main_batch(pgs)
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda q: oracle.align(q, y, pgs.F32), reads))
        cap = 64 + 1024 // len(reads)
        emu = list(ex.map(lambda q: emulate(q, y, R, 3.0, -3.0, 2.0, cap) if len(q) > P else None, reads))
    return names, reads, y, exp, emu


def _check(res, exp, names, what):
    for name, got, e in zip(names, res, exp):
        for f in FIELDS:
            assert got[f] == e[f], (what, name, f, got[f], e[f])


def test_filter_against_oracle_and_emulation(pgs, main_case):
    names, reads, y, exp, emu = main_case
    bucket = [e for e in emu if e is not None]
    offenders = sum(1 for e in bucket if e["offender"])
    for name, e in zip(names, emu):
        if e is not None:
            print("%-18s offender=%d %-18s B0=%g evaluated=%s" % (name, e["offender"], e["why"], e["B0"], e["evaluated"][:8]))
    assert {n for n, e in zip(names, emu) if e is not None and e["offender"]} == {"random0", "random1", "random2", "insertion2"}
    assert 2 * offenders <= len(bucket)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 100_000)
        res = ctx.align_batch(reads, y, semantics=pgs.F32)
        path, cnt, kernel = " ".join(ctx.last_path()), ctx.last_counters(), ctx.last_kernel()
        print(path, cnt, kernel["name"])
        _check(res, exp, names, "prefix filter")
        assert "prefix[SL=2,R=19,P=38]" in path and path.index("prefix[") < path.index("score["), path
        assert cnt["prefix_certified"] == len(bucket) - offenders, (cnt, offenders)
        assert cnt["requeried"] == offenders and cnt["whole_batch_again"] == 0, (cnt, offenders)
        # the prefix instance is named; its cells are the cells actually swept: P rows of the bucket's reads, all rows of its offenders
        # and of the reads of other buckets
        swept = sum(len(q) for q, e in zip(reads, emu) if e is None or e["offender"])
        assert "prefix rows" in kernel["name"] and kernel["lanes"] == LANES and kernel["cells"] == len(y) * (P * len(bucket) + swept), kernel
        ctx.set_option("no_prefix")
        res = ctx.align_batch(reads, y, semantics=pgs.F32)
        path, cnt = " ".join(ctx.last_path()), ctx.last_counters()
        _check(res, exp, names, "no_prefix")
        assert "prefix[" not in path and cnt["prefix_certified"] == 0, (path, cnt)
        # the size gate: without prefix_min_cols a reference this short never takes the filter
        ctx.set_option("no_prefix", None)
        ctx.set_option("prefix_min_cols", None)
        ctx.align_batch(reads[:4], y, semantics=pgs.F32)
        assert "prefix[" not in " ".join(ctx.last_path())
    finally:
        ctx.close()


def test_most_reads_offend(pgs, main_case):
    """More than half of the bucket without a hit: the sweep decides for everybody (whole_batch_again), nothing stays certified."""
    names, reads, y, exp, emu = main_case
    keep = [k for k, nm in enumerate(names) if nm in ("exact", "errors", "random0", "random1", "random2", "short30")]
    sub = [reads[k] for k in keep]
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 100_000)
        res = ctx.align_batch(sub, y, semantics=pgs.F32)
        path, cnt = " ".join(ctx.last_path()), ctx.last_counters()
        _check(res, [exp[k] for k in keep], [names[k] for k in keep], "most reads offend")
        assert "prefix[" in path and "whole_again" in path, path
        assert cnt["whole_batch_again"] == 1 and cnt["prefix_certified"] == 0 and cnt["requeried"] == 0, cnt
    finally:
        ctx.close()


def test_reads_at_the_certification_bound(pgs, oracle):
    """B0 one unit above the bound certifies, B0 at the bound is swept again.  The threshold of such a read is one score unit, which
    on a reference over the read's own letters flags every sub-chunk (over the cap: swept again either way), so the reference here
    is over A / C and the two reads over G / T: prefix values are zero away from the planted copies."""
    n = 200_000 + 50
    rng = np.random.default_rng(88)
    y = bytearray(rng.choice(list(b"AC"), n).astype(np.uint8))
    gt = lambda k: bytes(rng.choice(list(b"GT"), k).astype(np.uint8))
    above = gt(117)                                                      # 117 matches: 351 = bound + 1
    y[300 * SUB + 9:300 * SUB + 9 + 117] = above
    at_bound = gt(118)                                                   # 118 matches across two inserted columns: 354 - 4 = 350
    y[500 * SUB + 40:500 * SUB + 40 + 120] = at_bound[:50] + b"A" + at_bound[50:90] + b"C" + at_bound[90:]
    others = [gt(M), gt(M)]
    for k, o in enumerate(others):
        y[(100 + 50 * k) * SUB:(100 + 50 * k) * SUB + M] = o
    reads = [above + b"N" * (M - 117), at_bound + b"N" * (M - 118)] + others
    y = bytes(y)
    exp = [oracle.align(q, y, pgs.F32) for q in reads]
    assert bound(M, R, 3.0, 2.0) == 350 and [e["score"] for e in exp] == [351, 350, 450, 450]
    cap = 64 + 1024 // len(reads)
    emu = [emulate(q, y, R, 3.0, -3.0, 2.0, cap) for q in reads]
    assert [e["offender"] for e in emu] == [False, True, False, False], [(e["offender"], e["why"], e["B0"]) for e in emu]
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 100_000)
        res = ctx.align_batch(reads, y, semantics=pgs.F32)
        cnt = ctx.last_counters()
        _check(res, exp, ["above", "at_bound", "copy0", "copy1"], "bound")
        assert cnt["requeried"] == 1 and cnt["prefix_certified"] == 3 and cnt["whole_batch_again"] == 0, cnt
    finally:
        ctx.close()


def _run_and_count(pgs, reads, y, exp, emu, names, scoring, what):
    """align_batch with the filter engaged: every field against the oracle, the three counters exactly as the emulation says."""
    offenders = sum(1 for e in emu if e["offender"])
    assert 2 * offenders <= len(emu)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 100_000)
        res = ctx.align_batch(reads, y, semantics=pgs.F32, match=scoring[0], mismatch=scoring[1], gap=scoring[2])
        path, cnt = " ".join(ctx.last_path()), ctx.last_counters()
    finally:
        ctx.close()
    print(what, path, cnt)
    _check(res, exp, names, what)
    assert "prefix[SL=2,R=19,P=38]" in path, path
    assert (cnt["prefix_certified"], cnt["requeried"], cnt["whole_batch_again"]) == (len(emu) - offenders, offenders, 0), (cnt, offenders)


def test_one_unit_below(pgs, oracle):
    """5 / -4 / 1: a copy with one inserted column, further left, scores one unit below the exact copy that follows it; the read is
    settled by the filter (both copies are among the evaluated sub-chunks), not by the sweep."""
    scoring = (5.0, -4.0, 1.0)
    n = 200_000 + 9
    y = bytearray(pgs.synth.dna(616, n).tobytes())
    reads = [bytes(y[o:o + M]) for o in (400 * SUB + 77, 90 * SUB + 1, 650 * SUB + 200, 30 * SUB + 5)]
    x = reads[0]
    y[100 * SUB + 30:100 * SUB + 30 + M + 1] = x[:70] + b"A" + x[70:]     # further left, 749
    y = bytes(y)
    exp = [oracle.align(q, y, pgs.F32, *scoring) for q in reads]
    assert exp[0]["score"] == 750 and exp[0]["end_y"] == 400 * SUB + 77 + M
    cap = 64 + 1024 // len(reads)
    emu = [emulate(q, y, R, *scoring, cap) for q in reads]
    assert not emu[0]["offender"] and emu[0]["result"] == (750.0, M, 400 * SUB + 77 + M), emu[0]
    assert {100, 400} <= set(emu[0]["evaluated"])                      # both copies are evaluated on all rows
    _run_and_count(pgs, reads, y, exp, emu, ["copy%d" % k for k in range(4)], scoring, "one unit below")


def test_end_cell_two_sub_chunks_right(pgs, oracle):
    """The prefix rows end in the last columns of sub-chunk c, the end cell behind an insertion of 150 columns in c + 2, and the read is
    CERTIFIED: at 5 / -4 / 1 the insertion costs 150, B = 600 is above the bound 567.  Its threshold is 33, which a reference over the
    read's own letters reaches in most sub-chunks (over the cap), so the reference is over A / C and the reads over G / T."""
    scoring = (5.0, -4.0, 1.0)
    n = 200_000 + 31
    rng = np.random.default_rng(99)
    y = bytearray(rng.choice(list(b"AC"), n).astype(np.uint8))
    gt = lambda k: bytes(rng.choice(list(b"GT"), k).astype(np.uint8))
    c = 300
    far = gt(M)
    cut = (c + 1) * SUB - 3                                              # the first P + 2 rows end here, in sub-chunk c
    y[cut - (P + 2):cut] = far[:P + 2]
    y[cut + 150:cut + 150 + M - P - 2] = far[P + 2:]                     # ... the other rows behind 150 columns of A / C
    others = [gt(M), gt(M), gt(140)]
    for k, o in enumerate(others):
        y[(100 + 50 * k) * SUB + 11:(100 + 50 * k) * SUB + 11 + len(o)] = o
    reads = [far] + others
    y = bytes(y)
    exp = [oracle.align(q, y, pgs.F32, *scoring) for q in reads]
    assert bound(M, R, 5.0, 1.0) == 567 and exp[0]["score"] == 600 and (exp[0]["end_y"] - 1) // SUB == c + 2, exp[0]
    cap = 64 + 1024 // len(reads)
    emu = [emulate(q, y, R, *scoring, cap) for q in reads]
    assert [e["offender"] for e in emu] == [False] * 4, [(e["offender"], e["why"], e["B0"]) for e in emu]
    assert emu[0]["result"] == (600.0, M, exp[0]["end_y"]) and int(np.flatnonzero(emu[0]["values"] == emu[0]["values"].max())[0]) == c
    _run_and_count(pgs, reads, y, exp, emu, ["far", "copy0", "copy1", "copy140"], scoring, "end cell in c + 2")


@pytest.mark.parametrize("what", ["u8", "fractional"])
def test_other_engines_do_not_engage(pgs, oracle, main_case, what):
    names, reads, y, exp, emu = main_case
    sub = reads[:4]
    kw = dict(semantics=pgs.U8SAT) if what == "u8" else dict(semantics=pgs.F32, match=3.5, mismatch=-3.25, gap=2.0)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 100_000)
        res = ctx.align_batch(sub, y, **kw)
        path, cnt = " ".join(ctx.last_path()), ctx.last_counters()
        assert "prefix[" not in path and cnt["prefix_certified"] == 0, (path, cnt)
        with ThreadPoolExecutor(4) as ex:
            e2 = list(ex.map(lambda q: oracle.align(q, y, kw["semantics"], kw.get("match", 3.0), kw.get("mismatch", -3.0), kw.get("gap", 2.0)), sub))
        _check(res, e2, names[:4], what)
    finally:
        ctx.close()
