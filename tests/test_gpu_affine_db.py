"""Affine-gap database search against a short reference on the device: sw_affine_prof_kernel behind mi355_sw_affine_* for
references (ranges) of at most 512 letters, and the row window of the affine traceback (lemma L18).  Checked for
equality of every field against tests/affine_ref.py (score, end cell) and tests/affine_trace_ref.py (pos, both consensus strings,
begin cell, CIGAR): every reference length at which the kernel instance or its padding changes, sequence lengths around the slot's
skew and the 64-row segment refill, batch sizes around a slot and a workgroup, planted gaps across lane boundaries, whole lanes and
segment refills, ties, scorings up to the bound of the tracking key, per-range maxima, long sequences that the exact kernel's LDS
does not hold, and every case that the former path can compute once more under option no_affine_prof.

A range takes the new kernel when its problems hold at least 2^18 cells in all (MIN_CELLS below; smaller calls stay on the exact
kernel): `fill` adds unrelated sequences of at most 1 000 rows to a batch until it does.  Expected values are computed once per
module."""
import numpy as np
import pytest

from tests import affine_ref, affine_trace_ref as tr, score_instances as si

pytestmark = pytest.mark.gpu

ENOTSUP = -95
MIN_CELLS = 1 << 18
DEFAULT = (3, -3, 5, 1)
FIELDS = ("score", "end_x", "end_y", "pos", "cons_x", "cons_y", "begin_x", "begin_y", "cigar")
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
AA = np.frombuffer(si.AA20, dtype=np.uint8)

_cache = {}


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def kw(sc, lut=None):
    return dict(match=float(sc[0]), mismatch=float(sc[1]), gap_open=float(sc[2]), gap_extend=float(sc[3]), lut=lut)


def expected_R(n):
    return 9 if n <= 144 else 10 if n <= 160 else 20 if n <= 320 else 32


def rand(rng, n, alpha=DNA):
    return alpha[rng.integers(0, len(alpha), n)].tobytes()


def mutate(rng, s, alpha=DNA, rate=0.06):
    """A copy of s with substitutions and single-letter indels."""
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(alpha[rng.integers(0, len(alpha))]))
        out.append(c if u > rate else int(alpha[rng.integers(0, len(alpha))]))
    return bytes(out)


def fill(rng, xs, n, alpha=DNA):
    """xs and as many unrelated sequences of 600 .. 1 000 rows as the batch needs to hold MIN_CELLS cells against n columns."""
    xs = list(xs)
    rows = sum(len(x) for x in xs)
    while rows * n < MIN_CELLS:
        m = int(rng.integers(600, 1001))
        xs.append(rand(rng, m, alpha))
        rows += m
    return xs


def locate(key, xs, y, sc=DEFAULT, lut=None):
    if key not in _cache:
        _cache[key] = affine_ref.locate_batch(xs, y, *sc, lut=lut)
    return _cache[key]


def traces(key, xs, y, sc=DEFAULT, lut=None):
    if key not in _cache:
        _cache[key] = tr.trace_batch(xs, y, *sc, lut=lut)
    return _cache[key]


def score_run(ctx, xs, y, sc=DEFAULT, lut=None, option=None):
    """(dict of arrays, path) of affine_batch_run, under `option` if given (reset afterwards)."""
    if option:
        ctx.set_option(option, 1)
    try:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
        got = ctx.affine_batch_run(**kw(sc, lut))
        path = ctx.last_path()
    finally:
        if option:
            ctx.set_option(option, 0)
    return got, path


def trace_run(ctx, xs, y, sc=DEFAULT, lut=None, option=None):
    if option:
        ctx.set_option(option, 1)
    try:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
        got = ctx.affine_batch_trace(**kw(sc, lut))
        path = ctx.last_path()
    finally:
        if option:
            ctx.set_option(option, 0)
    n = len(got["cons_x"])
    rows = [{k: (got[k][q] if isinstance(got[k], list) else got[k][q].item()) for k in FIELDS} for q in range(n)]
    return rows, path


def check_scores(got, exp, what=""):
    es, ei, ej = exp
    bad = [(k, float(got["score"][k]), int(got["end_x"][k]), int(got["end_y"][k]), float(es[k]), int(ei[k]), int(ej[k]))
           for k in range(len(es)) if (got["score"][k], got["end_x"][k], got["end_y"][k]) != (es[k], ei[k], ej[k])]
    assert not bad, (what, bad[:4])


def check_traces(got, exp, ids=None):
    ids = range(len(exp)) if ids is None else ids
    bad = [(q, k, got[q][k], e[k]) for q, e in zip(ids, exp) for k in FIELDS if got[q][k] != e[k]]
    assert not bad, bad[:4]


def prof_tags(path):
    return [t for t in path if t.startswith("affine_prof[")]


def both_ways(ctx, xs, y, exp, sc=DEFAULT, lut=None, R=None):
    """The batch on the new kernel and once more on the former path: equal to the checker and to each other, the tag where it
    belongs."""
    got, path = score_run(ctx, xs, y, sc, lut)
    assert prof_tags(path) == ["affine_prof[R=%d]" % (R or expected_R(len(y)))] and "affine_exact" not in path, path
    check_scores(got, exp, "affine_prof")
    old, path = score_run(ctx, xs, y, sc, lut, option="no_affine_prof")
    assert not prof_tags(path) and "affine_exact" in path, path
    check_scores(old, exp, "no_affine_prof")
    return got


# ---- reference lengths: R 9 -> 10 -> 20 -> 32, padding columns, one column --------------------------------------------------------
def _reference_case(n):
    rng = np.random.default_rng(9100 + n)
    y = rand(rng, n)
    xs = [mutate(rng, y), rand(rng, 40) + y + rand(rng, 25), y[n // 2:] + rand(rng, 70), b"", rand(rng, 33) + y[:max(1, n // 3)]]
    xs += [rand(rng, m) for m in (1, 17, 65, 130)]
    return fill(rng, xs, n), y


@pytest.mark.parametrize("n", [1, 8, 9, 143, 144, 145, 160, 161, 320, 321, 512])
def test_reference_lengths(ctx, n):
    xs, y = _reference_case(n)
    exp = locate(("ref", n), xs, y)
    assert exp[0][1] == 3.0 * n and exp[2][1] == n                  # the exact copy ends in the last column of y
    both_ways(ctx, xs, y, exp)


def test_reference_of_513_letters_is_not_taken(ctx):
    xs, y = _reference_case(513)
    got, path = score_run(ctx, xs, y)
    assert not prof_tags(path) and "affine_exact" in path, path
    check_scores(got, locate(("ref", 513), xs, y))


def test_small_calls_stay_on_the_exact_kernel(ctx):
    rng = np.random.default_rng(9001)
    y = rand(rng, 144)
    xs = [mutate(rng, y), rand(rng, 129), b"", y[30:90]]           # 413 rows x 144 columns: below 2^18 cells
    got, path = score_run(ctx, xs, y)
    assert not prof_tags(path) and "affine_exact" in path, path
    check_scores(got, locate("small", xs, y))


# ---- sequence lengths: the slot's skew, segment refill and history, no rows at all ------------------------------------------------
def _length_case():
    rng = np.random.default_rng(9200)
    y = rand(rng, 144)
    lens = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 0, 144, 200]
    xs = []
    for m in lens:
        at = int(rng.integers(0, max(1, 144 - m)))
        xs.append((mutate(rng, (y + y)[at:at + m]) + rand(rng, m))[:m])
        assert len(xs[-1]) == m
    return fill(rng, xs, 144), y, lens


def test_sequence_lengths(ctx):
    xs, y, lens = _length_case()
    exp = locate("lengths", xs, y)
    got = both_ways(ctx, xs, y, exp)
    k = lens.index(0)
    assert (got["score"][k], got["end_x"][k], got["end_y"][k]) == (0.0, 0, 0)
    assert all(exp[0][q] > 0 for q, m in enumerate(lens) if m)


def _long_x(rows=6000, at=4000):
    rng = np.random.default_rng(9300)
    y = rand(rng, 144)
    x = bytearray(rand(rng, rows))
    copy = y[10:70] + rand(rng, 4) + y[70:140]                      # four rows of x against a gap
    x[at:at + len(copy)] = copy
    return bytes(x), y


def test_6000_rows_against_144_columns(ctx, pgs):
    """The exact kernel's LDS diagonals hold about 5 600 rows: without sw_affine_prof_kernel this input is refused."""
    x, y = _long_x()
    exp = locate("long6000", [x], y)
    assert exp[0][0] >= 3 * 130 - 8 - 30 and 4100 < exp[1][0] <= 4140
    got, path = score_run(ctx, [x], y)
    assert prof_tags(path) == ["affine_prof[R=9]"], path
    check_scores(got, exp)
    with pytest.raises(pgs.MI355Error) as e:
        score_run(ctx, [x], y, option="no_affine_prof")
    assert e.value.code == ENOTSUP
    one = ctx.affine_align(x, y)                                    # the single-alignment call takes the same kernel
    assert prof_tags(ctx.last_path()) == ["affine_prof[R=9]"]
    assert (one["score"], one["end_x"], one["end_y"]) == (exp[0][0], exp[1][0], exp[2][0])


# ---- batch sizes: one slot, a workgroup and one more, two and one more, and a few hundred of mixed lengths -------------------------
@pytest.mark.parametrize("count", [1, 16, 17, 33, 300])
def test_batch_sizes(ctx, count):
    rng = np.random.default_rng(9400 + count)
    y = rand(rng, 144)
    if count == 1:
        xs = [rand(rng, 900) + mutate(rng, y) + rand(rng, 900)]
    else:
        hi = 700 if count == 300 else 420
        lens = [int(v) for v in rng.integers(0, hi, count)]         # (unsorted, some of them empty: the id mapping)
        lens[count // 2] = 0
        xs = [mutate(rng, (y + y)[m % 90:m % 90 + m])[:m] if k % 3 else rand(rng, m) for k, m in enumerate(lens)]
        assert sum(len(x) for x in xs) * 144 >= MIN_CELLS
    exp = locate(("batch", count), xs, y)
    both_ways(ctx, xs, y, exp)
    got, _ = score_run(ctx, xs, y)
    t = ctx.last_timings()
    assert t["score_launches"] >= 1 and t["cells"] == float(sum(len(x) for x in xs) * 144) and t["score_us"] > 0
    k = ctx.last_kernel()
    assert k["cells"] == t["cells"] and k["lanes"] == 16 and k["rows_per_lane"] == 9 and k["valu_ops_per_cell"] > 7
    assert k["name"].startswith("sw_affine_prof_kernel<R=9")


# ---- planted alignments -----------------------------------------------------------------------------------------------------------
N10 = b"N" * 10                                                     # a letter no reference here has
N40 = b"N" * 40                                                     # ... as many rows as no gap pays for: two copies stay two alignments


def _planted(n):
    """(queries, reference of n >= 144 letters, names): rows per lane R = 9 (n = 144) or 10 (n = 150: six padding columns)."""
    rng = np.random.default_rng(9500 + n)
    R = expected_R(n)
    y = rand(rng, n)
    b = 3 * R                                                       # first column (0-based) of lane 3
    cases = {
        # letters b - 1 .. b + 1 of y skipped: a gap in x across the lane boundary
        "gap_across_lanes": y[b - 22:b - 1] + y[b + 2:b + 40],
        # R + 3 letters of y skipped: the gap spans a whole lane
        "gap_spans_lane": y[40:40 + 2 * R] + y[43 + 3 * R:43 + 3 * R + 45],
        # nine rows of x against a gap, rows 60 .. 68: across the refill of the 64-row segment
        "rows_across_refill": N10 * 2 + y[10:50] + rand(rng, 9) + y[50:100],
        # ... and rows 125 .. 131 of a longer one
        "rows_across_second_refill": N10 * 8 + y[5:50] + rand(rng, 7) + y[50:110] + N10,
        "ends_in_last_column": N10 + y[n - 50:],
        "ends_in_last_row": N10 * 3 + y[30:80],
        # equal maxima in one column, two rows
        "tie_same_column": y[20:60] + N40 + y[20:60] + N10,
        # equal maxima in two lanes, the later column at the earlier row
        "tie_later_column_first": y[80:120] + N40 + y[20:60],
        # ... and in two columns of one lane
        "tie_same_lane": y[6 * R - 34:6 * R + 6] + N40 + y[6 * R - 38:6 * R + 2],
        "no_match": N10 * 5,
    }
    names = list(cases)
    return fill(rng, [cases[k] for k in names], n), y, names


@pytest.mark.parametrize("n", [144, 150])
def test_planted_alignments(ctx, n):
    xs, y, names = _planted(n)
    k = {name: q for q, name in enumerate(names)}
    exp = locate(("planted", n), xs, y)
    both_ways(ctx, xs, y, exp)
    ext = traces(("planted_trace", n), xs[:len(names)], y)
    # the checker's own answers show that the planted features are there
    R = expected_R(n)
    assert "3D" in ext[k["gap_across_lanes"]]["cigar"] and "%dD" % (R + 3) in ext[k["gap_spans_lane"]]["cigar"]
    assert "9I" in ext[k["rows_across_refill"]]["cigar"] and "7I" in ext[k["rows_across_second_refill"]]["cigar"]
    assert ext[k["rows_across_refill"]]["begin_x"] == 21 and ext[k["rows_across_second_refill"]]["begin_x"] == 81
    assert ext[k["ends_in_last_column"]]["end_y"] == n and ext[k["ends_in_last_row"]]["end_x"] == len(xs[k["ends_in_last_row"]])
    assert (ext[k["tie_same_column"]]["score"], ext[k["tie_same_column"]]["end_x"], ext[k["tie_same_column"]]["end_y"]) == (120.0, 40, 60)
    assert (ext[k["tie_later_column_first"]]["score"], ext[k["tie_later_column_first"]]["end_x"], ext[k["tie_later_column_first"]]["end_y"]) == (120.0, 120, 60)
    assert (ext[k["tie_same_lane"]]["score"], ext[k["tie_same_lane"]]["end_x"], ext[k["tie_same_lane"]]["end_y"]) == (120.0, 120, 6 * R + 2)
    assert ext[k["no_match"]]["score"] == 0
    got, path = trace_run(ctx, xs, y)
    assert prof_tags(path) == ["affine_prof[R=%d]" % R] and "affine_trace" in path, path
    check_traces(got, ext)
    for g in got:
        assert tr.rescore(g["cons_x"], g["cons_y"], *DEFAULT) == g["score"]
    old, path = trace_run(ctx, xs, y, option="no_affine_prof")
    assert not prof_tags(path) and "affine_exact" in path, path
    assert old == got


# ---- scorings ---------------------------------------------------------------------------------------------------------------------
def test_linear_special_case(ctx, pgs, oracle):
    xs, y, _ = _length_case()
    sc = (3, -3, 2, 2)
    exp = locate("lengths_linear", xs, y, sc)
    got = both_ways(ctx, xs, y, exp, sc)
    lin = ctx.batch_run(match=3.0, mismatch=-3.0, gap=2.0, flags=pgs.capi.SCORE_ONLY)
    for q, x in enumerate(xs):
        mine = (float(got["score"][q]), int(got["end_x"][q]), int(got["end_y"][q]))
        assert mine == (lin[q]["score"], lin[q]["end_x"], lin[q]["end_y"]), (q, mine, lin[q])
        if x and q < 16:
            o = oracle.locate(x, y, 0, match=3.0, mismatch=-3.0, gap=2.0)
            assert mine == (float(o[0]), int(o[1]), int(o[2])), (q, mine, o)


def _table(seed, symmetric):
    rng = np.random.default_rng(seed)
    t = rng.integers(-4, 12, (20, 20))
    if symmetric:
        t = np.triu(t) + np.triu(t, 1).T
    t[np.arange(20), np.arange(20)] = rng.integers(4, 12, 20)
    lut = np.full((256, 256), -4.0, dtype=np.float32)
    lut[np.ix_(AA, AA)] = t
    assert symmetric or not np.array_equal(lut, lut.T)
    return lut


def _protein_case(seed):
    rng = np.random.default_rng(seed)
    y = rand(rng, 144, AA)
    xs = [mutate(rng, y, AA, 0.15), rand(rng, 30, AA) + y[20:80] + rand(rng, 6, AA) + y[80:130], y[40:70] + y[78:144], rand(rng, 200, AA),
          b"BZX" * 20 + y[60:100] + b"-*" * 9, rand(rng, 129, AA), b"J" * 70]
    return fill(rng, xs, 144, AA), y


@pytest.mark.parametrize("symmetric", [True, False], ids=["table_11_1", "asymmetric_table"])
def test_table_scoring(ctx, symmetric):
    xs, y = _protein_case(9600)
    lut = _table(9601 + symmetric, symmetric)
    sc = (0, 0, 11, 1)
    exp = locate(("table", symmetric), xs, y, sc, lut)
    both_ways(ctx, xs, y, exp, sc, lut)
    ext = traces(("table_trace", symmetric), xs[:7], y, sc, lut)
    assert "I" in ext[1]["cigar"] and "D" in ext[2]["cigar"] and ext[6]["score"] == 0
    got, path = trace_run(ctx, xs, y, sc, lut)
    assert prof_tags(path) == ["affine_prof[R=9]"], path
    check_traces(got, ext)
    for g in got:
        assert tr.rescore(g["cons_x"], g["cons_y"], *sc, lut=lut) == g["score"]


def test_letters_that_the_other_side_lacks(ctx):
    rng = np.random.default_rng(9700)
    y = rand(rng, 160, np.frombuffer(b"ACGTT", dtype=np.uint8))
    ax = np.frombuffer(b"ACGNX", dtype=np.uint8)                    # x has no T, y has no N and no X
    xs = fill(rng, [rand(rng, m, ax) for m in (5, 64, 129, 300)] + [y[:80].replace(b"T", b"N")], 160, ax)
    both_ways(ctx, xs, y, locate("lacks", xs, y))


def test_key_bound_from_both_sides(ctx, pgs):
    rng = np.random.default_rng(9800)
    y = rand(rng, 511)
    xs = [rand(rng, 20) + y + rand(rng, 20), mutate(rng, y[100:400])]
    assert sum(len(x) for x in xs) * 511 >= MIN_CELLS
    sc = (511, -400, 700, 9)                                        # smax * (n + 1) = 2^18 - 512: taken
    exp = locate("bound511", xs, y, sc)
    assert exp[0][0] == 511.0 * 511
    both_ways(ctx, xs, y, exp, sc)
    sc = (512, -400, 700, 9)                                        # 2^18: not taken; right, or refused where it was before
    try:
        got, path = score_run(ctx, xs, y, sc)
    except pgs.MI355Error as e:
        assert e.code == ENOTSUP
        with pytest.raises(pgs.MI355Error):
            score_run(ctx, xs, y, sc, option="no_affine_prof")
    else:
        assert not prof_tags(path), path
        check_scores(got, locate("bound512", xs, y, sc))
    sc = (3, -3, 1 << 18, 1)                                        # gap_open = 2^18: not taken either
    got, path = score_run(ctx, xs, y, sc)
    assert not prof_tags(path), path
    check_scores(got, locate("open2^18", xs, y, sc))


# ---- per-range maxima -------------------------------------------------------------------------------------------------------------
def test_score_ranges_short_and_long(ctx):
    rng = np.random.default_rng(9900)
    ref = bytearray(rand(rng, 4200))
    xs = [rand(rng, int(m)) for m in rng.integers(1, 400, 24)] + [b""]
    ranges = [(3, 147), (500, 1012), (1300, 1600), (1801, 3801)]     # 144, 512 and 300 columns, and 2 000
    for q, (lo, hi) in zip((0, 5, 9, 13), ranges):
        ref[lo + 20:lo + 20 + min(len(xs[q]), hi - lo - 40)] = xs[q][:hi - lo - 40]
    ref = bytes(ref)
    assert sum(len(x) for x in xs) * 144 >= MIN_CELLS
    ctx.set_reference(ref)
    ctx.batch_upload(xs)
    mx = ctx.affine_score_ranges(ranges)
    path = ctx.last_path()
    assert prof_tags(path) == ["affine_prof[R=9]", "affine_prof[R=32]", "affine_prof[R=20]"], path
    assert any(t.startswith("affine[cell=f16") for t in path), path
    exp = np.array([affine_ref.locate_batch(xs, ref[lo:hi])[0] for lo, hi in ranges])
    assert np.array_equal(mx.astype(np.float64), exp), (mx.tolist(), exp.tolist())
    t = ctx.last_timings()
    assert t["score_launches"] >= 4 and t["cells"] == float(sum(len(x) for x in xs) * (144 + 512 + 300 + 2000))
    ctx.set_option("no_affine_prof", 1)
    try:
        old = ctx.affine_score_ranges(ranges)
        path = ctx.last_path()
    finally:
        ctx.set_option("no_affine_prof", 0)
    assert not prof_tags(path) and "affine_exact" in path, path
    assert np.array_equal(old, mx)


def test_score_ranges_all_three_stages_write_one_array(ctx):
    """One call in which sw_affine_prof_kernel, the sweep and the exact kernel each write part of one `maxima` array: ranges on both
    sides of the sweep's 1 024 columns and a query beyond its 512 rows.  The 700-column range is the exact kernel's for every query,
    the 600-row query on the 2 000-column range as well."""
    rng = np.random.default_rng(9901)
    ref = bytearray(rand(rng, 4200))
    xs = [rand(rng, int(m)) for m in rng.integers(1, 400, 24)] + [b"", rand(rng, 600)]
    ranges = [(3, 147), (500, 1012), (1300, 1600), (1801, 3801), (3400, 4100)]   # 144, 512 and 300 columns, 2 000 and 700
    for q, (lo, hi) in zip((0, 5, 9, 13, 25), ranges):
        ref[lo + 20:lo + 20 + min(len(xs[q]), hi - lo - 40)] = xs[q][:hi - lo - 40]
    ref = bytes(ref)
    assert sum(len(x) for x in xs) * 144 >= MIN_CELLS
    exp = np.array([affine_ref.locate_batch(xs, ref[lo:hi])[0] for lo, hi in ranges])
    assert exp.max(axis=1).tolist() == [315, 975, 348, 1143, 1800] and not exp[:, 24].any()
    ctx.set_reference(ref)
    ctx.batch_upload(xs)
    mx = ctx.affine_score_ranges(ranges)
    path = ctx.last_path()
    assert np.array_equal(mx.astype(np.float64), exp), (mx.tolist(), exp.tolist())
    assert prof_tags(path) == ["affine_prof[R=9]", "affine_prof[R=32]", "affine_prof[R=20]"], path
    assert any(t.startswith("affine[cell=f16") for t in path) and "affine_exact" in path, path
    ctx.set_option("no_affine_prof", 1)
    try:
        old = ctx.affine_score_ranges(ranges)
    finally:
        ctx.set_option("no_affine_prof", 0)
    assert np.array_equal(old.astype(np.float64), exp), (old.tolist(), exp.tolist())


# ---- traceback: the row window ----------------------------------------------------------------------------------------------------
def _row_window_case():
    x6, y = _long_x()
    rng = np.random.default_rng(9950)
    x3 = bytearray(rand(rng, 3000))
    copy = y[20:75] + y[79:130]                                     # ends near row 2 500; four letters of y against a gap
    x3[2400:2400 + len(copy)] = copy
    x20 = y[50:70] + b"N" * 1980                                    # ends in row 20: the window is the matrix's first rows
    return [bytes(x3), x20, x6], y


def test_traceback_row_window(ctx, pgs):
    xs, y = _row_window_case()
    exp = traces("row_window", xs, y)
    assert 2490 < exp[0]["end_x"] <= 2530 and "4D" in exp[0]["cigar"] and (exp[1]["end_x"], exp[1]["cigar"]) == (20, "20M")
    assert 4100 < exp[2]["end_x"] <= 4140 and "4I" in exp[2]["cigar"]
    got, path = trace_run(ctx, xs, y)
    assert prof_tags(path) == ["affine_prof[R=9]"] and "affine_trace" in path, path
    check_traces(got, exp)
    for g in got:
        assert tr.rescore(g["cons_x"], g["cons_y"], *DEFAULT) == g["score"]
    one = ctx.affine_align_trace(xs[2], y)
    assert prof_tags(ctx.last_path()) == ["affine_prof[R=9]"]
    check_traces([one], exp[2:])
    # the two that the exact kernel's LDS holds, once more on the former path: the same bytes
    old, path = trace_run(ctx, xs[:2], y, option="no_affine_prof")
    assert not prof_tags(path) and "affine_exact" in path and "affine_trace" in path, path
    assert old == got[:2]
    with pytest.raises(pgs.MI355Error) as e:
        trace_run(ctx, xs, y, option="no_affine_prof")
    assert e.value.code == ENOTSUP
