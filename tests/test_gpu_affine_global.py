"""The global alignment between two anchors on the device (mi355_sw_affine_global_run / _trace) against tests/affine_global_ref.py
applied to the letters x[q_lo:q_hi] and the slice y[left:right].  Every case runs through every dispatch — the default one
(sw_affine_pair_glob_kernel / sw_affine_band_glob_kernel where they admit the pair), option no_affine_pairs (the exact kernel) and,
where a pair is banded, option no_affine_band — and through both calls, run and trace: every field and both strings must equal the
checker, the strings must be worth the score, and the path must show which kernel ran: never an extension, local or end-to-end tag,
"affine_trace" only in trace calls.  Scores are integers: no tolerance.  Expected values are computed once per case.

Three mutations of the new code, and the cases that fail under each (decided on the CPU by the checker where it can be, and then
asserted here, so that the cases keep that power):

  * the corner replaced by the row-m maximum (the extension's to-end fold): every pair with score != to_end_score.
    test_every_pair_instance_and_its_edges asserts that for the window of m + 40 columns of each row count (m >= 31),
    test_capture_not_last_value for its windows of 400 and 1000 columns, test_against_the_extension_on_the_device for most of its
    49 windows, test_gap_heavy_answers for the removed-block pair;
  * the floor left on (a clamp in the cell, or max(H, 0) on the answer): every pair with score < 0 or a negative cell on its
    best path.  test_gap_heavy_answers asserts score < 0 for the unrelated strings, test_degenerate_and_unreachable_pairs and the
    short windows (1, 2 columns against 31 and more rows) of test_every_pair_instance_and_its_edges have negative answers too;
  * the capture one column late (t == n instead of t == n - 1; the band kernel: the register of diagonal n - m + 1): the value read
    is that of a padding cell or of the neighbour H(m, n + 1) — a padding cell is strictly below a real one, so every pair that runs
    on the pair kernel fails, in every test here but the host-filled ones; in the band kernel the neighbouring register is out of
    band (-inf) where n - m == hi_e, which test_every_band_instance places in each instance, and another cell elsewhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import affine_extend_band_ref as BR
from tests import affine_extend_ref as ER
from tests import affine_global_ref as G

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
NINF = float("-inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
FIELDS = ("score", "end_x", "end_y", "pos", "cons_x", "cons_y", "cigar")
STRINGS = ("cons_x", "cons_y", "cigar")
FOREIGN = ("affine_pair[", "affine_pair_e2e", "affine_pair_ext", "affine_band[", "affine_band_ext", "affine_prof", "affine[")


def _listed(name, header):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+int\s+%s\[\]\s*=\s*\{([^}]*)\}" % name, f.read())
    return tuple(int(v) for v in m.group(1).split(","))


PAIR_R = _listed("kPairR", "sw_affine_pair_kernel.h")
BAND_R = _listed("kBandR", "sw_affine_band_kernel.h")


def pair_R(m):
    return min(r for r in PAIR_R if 16 * r >= m)


def band_R(W):
    return min(r for r in BAND_R if 16 * r >= W)


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


class Scoring:
    def __init__(self, name, match=3, mismatch=-3, gap_open=5, gap_extend=1, lut=None):
        self.name, self.match, self.mismatch, self.open, self.ext, self.lut = name, match, mismatch, gap_open, gap_extend, lut

    def kw(self):
        return dict(match=float(self.match), mismatch=float(self.mismatch), gap_open=float(self.open), gap_extend=float(self.ext), lut=self.lut)


DEFAULT = Scoring("3/-3/5/1")
HARD_MISMATCH = Scoring("3/-10/5/1", 3, -10, 5, 1)
LINEAR = Scoring("2/-4/3/3", 2, -4, 3, 3)


def dna(rng, n, letters="ACGT"):
    return "".join(letters[v] for v in rng.integers(0, len(letters), n))


def mutate(rng, s, rate=0.08, letters="ACGT"):
    """A copy of s with substitutions, short insertions and short deletions."""
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(letters[rng.integers(0, len(letters))])
        out.append(ch if u > rate else letters[rng.integers(0, len(letters))])
    return "".join(out)


class Pair:
    """One pair of a list: query q, its letters [q_lo, q_hi) (None: all), the window [lo, hi), the direction, the band (None: none)."""
    def __init__(self, q, lo, hi, q_lo=None, q_hi=None, back=0, band=None):
        self.q, self.lo, self.hi, self.q_lo, self.q_hi, self.back, self.band = q, lo, hi, q_lo, q_hi, back, band

    def letters(self, xs):
        x = xs[self.q]
        return x if self.q_lo is None else x[self.q_lo:self.q_hi]

    def kind(self, xs):
        """Where the header sends the pair under an admitted scoring: "host", "pair", "band", "exact" or "exact_band", and its R."""
        m, n = len(self.letters(xs)), self.hi - self.lo
        if m < 1 or n < 1 or not G.reachable(m, n, *(self.band or (None, None))):
            return "host", 0
        lo_e, hi_e = (max(self.band[0], -m), min(self.band[1], n)) if self.band else (-m, n)
        if (lo_e, hi_e) == (-m, n):
            return ("pair", pair_R(m)) if m <= 512 else ("exact", 0)
        W = hi_e - lo_e + 1
        return ("band", band_R(W)) if m <= 512 and W <= 256 else ("exact_band", 0)


def expected(xs, y, pairs, sc):
    rows = [G.trace(p.letters(xs), y[p.lo:p.hi], *(p.band or (None, None)), backward=bool(p.back), **sc.kw()) for p in pairs]
    return {f: ([r[f] for r in rows] if f in STRINGS else np.array([r[f] for r in rows], dtype=np.float64)) for f in FIELDS}


def same(got, exp, fields):
    for f in fields:
        a, b = got[f], exp[f]
        ok = np.array_equal(np.asarray(a, dtype=np.float64), b) if isinstance(b, np.ndarray) else list(a) == list(b)
        assert ok, (f, [(k, u, v) for k, (u, v) in enumerate(zip(a, b)) if u != v][:5])


def call_args(pairs):
    ranged = any(p.q_lo is not None for p in pairs)
    assert not ranged or all(p.q_lo is not None for p in pairs)
    kw = dict(backward=[p.back for p in pairs] if any(p.back for p in pairs) else None)
    if any(p.band for p in pairs):
        big = 1 << 40                                                 # a pair without a band in a banded list: a band that covers everything
        kw.update(band_lo=[p.band[0] if p.band else -big for p in pairs], band_hi=[p.band[1] if p.band else big for p in pairs])
    if ranged:
        kw.update(q_lo=[p.q_lo for p in pairs], q_hi=[p.q_hi for p in pairs])
    return [p.q for p in pairs], [p.lo for p in pairs], [p.hi for p in pairs], kw


def kernel_tags(path):
    return sorted(t for t in path if t.startswith("affine") and t != "affine_trace")


def tags_for(kinds, option):
    out = set()
    for kind, R in kinds:
        if kind == "host":
            continue
        banded = kind in ("band", "exact_band")
        if option == "no_affine_pairs" or kind.startswith("exact") or (option == "no_affine_band" and banded):
            out.add("affine_exact_band" if banded else "affine_exact")
        else:
            out.add("affine_%s_glob[R=%d]" % (kind, R))
    return sorted(out)


def check(ctx, xs, y, pairs, sc=DEFAULT, exp=None, upload=True, kinds=None):
    """Every dispatch, both calls: equal to the checker field for field, strings worth their score, paths that name the kernels.
    kinds: where each pair runs by default (Pair.kind unless given).  Returns the expectation."""
    if upload:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
    exp = expected(xs, y, pairs, sc) if exp is None else exp
    q, lo, hi, kw = call_args(pairs)
    kinds = [p.kind(xs) for p in pairs] if kinds is None else kinds
    traced = any(k != "host" for k, _ in kinds)
    options = (None, "no_affine_pairs") + (("no_affine_band",) if any(p.band for p in pairs) else ())
    for option in options:
        if option:
            ctx.set_option(option, 1)
        try:
            run = ctx.affine_global_run(q, lo, hi, **kw, **sc.kw())
            run_path = ctx.last_path()
            tr = ctx.affine_global_trace(q, lo, hi, **kw, **sc.kw())
            tr_path = ctx.last_path()
        finally:
            if option:
                ctx.set_option(option, 0)
        same(run, exp, ("score",))
        same(tr, exp, FIELDS)
        for path in (run_path, tr_path):
            assert not [t for t in path if t.startswith(FOREIGN)], (option, path)
            assert kernel_tags(path) == tags_for(kinds, option), (option, path)
        assert "affine_trace" not in run_path and ("affine_trace" in tr_path) == traced, (option, run_path, tr_path)
    for k, p in enumerate(pairs):
        cx, cy = exp["cons_x"][k], exp["cons_y"][k]
        if cx:
            assert G.rescore(cx, cy, **sc.kw()) == exp["score"][k]
    return exp


# ---- every pair instance and its edges ------------------------------------------------------------------------------------------
ROWS = (1, 2, 31, 32, 33, 80, 81, 150, 160, 161, 256, 257, 384, 385, 512)


def columns_for(m):
    cols = [1, 2, 15, 16, 17, 63, 64, 65, m, m + 40] + ([m - 7] if m > 7 else [])
    return sorted(set(cols))


@pytest.mark.parametrize("m", ROWS)
def test_every_pair_instance_and_its_edges(ctx, m):
    rng = np.random.default_rng(1000 + m)
    x = dna(rng, m)
    y = (mutate(rng, x) + dna(rng, 700))[:m + 60] if m > 2 else x + dna(rng, 80)
    pairs = [Pair(0, 0, n, back=b) for n in columns_for(m) for b in (0, 1)]
    exp = check(ctx, [x], y, pairs)
    R = pair_R(m)
    # the window of m + 40 columns: the corner is not the row's maximum (mutation 1), the windows of 1 and 2 columns are negative
    n = m + 40
    if m >= 31:
        assert G.score(x, y[:n]) != ER.to_end(ER.matrices(x, y[:n])[0])[0]
        assert G.score(x, y[:1]) < 0
    # one pair, one launch: the instance, its cells, and an op count strictly below the extension instance's on the same pair
    run = ctx.affine_global_run([0], [0], [n])
    k, t = ctx.last_kernel(), ctx.last_timings()
    assert run["score"][0] == G.score(x, y[:n])
    assert k["name"] == "sw_affine_pair_glob_kernel<R=%d>" % R and k["rows_per_lane"] == R and k["lanes"] == 16
    assert k["cells"] == float(m * n) and t["score_launches"] == 1 and t["cells"] == float(m * n)
    ctx.affine_extend_run([0], [0], [n])
    ke = ctx.last_kernel()
    assert ke["name"] == "sw_affine_pair_ext_kernel<R=%d>" % R and ke["cells"] == k["cells"]
    assert k["valu_ops_per_cell"] < ke["valu_ops_per_cell"]
    assert exp["end_x"].tolist() == [m] * len(pairs)


def test_513_rows_go_to_the_exact_kernel(ctx):
    rng = np.random.default_rng(513)
    x = dna(rng, 513)
    y = mutate(rng, x) + dna(rng, 40)
    pairs = [Pair(0, 0, len(y) - 40), Pair(0, 0, len(y), back=1), Pair(0, 3, 500)]
    assert [p.kind([x])[0] for p in pairs] == ["exact"] * 3
    check(ctx, [x], y, pairs)


# ---- capture, not the last value ------------------------------------------------------------------------------------------------
def test_capture_not_last_value(ctx):
    rng = np.random.default_rng(77)
    y = dna(rng, 1100)
    xs = [mutate(rng, y[:90])[:81], mutate(rng, y[:170])[:150], mutate(rng, y[:180])[:160], mutate(rng, y[:170])[:150],
          mutate(rng, y[:25])[:20], dna(rng, 20)]
    assert [len(x) for x in xs] == [81, 150, 160, 150, 20, 20]
    four = [Pair(0, 0, 20), Pair(1, 0, 150), Pair(2, 0, 400), Pair(3, 0, 1000)]     # one wavefront of the R = 10 instance
    assert {p.kind(xs) for p in four} == {("pair", 10)}
    # the corner of the long windows is far from the row's maximum: "the last value" and "the row's maximum" both fail
    for p in four[2:]:
        w = y[p.lo:p.hi]
        assert G.score(xs[p.q], w) != ER.to_end(ER.matrices(xs[p.q], w)[0])[0]
    six = four + [Pair(4, 0, 30), Pair(5, 5, 22)]                                   # and two pairs that launch separately (R = 2)
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    for pairs in (four, four[::-1], six, six[::-1]):
        check(ctx, xs, y, pairs, upload=False)
        ctx.affine_global_run(*call_args(pairs)[:3])
        assert ctx.last_timings()["score_launches"] == (1 if len(pairs) == 4 else 2)


# ---- negative and gap-heavy answers ---------------------------------------------------------------------------------------------
def test_gap_heavy_answers(ctx):
    rng = np.random.default_rng(5)
    a, b = dna(rng, 120), dna(rng, 140)
    # unrelated strings under a hard mismatch: negative, many gaps; over disjoint alphabets: no letter pair at all, two long gaps
    c, d = dna(rng, 120, "AC"), dna(rng, 140, "GT")
    y = b + d + dna(rng, 300)
    assert G.score(a, b, **HARD_MISMATCH.kw()) < 0 and G.score(c, d, **HARD_MISMATCH.kw()) == -(5.0 + 119.0) - (5.0 + 139.0)
    check(ctx, [a, c], y, [Pair(0, 0, 140), Pair(0, 0, 140, back=1), Pair(0, 10, 95), Pair(1, 140, 280), Pair(1, 140, 280, back=1)], HARD_MISMATCH)
    # x = a window with one 30-letter block removed and one inserted
    w = dna(rng, 200)
    x = w[:50] + w[80:140] + dna(rng, 30) + w[140:]
    y = w + dna(rng, 50)
    exp = check(ctx, [x], y, [Pair(0, 0, 200), Pair(0, 0, 200, back=1), Pair(0, 0, 250)])
    assert "30D" in exp["cigar"][0] and "30I" in exp["cigar"][0]
    assert exp["score"][2] != ER.to_end(ER.matrices(x, y[:250])[0])[0]
    # homopolymers: every placement of a gap ties (diagonal over E over F, the shortest gap)
    xs = ["A" * 40, "A" * 25 + "C" * 10, "AC" * 20]
    y = "A" * 60 + "C" * 20 + "AC" * 30
    pairs = [Pair(0, 0, 50), Pair(0, 0, 33, back=1), Pair(1, 20, 75), Pair(1, 20, 75, back=1), Pair(2, 80, 134), Pair(2, 81, 111), Pair(0, 0, 50, band=(-3, 12))]
    for sc in (DEFAULT, LINEAR):
        check(ctx, xs, y, pairs, sc)
    # open == extend on ordinary strings
    x = mutate(rng, w, 0.15)
    check(ctx, [x], w, [Pair(0, 0, 200), Pair(0, 0, 190, back=1), Pair(0, 0, 200, band=(-25, 25))], LINEAR)


# ---- degenerate and unreachable pairs -------------------------------------------------------------------------------------------
def test_degenerate_and_unreachable_pairs(ctx):
    rng = np.random.default_rng(9)
    y = dna(rng, 300)
    xs = [mutate(rng, y[:60]), dna(rng, 33)]
    m0 = len(xs[0])
    host = [Pair(0, 5, 5, 7, 7), Pair(0, 9, 9, 0, m0), Pair(1, 100, 140, 4, 4), Pair(1, 100, 101, 33, 33, back=1), Pair(0, 0, 0, 3, 4, back=1)]
    exp = check(ctx, xs, y, host)                                      # a list of only such pairs: no kernel tag (check compares the tags)
    assert exp["score"].tolist() == [0.0, -(5.0 + (m0 - 1)), -(5.0 + 39.0), -5.0, -5.0]
    assert exp["cons_x"][2] == "-" * 40 and exp["cons_y"][2] == y[100:140][::-1] and exp["pos"].tolist() == [0, 0, 1, 1, 0]
    for p in host:
        check(ctx, xs, y, [p], upload=False)
    real = [Pair(0, 0, 60, 0, m0), Pair(1, 100, 140, 0, 33, back=1)]
    check(ctx, xs, y, [host[0], real[0], host[1], host[2], real[1], host[3]], upload=False)
    # under bands: the degenerate pairs need band_lo <= -m (n = 0) and band_hi >= n (m = 0)
    banded = [Pair(0, 9, 9, 0, 10, band=(-10, 0)), Pair(0, 9, 9, 0, 10, band=(-9, 0)), Pair(1, 100, 140, 4, 4, band=(0, 40)),
              Pair(1, 100, 140, 4, 4, band=(-3, 39)), Pair(0, 5, 5, 7, 7, band=(0, 0))]
    exp = check(ctx, xs, y, banded, upload=False)
    assert exp["score"].tolist() == [-14.0, NINF, -44.0, NINF, 0.0]
    # n - m one outside each band edge: -inf and empty strings; exactly on each edge: computed
    x = xs[0]
    edges = []
    for lo, hi in ((-4, 6), (-20, 0), (0, 9)):
        edges += [Pair(0, 0, m0 + hi + 1, 0, m0, band=(lo, hi)), Pair(0, 0, m0 + hi, 0, m0, band=(lo, hi)), Pair(0, 0, m0 + lo, 0, m0, band=(lo, hi)),
                  Pair(0, 0, m0 + lo - 1, 0, m0, band=(lo, hi), back=1)]
    exp = check(ctx, xs, y, edges, upload=False)
    assert [s == NINF for s in exp["score"]] == [True, False, False, True] * 3
    assert all(exp["cons_x"][k] == "" and exp["end_x"][k] == 0 for k in (0, 3, 4, 7, 8, 11))
    check(ctx, xs, y, [host[2], edges[0], real[0], edges[1], host[1], edges[3]], upload=False)


# ---- every band instance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", BAND_R)
def test_every_band_instance(ctx, R):
    rng = np.random.default_rng(300 + R)
    m = 300
    x = dna(rng, m)
    y = mutate(rng, x, 0.1) + dna(rng, 400)
    pairs = []
    for W in (16 * R, 16 * R - 1):
        lo, hi = -(8 * R), W - 1 - 8 * R
        # n - m on the band's two edges (diagonals 0 and W - 1) and in a lane's first and last register
        for D in sorted({0, W - 1, R - 1, R, 15 * R - 1, 15 * R} & set(range(W))):
            pairs.append(Pair(0, 0, m + lo + D, band=(lo, hi), back=len(pairs) % 2))
    assert {p.kind([x]) for p in pairs} == {("band", R)}
    check(ctx, [x], y, pairs)
    p = pairs[0]
    ctx.affine_global_run([0], [0], [p.hi], band_lo=p.band[0], band_hi=p.band[1])
    k, t = ctx.last_kernel(), ctx.last_timings()
    assert k["name"] == "sw_affine_band_glob_kernel<R=%d>" % R and k["rows_per_lane"] == R and k["cells"] == float(m * 16 * R)
    assert t["score_launches"] == 1
    ctx.affine_extend_run([0], [0], [p.hi], band_lo=p.band[0], band_hi=p.band[1])
    ke = ctx.last_kernel()
    assert ke["name"] == "sw_affine_band_ext_kernel<R=%d>" % R and k["valu_ops_per_cell"] < ke["valu_ops_per_cell"]


def test_band_rows_widths_and_the_covering_band(ctx):
    rng = np.random.default_rng(31)
    xs = [dna(rng, 1), dna(rng, 2), dna(rng, 511), dna(rng, 512), dna(rng, 513), dna(rng, 300)]
    y = mutate(rng, xs[4], 0.06) + dna(rng, 300)
    xs[2], xs[3] = xs[4][:511], xs[4][:512]
    xs[5] = mutate(rng, y[:300], 0.06)[:290]
    pairs = [Pair(0, 0, 3, band=(-8, 8)), Pair(0, 0, 1, band=(0, 0)), Pair(1, 0, 2, band=(-1, 1)), Pair(1, 4, 9, band=(-8, 3), back=1),
             Pair(2, 0, 508, band=(-8, 8)), Pair(3, 0, 520, band=(-8, 8), back=1), Pair(3, 0, 512, band=(0, 0)),
             Pair(4, 0, 510, band=(-8, 8)),                               # 513 rows: the exact kernel under the band
             Pair(5, 0, 300, band=(-128, 128)),                           # W = 257: the exact kernel under the band
             Pair(5, 0, 300, band=(-128, 127))]                           # W = 256: the widest instance
    kinds = [p.kind(xs) for p in pairs]
    assert kinds[7] == ("exact_band", 0) and kinds[8] == ("exact_band", 0) and kinds[9] == ("band", 16) and kinds[6] == ("band", 1)
    assert kinds[0] == ("pair", 2) and kinds[1] == ("band", 1)            # 1 x 3 under [-8, 8]: covered; 1 x 1 under [0, 0]: one diagonal of three
    check(ctx, xs, y, pairs)
    # a band that covers the matrix takes the unbanded path: the same bytes, the pair kernel's tag
    q, lo, hi = [5, 1, 3], [0, 0, 0], [300, 2, 520]
    plain = ctx.affine_global_trace(q, lo, hi)
    plain_path = ctx.last_path()
    cover = ctx.affine_global_trace(q, lo, hi, band_lo=[-290, -5, -1 << 40], band_hi=[300, 2, 1 << 40])
    assert ctx.last_path() == plain_path and any(t.startswith("affine_pair_glob") for t in plain_path)
    assert not any(t.startswith("affine_band") or t == "affine_exact_band" for t in plain_path)
    for f in FIELDS:
        assert list(plain[f]) == list(cover[f]), f


def test_an_indel_outside_a_narrow_band_changes_the_answer(ctx):
    rng = np.random.default_rng(41)
    a, b, c = dna(rng, 59) + "A", "C" + dna(rng, 58) + "A", "C" + dna(rng, 59)
    # twelve letters of the window missing from the read, and further on twelve letters of the read missing from the window: the path
    # leaves diagonal 0 for diagonal 12 and comes back, so the corner lies on diagonal 0 and every band holds it
    x = a + b + "T" * 12 + c
    y = a + "G" * 12 + b + c + dna(rng, 30)
    n = 192
    # shown with the checker first: [-4, 12] holds the path on its edge, [-4, 11] and [-4, 4] do not and score lower
    full, edge = G.trace(x, y[:n]), G.trace(x, y[:n], -4, 12)
    assert full["cigar"] == edge["cigar"] == "60M12D60M12I60M" and full["score"] == edge["score"] == 540.0 - 32.0
    assert G.score(x, y[:n], -4, 4) < G.score(x, y[:n], -4, 11) < full["score"]
    pairs = [Pair(0, 0, n), Pair(0, 0, n, band=(-4, 12)), Pair(0, 0, n, band=(-4, 12), back=1), Pair(0, 0, n, band=(-4, 11)),
             Pair(0, 0, n, band=(-4, 4)), Pair(0, 0, n, band=(-4, 4), back=1), Pair(0, 0, n + 12, band=(-20, 11))]
    exp = check(ctx, [x], y, pairs)
    assert exp["score"][6] == NINF


# ---- against merged code on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [None, (-8, 8)])
def test_against_the_extension_on_the_device(ctx, band):
    rng = np.random.default_rng(49)
    y = dna(rng, 48)
    x = mutate(rng, y[:36], 0.1)[:33]
    assert len(x) == 33
    ctx.set_reference(y)
    ctx.batch_upload([x])
    kw = dict(band_lo=band[0], band_hi=band[1]) if band else {}
    ext = ctx.affine_extend_run([0], [0], [48], **kw)
    glob = ctx.affine_global_run([0] * 49, [0] * 49, list(range(49)), **kw)["score"]
    assert "affine_pair_ext" not in " ".join(ctx.last_path()) and "affine_band_ext" not in " ".join(ctx.last_path())
    assert float(glob.max()) == float(ext["to_end_score"][0]) and int(np.argmax(glob)) == int(ext["to_end_y"][0])
    assert int((glob != glob.max()).sum()) >= 40                      # the corner is not the row's maximum for most windows
    exp = [G.score(x, y[:n], *(band or (None, None))) for n in range(49)]
    assert glob.tolist() == exp


# ---- admission from both sides --------------------------------------------------------------------------------------------------
def test_admission_from_both_sides(ctx, pgs):
    rng = np.random.default_rng(23)
    y = dna(rng, 600)
    xs = [mutate(rng, y[:26])[:20], dna(rng, 512)]
    assert len(xs[0]) == 20
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    pairs = [Pair(0, 0, 30)]
    # 3 gap_open + (rows + columns) gap_extend - smin < 2^24 with 20 rows, 30 columns, smin = -3: gap_open <= 5592387
    assert 3 * 5592387 + 50 + 3 < 2 ** 24 <= 3 * 5592388 + 50 + 3 and 3 * 5592388 + 50 < 2 ** 24 <= 3 * 5592389 + 50
    below, above, beyond = (Scoring("o=%d" % o, 3, -3, o, 1) for o in (5592387, 5592388, 5592389))
    check(ctx, xs, y, pairs, below, upload=False)                                           # the pair kernel
    check(ctx, xs, y, pairs, above, upload=False, kinds=[("exact", 0)])                     # the exact kernel
    good = ctx.affine_global_trace([0], [0], [30])
    for call in (ctx.affine_global_run, ctx.affine_global_trace):
        with pytest.raises(pgs.capi.MI355Error) as e:
            call([0, 0], [0, 0], [25, 30], **beyond.kw())                                    # (the window of 25 columns is still admitted)
        assert e.value.code == ENOTSUP and "pair 1 " in str(e.value) and "20 rows x 30 columns" in str(e.value)
        again = ctx.affine_global_trace([0], [0], [30])
        assert all(list(again[f]) == list(good[f]) for f in FIELDS)
    # the band kernel: a rows + 3 gap_open + (W + 1) gap_extend - smin < 2^24 with 20 rows, a = 3, W = 9: 60 + 3 o + 10 + 3
    bp = [Pair(0, 0, 24, band=(-4, 4))]
    assert 60 + 3 * 5592380 + 13 < 2 ** 24 <= 60 + 3 * 5592381 + 13
    check(ctx, xs, y, bp, Scoring("o", 3, -3, 5592380, 1), upload=False)
    check(ctx, xs, y, bp, Scoring("o", 3, -3, 5592381, 1), upload=False, kinds=[("exact_band", 0)])
    # L23 has no key inequality: match = 600 at 512 rows, smax (rows + 1) = 307800 >= 2^18, runs on the pair kernel and equals the exact
    # kernel (check runs both); the extension call sends the same pair to its exact kernel
    big = Scoring("600/-3/5/1", 600, -3, 5, 1)
    long_pairs = [Pair(1, 0, 540), Pair(1, 20, 520, back=1)]
    assert long_pairs[0].kind(xs) == ("pair", 32)
    check(ctx, xs, y, long_pairs, big, upload=False)
    ctx.affine_extend_run([1], [0], [540], **big.kw())
    assert "affine_exact" in ctx.last_path() and not any(t.startswith("affine_pair_ext") for t in ctx.last_path())


# ---- refusals and errors leave the context usable -------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, pgs):
    rng = np.random.default_rng(61)
    y = dna(rng, 400)
    xs = [mutate(rng, y[:100]), dna(rng, 50)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    q, lo, hi = [0, 1, 0], [0, 30, 10], [110, 90, 70]
    bands = dict(band_lo=[-30, -12, -50], band_hi=[30, 12, 0])
    good = ctx.affine_global_trace(q, lo, hi, **bands)
    bad = [dict(args=([0, 2, 0], lo, hi), kw=bands), dict(args=([0, -1, 0], lo, hi), kw={}), dict(args=(q, lo, [110, 401, 70]), kw={}),
           dict(args=(q, [0, 95, 10], hi), kw={}), dict(args=(q, lo, hi), kw=dict(q_lo=[0, 0, 5], q_hi=[10, 51, 6])),
           dict(args=(q, lo, hi), kw=dict(q_lo=[0, 7, 5], q_hi=[10, 6, 6])), dict(args=(q, lo, hi), kw=dict(band_lo=[-30, 1, -50], band_hi=[30, 12, 0])),
           dict(args=(q, lo, hi), kw=dict(band_lo=[-30, -1, -50], band_hi=[30, 12, -1])), dict(args=(q, lo, hi), kw=dict(gap_open=1.0, gap_extend=2.0)),
           dict(args=(q, lo, hi), kw=dict(gap_extend=0.0))]
    for b in bad:
        for call in (ctx.affine_global_run, ctx.affine_global_trace):
            with pytest.raises(pgs.capi.MI355Error) as e:
                call(*b["args"], **b["kw"])
            assert e.value.code == EINVAL, b
            again = ctx.affine_global_trace(q, lo, hi, **bands)
            assert all(list(again[f]) == list(good[f]) for f in FIELDS)
    # exactly one band, or a null output, straight at the C interface; nothing is written
    L = pgs.capi.lib()
    el, n, keep = ctx._extend_list(q, lo, hi, None, None, None)
    p, keep2 = pgs.capi.make_affine_params()
    blo, bhi = (C.c_int64 * 3)(-30, -12, -50), (C.c_int64 * 3)(30, 12, 0)
    f3 = (C.c_float * 3)(7, 7, 7)
    res = (pgs.capi.Result * 3)()
    assert L.mi355_sw_affine_global_run(ctx._ctx, C.byref(el), blo, None, C.byref(p), f3) == EINVAL
    assert L.mi355_sw_affine_global_run(ctx._ctx, C.byref(el), None, bhi, C.byref(p), f3) == EINVAL
    assert L.mi355_sw_affine_global_run(ctx._ctx, C.byref(el), blo, bhi, C.byref(p), None) == EINVAL
    assert L.mi355_sw_affine_global_trace(ctx._ctx, C.byref(el), blo, bhi, C.byref(p), None) == EINVAL
    assert L.mi355_sw_affine_global_trace(ctx._ctx, C.byref(el), blo, None, C.byref(p), res) == EINVAL
    assert list(f3) == [7, 7, 7] and all(r.cons_x is None for r in res)
    el.npairs = 0                                                      # no pairs: 0, and nothing is written
    assert L.mi355_sw_affine_global_run(ctx._ctx, C.byref(el), blo, bhi, C.byref(p), None) == 0
    assert L.mi355_sw_affine_global_trace(ctx._ctx, C.byref(el), blo, bhi, C.byref(p), None) == 0
    el.npairs = 3
    assert L.mi355_sw_affine_global_run(ctx._ctx, C.byref(el), blo, bhi, C.byref(p), f3) == 0
    assert list(f3) == list(good["score"])
    again = ctx.affine_global_trace(q, lo, hi, **bands)
    assert all(list(again[f]) == list(good[f]) for f in FIELDS)
    # the Python front end
    out = pgs.AffineSWAligner.global_pairs(q, lo, hi, context=ctx, traceback=True, band=([-30, -12, -50], [30, 12, 0]))
    assert all(list(out[f]) == list(good[f]) for f in FIELDS)
    assert pgs.AffineSWAligner.global_pairs(q, lo, hi, context=ctx, band=(-200, 200))["score"].tolist() == ctx.affine_global_run(q, lo, hi)["score"].tolist()


# ---- fuzz -----------------------------------------------------------------------------------------------------------------------
AMINO = "ACDEFGHIKLMNPQRSTVWY"


def protein_table(rng):
    t = np.full((256, 256), -4.0, dtype=np.float32)
    s = rng.integers(-4, 4, (20, 20))
    s = np.minimum(s, s.T)
    for i, a in enumerate(AMINO):
        for j, b in enumerate(AMINO):
            t[ord(a), ord(b)] = float(s[i, j]) if i != j else float(rng.integers(4, 12))
    return t


@pytest.mark.parametrize("which", ["3/-3/5/1", "3/-10/5/1", "2/-4/3/3", "protein"])
def test_fuzz(ctx, which):
    rng = np.random.default_rng({"3/-3/5/1": 1, "3/-10/5/1": 2, "2/-4/3/3": 3, "protein": 4}[which])
    letters = AMINO if which == "protein" else "ACGT"
    sc = {"3/-3/5/1": DEFAULT, "3/-10/5/1": HARD_MISMATCH, "2/-4/3/3": LINEAR}.get(which) or Scoring("protein", 0, 0, 11, 1, protein_table(rng))
    y = dna(rng, 3000, letters)
    starts = [int(rng.integers(0, 2700)) for _ in range(24)]
    xs = [mutate(rng, y[s:s + int(rng.integers(40, 240))], 0.1, letters) for s in starts]
    pairs = []
    while len(pairs) < 200:
        q = int(rng.integers(0, len(xs)))
        m = int(rng.integers(1, min(200, len(xs[q])) + 1))
        q_lo = int(rng.integers(0, len(xs[q]) - m + 1))
        n = max(0, m + int(rng.integers(-30, 31)))
        lo = min(max(0, starts[q] + q_lo + int(rng.integers(-3, 4))), len(y) - n)
        band = None
        if len(pairs) % 2:
            w = int(rng.integers(0, 41))
            band = (-w, w)
        pairs.append(Pair(q, lo, lo + n, q_lo, q_lo + m, back=int(rng.integers(0, 2)), band=band))
    kinds = {p.kind(xs)[0] for p in pairs}
    assert {"pair", "band", "host"} <= kinds                          # unreachable pairs are part of the mix
    check(ctx, xs, y, pairs, sc)
