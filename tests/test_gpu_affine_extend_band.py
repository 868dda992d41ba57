"""The anchored seed extension inside a diagonal band on the device (mi355_sw_affine_extend_run_band / _trace_band) against
tests/affine_extend_band_ref.py applied to the letters x[q_lo:q_hi] and the slice y[left:right], clipped as the header says.  Every
case runs through both dispatches — the default one (sw_affine_band_ext_kernel where it admits the pair) and option no_affine_band
(the exact kernel under the band) — and through both calls, run and trace: every field and both strings must equal the checker, the
strings must be worth the traced score, every emitted cell must lie in the band, and the path must show which kernel ran (a banded
pair never on an unbanded kernel).  Scores are integers: no tolerance.  Expected values are computed once per case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import affine_extend_band_ref as br, score_instances as si

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
NINF = float("-inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_KERNEL_H = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "sw_affine_band_kernel.h")
RUN_FIELDS = ("score", "end_x", "end_y", "to_end_score", "to_end_y")
TRACE_FIELDS = RUN_FIELDS + ("pos", "cons_x", "cons_y", "cigar")
STRINGS = ("cons_x", "cons_y", "cigar")


def compiled_R():
    with open(BAND_KERNEL_H) as f:
        m = re.search(r"constexpr\s+int\s+kBandR\[\]\s*=\s*\{([^}]*)\}", f.read())
    return tuple(int(v) for v in m.group(1).split(","))


BAND_R = compiled_R()


def instance_of(W):
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


class Pair:
    """One pair of a list: query q, its letters [q_lo, q_hi) (None: all), the window [lo, hi), the band [blo, bhi], the direction, the
    traced alignment."""
    def __init__(self, q, lo, hi, blo, bhi, q_lo=None, q_hi=None, back=0, to_end=0):
        self.q, self.lo, self.hi, self.blo, self.bhi = q, lo, hi, blo, bhi
        self.q_lo, self.q_hi, self.back, self.to_end = q_lo, q_hi, back, to_end

    def letters(self, xs):
        x = xs[self.q]
        return x if self.q_lo is None else x[self.q_lo:self.q_hi]

    def effective(self, xs):
        """(m, n, lo_e, hi_e, W, covering)"""
        m, n = len(self.letters(xs)), self.hi - self.lo
        lo_e, hi_e = max(self.blo, -m), min(self.bhi, n)
        return m, n, lo_e, hi_e, hi_e - lo_e + 1, (lo_e == -m and hi_e == n)


def reference(x, y, p, sc):
    """(the run call's fields, the trace call's fields) by the checker, from one fill of the matrices over the clipped window."""
    xb, yb = br._b(x), br._b(y)
    if p.back:
        xb, yb = xb[::-1], yb[::-1]
    yb = yb[:br.clip(len(xb), len(yb), p.bhi)]
    H, E, F, S = br.matrices(xb, yb, p.blo, p.bhi, **sc.kw())
    s, i, j = br.best(H)
    ts, tj = br.to_end(H)
    run = dict(score=s, end_x=i, end_y=j, to_end_score=ts, to_end_y=tj)
    if p.to_end and tj < 0:
        tr = dict(run, score=NINF, end_x=0, end_y=0, pos=0, cons_x="", cons_y="", cigar="")
        return run, tr
    cs, ci, cj = (ts, len(xb), tj) if p.to_end else (s, i, j)
    cx, cy = br.walk(xb, yb, H, E, F, S, ci, cj, sc.open)
    tr = dict(score=cs, end_x=ci, end_y=cj, to_end_score=ts, to_end_y=tj, pos=1 if cj > 0 else 0, cons_x=cx, cons_y=cy,
              cigar=br.cigar(cx[::-1], cy[::-1]) if p.back else br.cigar(cx, cy))
    return run, tr


def columns(rows, fields):
    return {f: ([r[f] for r in rows] if f in STRINGS else np.array([r[f] for r in rows], dtype=np.float64)) for f in fields}


def expected(xs, y, pairs, sc):
    both = [reference(p.letters(xs), y[p.lo:p.hi], p, sc) for p in pairs]
    return columns([b[0] for b in both], RUN_FIELDS), columns([b[1] for b in both], TRACE_FIELDS)


def same(got, exp, fields):
    for f in fields:
        a, b = got[f], exp[f]
        ok = np.array_equal(np.asarray(a, dtype=np.float64), b) if isinstance(b, np.ndarray) else list(a) == list(b)
        assert ok, (f, [(k, u, v) for k, (u, v) in enumerate(zip(a, b)) if u != v][:5])


def call_args(pairs):
    ranged = any(p.q_lo is not None for p in pairs)
    assert not ranged or all(p.q_lo is not None for p in pairs)
    kw = dict(backward=[p.back for p in pairs] if any(p.back for p in pairs) else None,
              band_lo=[p.blo for p in pairs], band_hi=[p.bhi for p in pairs])
    if ranged:
        kw.update(q_lo=[p.q_lo for p in pairs], q_hi=[p.q_hi for p in pairs])
    return [p.q for p in pairs], [p.lo for p in pairs], [p.hi for p in pairs], kw, [p.to_end for p in pairs]


def band_tags(path):
    return [t for t in path if t.startswith("affine_band")]


def check(ctx, xs, y, pairs, sc=DEFAULT, exp=None, upload=True, kernels="band", options=("no_affine_band",)):
    """The default dispatch and one per option of `options`, both calls: equal to the checker field for field; the paths name the
    kernels.  kernels: what the banded pairs of the default dispatch run on — "band", "exact", "both", or "none" (no banded pair
    reaches a kernel).  Returns the expectation of the trace call."""
    if upload:
        ctx.set_reference(y)
        ctx.batch_upload(xs)
    exp = expected(xs, y, pairs, sc) if exp is None else exp
    q, lo, hi, kw, te = call_args(pairs)
    eff = [p.effective(xs) for p in pairs]
    unbanded = any(e[5] and e[0] >= 1 and e[1] >= 1 for e in eff)
    for option in (None,) + tuple(options):
        if option:
            ctx.set_option(option, 1)
        try:
            got = ctx.affine_extend_run(q, lo, hi, **kw, **sc.kw())
            p_run = ctx.last_path()
            traced = ctx.affine_extend_trace(q, lo, hi, to_end=te, **kw, **sc.kw())
            p_trace = ctx.last_path()
        finally:
            if option:
                ctx.set_option(option, 0)
        same(got, exp[0], RUN_FIELDS)
        same(traced, exp[1], TRACE_FIELDS)
        for k, p in enumerate(pairs):
            if traced["score"][k] == NINF:
                continue
            assert br.rescore(traced["cons_x"][k], traced["cons_y"][k], **sc.kw()) == traced["score"][k], k
            cells = br.path_cells(traced["cons_x"][k], traced["cons_y"][k], int(traced["end_x"][k]), int(traced["end_y"][k]))
            assert all(br.in_band(i, j, p.blo, p.bhi) for i, j in cells), k
        on_band = option is None and kernels in ("band", "both")
        on_exact = kernels != "none" and (option is not None or kernels in ("exact", "both"))
        for path in (p_run, p_trace):
            tags = band_tags(path)
            assert all(t.startswith("affine_band_ext[R=") for t in tags), path       # never the local band instance
            assert (len(tags) > 0) == on_band, (option, path)
            assert ("affine_exact_band" in path) == on_exact, (option, path)
            if not unbanded:                                                       # a banded pair never runs on an unbanded kernel
                assert not any(t.startswith("affine_pair") or t == "affine_exact" for t in path), path
    return exp[1]


def mirrored(xs, y, pairs):
    """The mirror image of a case: every string reversed, every window and range mirrored, every direction flipped; the bands stay."""
    n = len(y)
    out = []
    for p in pairs:
        L = len(xs[p.q])
        ql, qh = (None, None) if p.q_lo is None else (L - p.q_hi, L - p.q_lo)
        out.append(Pair(p.q, n - p.hi, n - p.lo, p.blo, p.bhi, ql, qh, 1 - p.back, p.to_end))
    return [x[::-1] for x in xs], y[::-1], out


def check_both_ways(ctx, xs, y, pairs, sc=DEFAULT, **kw):
    exp = check(ctx, xs, y, pairs, sc, **kw)
    mxs, my, mp = mirrored(xs, y, pairs)
    back = check(ctx, mxs, my, mp, sc, **kw)
    same(back, exp, RUN_FIELDS + ("pos", "cons_x", "cons_y"))
    return exp


def read_of(pgs, y, seed, at, m):
    """m letters of y from `at` on with a few substitutions, one letter dropped and a run of letters inserted where there is room."""
    x = np.frombuffer(y[at:at + m + 8], dtype=np.uint8).copy()
    r = pgs.synth.splitmix64(seed, 8)
    if m >= 12:
        for k in range(3):
            x[int(r[k] % np.uint64(m))] = b"ACGT"[int(r[3 + k] % np.uint64(4))]
    if m >= 40:
        cut = 5 + int(r[6] % np.uint64(m - 30))
        x = np.concatenate([x[:cut], x[cut + 1:cut + 12], np.frombuffer(b"TTG", dtype=np.uint8), x[cut + 12:]])
    return x[:m].tobytes()


def band_of(m, W):
    """A band of exactly W diagonals inside a matrix of m rows whose window is at least W columns long."""
    lo = -min(m, W // 2)
    return lo, lo + W - 1


# ---- every compiled instance at its edges: W = 16 R, 16 R - 1 and one more than the previous instance holds; rows 1 .. 512 -------------
ROWS = (1, 2, 17, 150, 512)


@pytest.mark.parametrize("R", BAND_R)
def test_every_instance_and_its_edges(ctx, pgs, R):
    prev = max([r for r in BAND_R if r < R], default=0)
    widths = sorted({16 * R, 16 * R - 1, 16 * prev + 1})
    y = pgs.synth.dna(13100 + R, 1600).tobytes()
    xs = [read_of(pgs, y, 13200 + 7 * R + k, 300, m) for k, m in enumerate(ROWS)]
    pairs = []
    for k, m in enumerate(ROWS):
        for W in widths:
            lo, hi = band_of(m, W)
            p = Pair(k, 300, 300 + m + hi + 5, lo, hi, to_end=(k + W) % 2)
            assert p.effective(xs)[4] == W and instance_of(W) == R and not p.effective(xs)[5]
            pairs.append(p)
    exp = check_both_ways(ctx, xs, y, pairs)
    assert max(exp["score"][len(widths) * 3:len(widths) * 4]) > 100
    lo, hi = band_of(150, 16 * R)
    ctx.affine_extend_run([3], [300], [300 + 150 + hi + 5], band_lo=lo, band_hi=hi)
    assert ctx.last_path() == ["affine_band_ext[R=%d]" % R], ctx.last_path()
    ki = ctx.last_kernel()
    assert ki["name"] == "sw_affine_band_ext_kernel<R=%d>" % R and ki["dtype"] == "f32" and ki["rows_per_lane"] == R, ki
    assert ki["cells"] == 150 * 16 * R and 15 < ki["valu_ops_per_cell"] <= 16 + 33 / R + 1e-9
    t = ctx.last_timings()
    assert t["score_us"] > 0 and t["score_launches"] == 1 and t["cells"] == ki["cells"]


# ---- the borders: column 0 and row 0 walk across the lanes of a slot ---------------------------------------------------------------------
@pytest.mark.parametrize("m", (40, 150, 250))
def test_column0_across_lanes(ctx, pgs, m):
    """lo_e = -m: the whole of column 0 is in the band, on diagonal D = m - i in row i — it crosses every lane boundary on its way
    down.  J junk letters in front of a copy: the path opens with J insertions along column 0."""
    sc = HARD_MISMATCH
    y = pgs.synth.dna(13300 + m, 1000).tobytes()
    a = 200
    pairs, xs = [], []
    for J in (3, 19, m - 8):
        xs.append(b"N" * J + y[a:a + m - J])
        pairs += [Pair(len(xs) - 1, a, a + m + 30, -m, 3), Pair(len(xs) - 1, a, a + m + 30, -m, 3, to_end=1)]
    R = instance_of(m + 4)
    assert all(p.effective(xs)[2] == -m and p.effective(xs)[4] == m + 4 for p in pairs) and m > R
    exp = check_both_ways(ctx, xs, y, pairs, sc)
    for k, J in enumerate((3, 19, m - 8)):
        L = m - J
        if 3 * L > 5 + J - 1:
            assert exp["score"][2 * k] == 3 * L - (5 + J - 1) and exp["cigar"][2 * k] == "%dI%dM" % (J, L)
    # a band that stops short of the junk: the insertions are forbidden, the answer changes
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    narrow = ctx.affine_extend_run([1], [a], [a + m + 30], band_lo=-18, band_hi=3, **sc.kw())
    assert narrow["score"][0] < exp["score"][2] or m - 19 < 8


@pytest.mark.parametrize("R", BAND_R)
def test_row0_across_lanes(ctx, pgs, R):
    """hi_e >= R: row 0, the initial registers, spans lanes.  The window has J extra leading columns: the path opens with J deletions
    along row 0."""
    sc = HARD_MISMATCH
    y = pgs.synth.dna(13400 + R, 1200).tobytes()
    a, L = 200, 120
    prev = max([r for r in BAND_R if r < R], default=0)
    J = max(2, 16 * prev + 1 - 5)                                       # W = J + 5 diagonals: on instance R
    xs = [y[a + J:a + J + L]]
    pairs = [Pair(0, a, a + J + L + 20, -2, J + 2), Pair(0, a, a + J + L + 20, -2, J + 2, to_end=1), Pair(0, a, a + J + L + 20, -2, J - 1)]
    assert instance_of(J + 5) == R and J + 2 >= R
    exp = check_both_ways(ctx, xs, y, pairs, sc)
    assert exp["score"][0] == 3 * L - (5 + J - 1) and exp["cigar"][0] == "%dD%dM" % (J, L)
    assert exp["score"][2] < exp["score"][0]                            # one diagonal short: the deletions are forbidden


# ---- four slots of one wavefront with four different row counts: the to-end fold fires at four different steps -------------------------
@pytest.mark.parametrize("W", (17, 33, 129))
def test_four_slots_of_a_wavefront(ctx, pgs, W):
    y = pgs.synth.dna(13500 + W, 1600).tobytes()
    rows = (1, 7, 150, 512)
    xs = [read_of(pgs, y, 13510 + k, 300, m) for k, m in enumerate(rows)]
    pairs = []
    for k, m in enumerate(rows):
        lo, hi = band_of(m, W)
        pairs.append(Pair(k, 300, 300 + m + hi + 9, lo, hi, to_end=1))
    assert len({instance_of(p.effective(xs)[4]) for p in pairs}) == 1   # one launch: the four pairs fill the first wavefront
    exp = check_both_ways(ctx, xs, y, pairs)
    assert all(exp["end_x"][k] == m for k, m in enumerate(rows))
    ctx.affine_extend_run(*call_args(pairs)[:3], band_lo=[p.blo for p in pairs], band_hi=[p.bhi for p in pairs])
    assert ctx.last_timings()["score_launches"] == 1


# ---- the shape of the window -----------------------------------------------------------------------------------------------------------------
def test_window_shapes(ctx, pgs):
    y = pgs.synth.dna(13601, (1 << 20) + 1024).tobytes()
    xs = [read_of(pgs, y, 13602, 500, 150), read_of(pgs, y, 13603, 500, 20)]
    pairs = [Pair(0, 500, 600, -60, 8), Pair(0, 500, 600, -60, 8, to_end=1),            # n < m, the end reachable (lo <= n - m)
             Pair(0, 500, 655, -8, 8), Pair(0, 500, 655, -8, 8, to_end=1),              # n shorter than m + hi
             Pair(0, 500, 649, -8, 8, to_end=1),                                        # the last in-band column of row m is n
             Pair(1, 500, 500 + (1 << 20), -8, 8), Pair(1, 500, 500 + (1 << 20), -8, 8, to_end=1),   # 2^20 columns, 17 diagonals
             Pair(0, 500, 500 + (1 << 20), -8, 8, back=0, to_end=1)]
    exp = check(ctx, xs, y, pairs)
    assert exp["score"][5] > 30 and exp["end_y"][6] <= 28 and exp["to_end_score"][1] > NINF
    # without the clip the exact kernel would refuse 20 x 2^20 cells and up; it takes the clipped window
    assert (1 << 20) * 150 > 1 << 26


# ---- to the end --------------------------------------------------------------------------------------------------------------------------------
def test_to_the_end(ctx, pgs):
    sc = HARD_MISMATCH
    y = pgs.synth.dna(13701, 800).tobytes()
    xs = [read_of(pgs, y, 13702, 100, 60), b"N" * 5, y[100:130]]
    pairs = [Pair(0, 100, 150, -4, 4), Pair(0, 100, 150, -4, 4, to_end=1),               # unreachable: lo = -4 > n - m = -10
             Pair(0, 100, 150, -10, 4, to_end=1),                                         # just reachable: one in-band cell of row m
             Pair(1, 100, 140, -5, 2), Pair(1, 100, 140, -5, 2, to_end=1),               # junk: the end is cheapest at column 0
             Pair(1, 100, 100, -5, 3, to_end=1),                                          # n = 0, band_lo <= -m: host-filled, covering
             Pair(1, 100, 100, -4, 3), Pair(1, 100, 100, -4, 3, to_end=1),               # n = 0, band_lo > -m: unreachable
             Pair(2, 100, 100, 0, 0, to_end=1), Pair(2, 100, 110, 0, 0, to_end=1)]        # the diagonal alone, n < m
    exp = check_both_ways(ctx, xs, y, pairs, sc)
    assert exp["to_end_score"][0] == NINF and exp["to_end_y"][0] == -1 and exp["score"][0] > 0
    assert (exp["score"][1], exp["end_x"][1], exp["end_y"][1], exp["cons_x"][1]) == (NINF, 0, 0, "")
    assert exp["to_end_score"][2] > NINF and exp["to_end_y"][2] == 50
    assert exp["to_end_y"][3] == 0 and exp["to_end_score"][3] == -9 and exp["cigar"][4] == "5I"
    assert exp["to_end_score"][5] == -9 and exp["to_end_y"][5] == 0 and exp["cigar"][5] == "5I"
    assert exp["to_end_y"][6] == -1 and exp["score"][7] == NINF
    assert exp["to_end_y"][9] == -1 and exp["score"][9] == NINF


# ---- ties --------------------------------------------------------------------------------------------------------------------------------------
def test_ties(ctx, pgs):
    # 0: the maximum 7 stands at (6,7) and at (7,6): the sweep by rows meets (6,7) first, the first in column-major order is (7,6)
    # 1: row m holds its maximum 0 in columns 2 and 4: the smallest wins
    xs = [b"CAACACAA", b"ACCA"]
    y = b"ACCACAC" + b"GG" + b"CACA" + b"GG"
    pairs = [Pair(0, 0, 7, -1, 1), Pair(1, 9, 13, -2, 1), Pair(1, 9, 13, -2, 1, to_end=1)]
    H = br.matrices(xs[0], y[0:7], -1, 1)[0]
    assert H.max() == 7 and H[6, 7] == 7 and H[7, 6] == 7
    H = br.matrices(xs[1], y[9:13], -2, 1)[0]
    assert list(np.nonzero(H[4] == H[4].max())[0]) == [2, 4]
    exp = check(ctx, xs, y, pairs)
    assert (exp["end_x"][0], exp["end_y"][0]) == (7, 6) and exp["to_end_y"][1] == 2 and exp["end_y"][2] == 2


# ---- identity and effect -----------------------------------------------------------------------------------------------------------------------
def test_a_covering_band_is_the_unbanded_call(ctx, pgs):
    y = pgs.synth.dna(13801, 1200).tobytes()
    xs = [read_of(pgs, y, 13802, 300, 150), read_of(pgs, y, 13803, 300, 40)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    q, lo, hi = [0, 1, 0, 1], [300, 300, 300, 700], [480, 360, 300, 760]
    back = [0, 0, 0, 1]
    plain = ctx.affine_extend_trace(q, lo, hi, backward=back, to_end=[0, 1, 1, 0])
    p_plain = ctx.last_path()
    for blo, bhi in (([-150, -40, -150, -40], [180, 60, 0, 60]), (-(1 << 40), 1 << 40)):
        banded = ctx.affine_extend_trace(q, lo, hi, backward=back, to_end=[0, 1, 1, 0], band_lo=blo, band_hi=bhi)
        assert ctx.last_path() == p_plain and not band_tags(ctx.last_path()) and "affine_exact_band" not in ctx.last_path()
        assert any(t.startswith("affine_pair_ext[R=") for t in ctx.last_path())
        for f in TRACE_FIELDS:
            a, b = banded[f], plain[f]
            assert (a.tobytes() == b.tobytes()) if isinstance(a, np.ndarray) else a == b, f
    run_p = ctx.affine_extend_run(q, lo, hi, backward=back)
    run_b = ctx.affine_extend_run(q, lo, hi, backward=back, band_lo=-(1 << 40), band_hi=1 << 40)
    assert all(run_p[f].tobytes() == run_b[f].tobytes() for f in RUN_FIELDS)


def test_a_band_changes_the_answer(ctx, pgs):
    """A read with a 10-letter deletion: half width 16 holds the gap, half width 4 does not."""
    y = pgs.synth.dna(13901, 1000).tobytes()
    a = 200
    xs = [y[a:a + 60] + y[a + 70:a + 160]]
    pairs = [Pair(0, a, a + 200, -16, 16), Pair(0, a, a + 200, -4, 4), Pair(0, a, a + 200, -16, 16, to_end=1), Pair(0, a, a + 200, -4, 4, to_end=1)]
    exp = check_both_ways(ctx, xs, y, pairs)
    assert exp["score"][0] == 3 * 150 - 14 and re.match(r"^\d+M10D\d+M$", exp["cigar"][0])
    assert 180 <= exp["score"][1] < 250 and "10D" not in exp["cigar"][1] and exp["to_end_score"][1] < exp["to_end_score"][0]
    assert exp["cons_x"][2] != exp["cons_x"][3]
    # the aligner class's front end takes the band as one (lo, hi) pair and reaches the banded entry points, run and trace
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    q, lo, hi = [0, 0], [a, a], [a + 200, a + 200]
    for tb in (False, True):
        want = (ctx.affine_extend_trace if tb else ctx.affine_extend_run)(q, lo, hi, band_lo=[-16, -4], band_hi=[16, 4])
        got = pgs.AffineSWAligner.extend_pairs(q, lo, hi, band=([-16, -4], [16, 4]), context=ctx, traceback=tb)
        assert sorted(band_tags(ctx.last_path())) == ["affine_band_ext[R=1]", "affine_band_ext[R=3]"]      # 9 and 33 diagonals
        assert sorted(got) == sorted(want) and all(list(got[f]) == list(want[f]) for f in want)
        assert (got["score"][0], got["score"][1]) == (exp["score"][0], exp["score"][1])
    one = pgs.AffineSWAligner.extend_pairs([0], [a], [a + 200], band=(-4, 4), context=ctx)
    assert one["score"][0] == exp["score"][1] and one["to_end_score"][0] == exp["to_end_score"][1]


# ---- directions --------------------------------------------------------------------------------------------------------------------------------
def test_directions_and_sub_ranges(ctx, pgs):
    y = pgs.synth.dna(14001, 2000).tobytes()
    x = read_of(pgs, y, 14002, 500, 200)
    xs = [x, y[900:1000]]
    # a seed at read offset 80..100: extend to the right of it and to the left of it, inside half width 12
    pairs = [Pair(0, 600, 760, -12, 12, 100, 200), Pair(0, 440, 580, -12, 12, 0, 80, back=1),
             Pair(0, 600, 760, -12, 12, 100, 200, to_end=1), Pair(0, 440, 580, -12, 12, 0, 80, back=1, to_end=1),
             Pair(1, 905, 1100, -3, 9, 5, 100), Pair(1, 700, 995, -3, 9, 0, 95, back=1, to_end=1)]
    exp = check(ctx, xs, y, pairs)
    assert exp["score"][4] == 3 * 95 and exp["score"][5] == 3 * 95 and exp["score"][0] > 100 and exp["score"][1] > 100
    check(ctx, xs, y, [p for p in pairs if not p.back], exp=None)
    check(ctx, xs, y, [p for p in pairs if p.back], exp=None)


# ---- fallbacks ---------------------------------------------------------------------------------------------------------------------------------
def test_fallbacks_to_the_exact_kernel_under_the_band(ctx, pgs):
    y = pgs.synth.dna(14101, 1600).tobytes()
    xs = [read_of(pgs, y, 14102, 300, 513), read_of(pgs, y, 14103, 300, 400)]
    rows513 = [Pair(0, 300, 900, -8, 8), Pair(0, 300, 900, -8, 8, to_end=1)]
    wide = [Pair(1, 300, 900, -128, 128), Pair(1, 300, 900, -128, 128, to_end=1)]
    ok = [Pair(1, 300, 900, -128, 127)]
    assert wide[0].effective(xs)[4] == 257 and ok[0].effective(xs)[4] == 256
    exp = check_both_ways(ctx, xs, y, rows513, kernels="exact")
    assert exp["score"][0] > 1000
    check(ctx, xs, y, wide, kernels="exact")
    check(ctx, xs, y, rows513 + wide + ok, kernels="both", options=("no_affine_band", "no_affine_pairs"))


def test_admission_bound_from_both_sides(ctx, pgs):
    # band kernel: a rows + 3 gap_open + (W + 1) gap_extend - smin < 2^24 (include/mi355_sw.h); rows = 6, W = 5, a = -smin = 3,
    # gap_extend = 1.  The exact kernel under a band holds a pair while a rows + 2 gap_open + W gap_extend - smin < 2^24
    y = b"ACGTTGCAAGGCTTAACCGGATATCG"
    xs = [y[0:6], y[8:10] + b"T" + y[11:14]]
    pairs = [Pair(0, 0, 8, -2, 2), Pair(1, 8, 16, -2, 2, to_end=1), Pair(0, 0, 8, -2, 2, to_end=1), Pair(1, 6, 14, -2, 2, back=1)]
    assert all(p.effective(xs)[0] == 6 and p.effective(xs)[4] == 5 for p in pairs)
    fixed = 3 * 6 + 6 * 1 + 3
    last_in = (2 ** 24 - 1 - fixed) // 3
    assert 3 * last_in + fixed < 2 ** 24 <= 3 * (last_in + 1) + fixed and 18 + 2 * (last_in + 1) + 5 + 3 < 2 ** 24
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    for go, kernels in ((last_in, "band"), (last_in + 1, "exact")):
        sc = Scoring("open=%d" % go, 3, -3, go, 1)
        exp = check(ctx, xs, y, pairs, sc, upload=False, kernels=kernels)
        assert exp["score"][0] == 18 and exp["score"][1] == 12
    # beyond the exact kernel's own float32 range: refused by name
    with pytest.raises(pgs.MI355Error) as e:
        ctx.affine_extend_run([0], [0], [8], gap_open=float(2 ** 23), gap_extend=1.0, band_lo=-2, band_hi=2)
    assert e.value.code == ENOTSUP and "pair 0 " in str(e.value)
    check(ctx, xs, y, pairs, upload=False)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, pgs):
    y = pgs.synth.dna(14201, 20_000).tobytes()
    xs = [pgs.synth.dna(14202, 6000).tobytes(), read_of(pgs, y, 14203, 50, 100)]
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    good = [Pair(1, 50, 300, -8, 8), Pair(1, 0, 150, -8, 8, back=1, to_end=1)]
    # 6000 rows under a band: beyond the band kernel and beyond the exact kernel's LDS: refused by name
    for call in (ctx.affine_extend_run, ctx.affine_extend_trace):
        with pytest.raises(pgs.MI355Error) as e:
            call([1, 0], [50, 0], [300, 9000], band_lo=-300, band_hi=300)
        assert e.value.code == ENOTSUP and "pair 1 " in str(e.value) and "banded" in str(e.value)
        check(ctx, xs, y, good, upload=False)
    # a band that misses the anchor's diagonal
    for blo, bhi in (([-8, 1], [8, 8]), ([-8, -8], [8, -1])):
        for call in (ctx.affine_extend_run, ctx.affine_extend_trace):
            with pytest.raises(pgs.MI355Error) as e:
                call([1, 1], [50, 60], [300, 300], band_lo=blo, band_hi=bhi)
            assert e.value.code == EINVAL and "band" in str(e.value)
    with pytest.raises(ValueError):
        ctx.affine_extend_run([1], [50], [300], band_lo=-8)
    # exactly one of the two NULL, and the unbanded calls' own checks in front of the band checks: nothing is written
    L = ctx._L
    p, keep = pgs.capi.make_affine_params()
    n = 2
    el = pgs.capi.ExtendList()
    qa, la, ra = (C.c_int32 * n)(1, 1), (C.c_int64 * n)(50, 60), (C.c_int64 * n)(300, 300)
    el.npairs, el.query, el.lefts, el.rights = n, qa, la, ra
    blo, bhi, bad = (C.c_int64 * n)(-8, -8), (C.c_int64 * n)(8, 8), (C.c_int64 * n)(-8, 1)
    f2, t2 = (C.c_float * n)(7, 7), (C.c_float * n)(7, 7)
    ex, ey, ty = (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()
    for lo_, hi_ in ((blo, None), (None, bhi), (bad, bhi)):
        assert L.mi355_sw_affine_extend_run_band(ctx._ctx, C.byref(el), lo_, hi_, C.byref(p), f2, ex, ey, t2, ty) == EINVAL
        assert L.mi355_sw_affine_extend_trace_band(ctx._ctx, C.byref(el), lo_, hi_, C.byref(p), None, res, t2, ty) == EINVAL
        assert len(L.mi355_sw_last_error(ctx._ctx)) > 0
    ra[1] = 20_001                                                      # the window check comes before the band check
    assert L.mi355_sw_affine_extend_run_band(ctx._ctx, C.byref(el), bad, bhi, C.byref(p), f2, ex, ey, t2, ty) == EINVAL
    assert b"window" in L.mi355_sw_last_error(ctx._ctx)
    ra[1] = 300
    assert list(f2) == [7, 7] and list(t2) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7] and list(ty) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)
    assert L.mi355_sw_affine_extend_run_band(ctx._ctx, C.byref(el), blo, bhi, C.byref(p), f2, ex, ey, t2, ty) == 0 and list(f2) != [7, 7]
    check(ctx, xs, y, good, upload=False)


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------------------
def fuzz_case(pgs, seed, alphabet, n_ref=6000, npairs=300):
    rng = np.random.default_rng(seed)
    y = si.letters(pgs, seed, n_ref, alphabet).tobytes()
    alpha = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    xs, pairs = [], []
    for k in range(60):
        m = int(rng.integers(1, 161))
        at = int(rng.integers(0, n_ref - m))
        x = np.frombuffer(y[at:at + m], dtype=np.uint8).copy()
        for _ in range(int(rng.integers(0, 1 + m // 12))):
            x[int(rng.integers(0, m))] = alpha[int(rng.integers(0, len(alpha)))]
        if m > 30 and k % 3 == 0:
            cut = int(rng.integers(5, m - 10))
            x = np.concatenate([x[:cut], x[cut + 3:], alpha[rng.integers(0, len(alpha), 3)]])
        if m > 30 and k % 3 == 1:
            cut = int(rng.integers(5, m - 10))
            x = np.concatenate([x[:cut], alpha[rng.integers(0, len(alpha), 4)], x[cut:m - 4]])
        xs.append((x.tobytes(), at))
    for k in range(npairs):
        q = int(rng.integers(0, len(xs)))
        x, at = xs[q]
        m = len(x)
        ql = int(rng.integers(0, m))
        qh = int(rng.integers(ql, m + 1)) if k % 5 else m
        n = int(rng.integers(0, 221))
        back = int(rng.integers(0, 2))
        if back:
            hi = min(n_ref, at + qh + int(rng.integers(0, 3)))
            lo = max(0, hi - n)
        else:
            lo = min(n_ref, max(0, at + ql - int(rng.integers(0, 3))))
            hi = min(n_ref, lo + n)
        if k % 17 == 0:
            lo = int(rng.integers(0, n_ref - 260))
            hi = lo + n
        half = int(rng.choice((0, 1, 2, 4, 8, 16, 32, 64, 100)))
        blo, bhi = -int(rng.integers(0, half + 1)), int(rng.integers(0, half + 1))
        if k % 11 == 0:
            blo, bhi = -(1 << 33), int(rng.integers(0, 5))
        pairs.append(Pair(q, lo, hi, blo, bhi, ql, qh, back, int(rng.integers(0, 2))))
    return [x for x, _ in xs], y, pairs


FUZZ = [Scoring("3/-3/5/1"), Scoring("3/-10/2/2", 3, -10, 2, 2), Scoring("1/-4/6/1", 1, -4, 6, 1)]


@pytest.mark.parametrize("sc", FUZZ, ids=[s.name for s in FUZZ])
def test_fuzz(ctx, pgs, sc):
    xs, y, pairs = fuzz_case(pgs, 14301, b"ACGT")
    exp = check(ctx, xs, y, pairs, sc, kernels="band")
    assert (exp["score"] >= 10 * sc.match).sum() > 30 and (exp["score"] == 0).sum() > 10 and (exp["to_end_score"] == NINF).sum() > 10
    assert ((exp["to_end_score"] < 0) & (exp["to_end_score"] > NINF)).sum() > 10


def test_fuzz_protein_table(ctx, pgs):
    lut = pgs.synth.make_lut(4242, 1.0)
    sc = Scoring("lut/aa20/11/1", gap_open=11, gap_extend=1, lut=lut)
    xs, y, pairs = fuzz_case(pgs, 14302, si.AA20)
    exp = check(ctx, xs, y, pairs, sc, kernels="band")
    assert (exp["score"] > 30).sum() > 30
