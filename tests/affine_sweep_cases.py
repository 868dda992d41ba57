"""Inputs and geometry arithmetic of tests/test_gpu_affine_sweep.py and tests/test_affine_sweep_cases_ref.py: the affine sweep
(sw_affine_kernel<R, SL> with affine_run / affine_sweep_launch of host_affine.h) run beyond its smallest configuration.  No GPU is
needed here: every input is a pure function of its arguments, the geometry is restated from the host's own expressions, and every
expected value comes from tests/affine_ref.py alone, computed once per process and shared by both test modules.

The cases are built against two mutations, either of which the earlier affine tests let pass:
  * `cg * NSLOT + slot` replaced by `slot` in sw_affine_kernel: every workgroup of a range then sweeps the first NSLOT tiles again
    and no column behind them is ever seen.  Cases A (and the workgroup tie of C) put the maximum behind them, and the CPU test
    shows that the first NSLOT tiles alone score strictly less.
  * the `- 63` dropped from `own_lo = first * sub_len - 63` in affine_run: the window of the exact kernel then begins at the first
    column of the sub-chunk the sweep named, and a maximum in the up to SL - 1 trailing columns of the sub-chunk before it, which
    the lagging lanes report with the next one, is not found again.  Cases B and C put maxima there, and the CPU test shows by the
    arithmetic below that they lie inside the host's window and outside the narrowed one.

What is where:
  A  WorkgroupCase   tiles beyond the first workgroup of a range (cg >= 1), idle workgroups, a one-column tile
  B  CutCase         an exact copy ending at every offset -17 .. +1 around a sub-chunk boundary and a tile boundary, in sub-chunk 0
                     (where own_lo clamps to 0) and in the last column of a range that is no multiple of the tile length
  C  TieCase         equal maxima in one sub-chunk, across a sub-chunk boundary, in two tiles, in two workgroups, at two rows
  D  bound_mix, long_and_empty, gap_open_bound   one call whose buckets go different ways
  E  ManyRanges      more ranges than one launch group of 32 768 holds

Not covered, because no input of test size reaches it: affine_sweep_launch splits a bucket's pairs over several launches once one
launch would sweep more than 2e13 cells (pairs_per_launch); every case here is one launch per bucket and launch group.

Scoring is 3 / -3 / 4 / 1 on ACGT unless a case says otherwise; SEP is a fifth letter that no query contains."""
import numpy as np

from tests import affine_ref, score_instances as si

SEP = ord("N")
REF_ARGS = (3, -3, 4, 1, None)                                      # match, mismatch, gap_open, gap_extend, lut of the checker
MATCH = 3
KSEG = 64                                                          # columns per segment (kSeg)
LOCATE_WIDEN = 63                                                  # the `- 63` of own_lo in affine_run
CL = 256                                                           # option `chunk` of cases A, E and the lone calls
GROUP = 32768                                                      # ranges per launch group of affine_run
# A copy of m letters scores MATCH * m, and only the last cell of an exact copy does: it is the unique maximum iff the query
# occurs once.  Among some 10^4 random columns a query of 12 letters occurs by chance with probability 10^4 / 4^12 < 0.001; a
# query of one letter (the shortest of shape 16 x 2) ties with every equal letter, so that shape's short query has 12.
MIN_UNIQUE = 12


# ---- geometry, as host_affine.h and sw_affine_kernel.h compute it --------------------------------------------------------------
def nslot(SL):
    """Tiles per workgroup (NSLOT)."""
    return 256 // SL


def sub_len(count, maxlen, chunk_len):
    """score_sub_len for a bucket of `count` queries, then affine_sweep_launch's fall-back to one sub-chunk per tile."""
    s = KSEG
    if count > 1:
        s = si.pow2_at_least(maxlen)
    if s > chunk_len or chunk_len % s:
        s = chunk_len
    return s


def tiles(n, chunk_len):
    return -(-n // chunk_len)


def cgroups(n, chunk_len, SL):
    """Workgroups per (pair, range) of a launch whose longest range has n columns."""
    return -(-tiles(n, chunk_len) // nslot(SL))


def tile_of(col, chunk_len):
    """Tile of the 1-based column `col` of a range."""
    return (col - 1) // chunk_len


def lane_of(row, R):
    """Lane of the 1-based row `row`: the lane lags lane 0 by as many columns."""
    return (row - 1) // R


def reported_sub(row, col, R, chunk_len, sublen):
    """The sub-chunk index under which the sweep publishes cell (row, col), 1-based, of a range: lane 0 publishes sub-chunk s of a
    tile once it has finished the tile's column (s + 1) * sublen, when lane k has finished k columns fewer; the tile's last
    sub-chunk is published after every lane has drained."""
    spt = chunk_len // sublen
    tile = tile_of(col, chunk_len)
    c = (col - 1) - tile * chunk_len
    s = c // sublen
    if s < spt - 1 and c > (s + 1) * sublen - 1 - lane_of(row, R):
        s += 1
    return tile * spt + s


def locate_window(first, sublen, n, widen=LOCATE_WIDEN):
    """(first, last) 1-based column of the range among which the exact kernel looks for the maximum of sub-chunk `first`."""
    return max(0, first * sublen - widen) + 1, min((first + 1) * sublen, n)


def in_window(col, win):
    return win[0] <= col <= win[1]


def occurrences(x, ref):
    """Number of (possibly overlapping) exact copies of x in ref."""
    k, at = 0, ref.find(x)
    while at >= 0:
        k, at = k + 1, ref.find(x, at + 1)
    return k


def _dna(pgs, seed, n):
    return si.letters(pgs, seed, n, b"ACGT").copy()


# ---- A: tiles beyond the first workgroup ---------------------------------------------------------------------------------------
WORKGROUP_SHAPES = [(16, 2), (16, 32), (8, 7), (8, 32)]


class WorkgroupCase:
    """One (reference, batch, ranges) of a tile shape (SL, R) under option chunk = CL; N = NSLOT, L / l = the longest / shortest
    query length of the shape's bucket (l at least MIN_UNIQUE).

    Ranges, none starting on a multiple of 4:
      0  starts at column 1 and spans 2 N + 3 tiles: three workgroups per pair (cg = 0, 1, 2), the last with three tiles
      1  five tiles: its workgroups with cg >= 1 have no tile at all
      2  N tiles and one column, ending at the reference's last column: its cg = 1 holds one tile of one column, its cg = 2 none
    Queries, in upload order; sorted by length the pairs are (1, 0) (2, 3) (4 alone):
      0  L, copy with 3 reference letters inserted at the last column of tile N - 1 and the first two of tile N of range 0: a gap
         that the last tile of one workgroup carries into the warm-up of the next workgroup's first
      1  l, exact copy ending in the reference's last column (range 2's tile of one column)
      2  L, exact copy ending inside tile 2 N + 1 of range 0
      3  L, unrelated
      4  L, two exact copies in range 0, ending in a tile of cg = 0 and in a tile of cg = 2: the first is the end cell
    Two copies of L = 512 letters do not fit side by side into the 2 CL + 130 columns of cg = 2 with query 2 ending in its middle
    tile, so for every shape query 2 begins with the second half of query 4 and the reference holds `query 4 | rest of query 2`:
    query 4's second copy ends L - L // 2 columns before query 2's.  Against query 4's first copy, query 2 scores half."""

    def __init__(self, pgs, shape, seed=0):
        lens, slot = si.shape_lengths(shape)
        SL, R = shape
        self.shape, self.slot = shape, slot
        N = self.N = nslot(SL)
        L, l = lens[-1], max(lens[0], MIN_UNIQUE)
        self.L, self.l = L, l
        base = 9000011 * (SL * 100 + R) + 131 * seed
        w0 = (2 * N + 2) * CL + 130
        r0 = (1, 1 + w0)
        r1 = (r0[1], r0[1] + 4 * CL + 77)
        n = r1[1] + 40
        n += (2 - n) % 4                                            # range 2 then starts one past a multiple of 4
        r2 = (n - (N * CL + 1), n)
        self.ranges = [r0, r1, r2]
        self.n = n
        assert all(a % 4 and b - a >= 1024 for a, b in self.ranges)
        ref = _dna(pgs, base + 1, n)
        h2 = L // 2
        q4 = _dna(pgs, base + 14, L)
        rest = _dna(pgs, base + 12, L - h2)
        q = [_dna(pgs, base + 10, L), _dna(pgs, base + 11, l), np.concatenate([q4[L - h2:], rest]), _dna(pgs, base + 13, L), q4]
        h = L // 2
        bnd = r0[0] + N * CL                                        # index of the first column of tile N of range 0
        p0 = np.concatenate([q[0][:h], _dna(pgs, base + 50, 3), q[0][h:]])
        at0 = bnd - 1 - h                                           # the inserted letters at indices bnd - 1 .. bnd + 1
        ref[at0:at0 + len(p0)] = p0
        at4 = r0[0] + CL + 57
        ref[at4:at4 + L] = q4
        seg = np.concatenate([q4, rest])
        e2 = r0[0] + (2 * N + 1) * CL + 100                         # index one past query 2's copy
        assert at4 + L < at0 and at0 + len(p0) < e2 - len(seg) and e2 < r0[1]
        ref[e2 - len(seg):e2] = seg
        ref[n - l:] = q[1]
        self.ref = ref.tobytes()
        self.queries = [v.tobytes() for v in q]
        # 1-based end columns, relative to range 0 (queries 2, 4) and to the whole reference
        self.q4_ends = (at4 + L - r0[0], e2 - (L - h2) - r0[0])
        self.q2_end = e2 - r0[0]
        self.q4_end_whole = at4 + L
        self.expected = None
        self.checks = None

    def geometry(self, n):
        """(chunk_len, sub_len, tiles, cgroups) of a launch whose longest range has n columns."""
        s = sub_len(5, self.L, CL)
        return CL, s, tiles(n, CL), cgroups(n, CL, self.shape[0])

    def compute(self):
        """Per-range maxima [3, nq] and (score, end_x, end_y)[nq] over the whole reference."""
        if self.expected is None:
            mx = np.array([affine_ref.locate_batch(self.queries, self.ref[lo:hi], *REF_ARGS)[0] for lo, hi in self.ranges])
            self.expected = (mx, affine_ref.locate_batch(self.queries, self.ref, *REF_ARGS))
        return self.expected

    def conditions(self):
        """What the inputs must hold, from the checker alone: dict(first_tiles = {query: (maximum over the first N tiles of its
        range, maximum over the range)}, faults = [...] as tests/test_gpu_affine.py's Case, copies = query 4's two copies)."""
        if self.checks is None:
            mx = self.compute()[0]
            span = self.N * CL
            first = {}
            for k, r in ((1, 2), (2, 0)):
                lo = self.ranges[r][0]
                first[k] = (affine_ref.locate(self.queries[k], self.ref[lo:lo + span], *REF_ARGS)[0], float(mx[r, k]))
            lo, hi = self.ranges[0]
            faults = []
            lin = [affine_ref.locate(self.queries[0], self.ref[lo:hi], 3, -3, g, g)[0] for g in (REF_ARGS[2], REF_ARGS[3])]
            if mx[0, 0] == lin[0] or mx[0, 0] == lin[1]:
                faults.append("query 0 in range 0: affine %g, linear %g at open, %g at extend: the gap does not matter" % (mx[0, 0], lin[0], lin[1]))
            copies = []
            for e in self.q4_ends:                                  # each copy alone, in a slice that holds nothing else of query 4
                a = lo + e - self.L - 8
                s, i, j = affine_ref.locate(self.queries[4], self.ref[a:lo + e + 8], *REF_ARGS)
                copies.append((s, i, a + j - lo))
            self.checks = dict(first_tiles=first, faults=faults, copies=copies)
        return self.checks


_workgroup = {}


def workgroup_case(pgs, shape):
    if shape not in _workgroup:
        _workgroup[shape] = WorkgroupCase(pgs, shape)
    return _workgroup[shape]


# ---- B: the end column around every cut ----------------------------------------------------------------------------------------
CUT_SHAPES = [(8, 7), (16, 4)]
CUT_OFFSETS = tuple(range(-17, 2))
CUT_N = 2 * 1024 + 300
# (chunk_len, sub_len) of the two configurations: a batch under option chunk = 1024, a lone call under chunk = 256
BATCH_GEOMETRY = (1024, 256)
LONE_GEOMETRY = (CL, KSEG)
# query index -> the cut B its copy ends at B + d.  512 is a sub-chunk boundary inside a tile of the batch and a tile boundary of the
# lone call, 1024 a tile boundary of both, 1152 = 4 * 256 + 128 a sub-chunk boundary inside a tile of the lone call.
CUT_AT = {0: 512, 1: 1024, 2: 1152}
CUT_KINDS = {"batch": {"sub": 0, "tile": 1}, "lone": {"sub": 2, "tile": 1}}


class CutCase:
    """One reference of CUT_N columns and five queries of a shape (SL, R), each with one exact copy, for an offset d:
      0, 1, 2  L rows, ending at column CUT_AT[k] + d
      3        m0 rows, ending inside sub-chunk 0 at column m0, m0 + 1 or 63 (by d, in turn): the own_lo clamp.  m0 = L where
               L + 1 <= 63 leaves all three inside the lone call's first 64 columns, else the bucket's shortest length
      4        L rows, ending at the last column; CUT_N is no multiple of either tile length
    Every copy ends at its query's last row, which lies in the tile's last lane: the greatest lag, SL - 1 columns."""

    def __init__(self, pgs, shape, d):
        lens, slot = si.shape_lengths(shape)
        assert slot == 0
        SL, R = shape
        self.shape, self.d = shape, d
        L = self.L = lens[-1]
        m0 = L if L + 1 <= 63 else lens[0]
        assert m0 + 1 <= 63
        c0 = (m0, m0 + 1, 63)[(d - CUT_OFFSETS[0]) % 3]
        base = 5000011 * (SL * 100 + R) + 1009 * (d - CUT_OFFSETS[0])
        n = CUT_N
        ref = _dna(pgs, base + 1, n)
        self.ends = [CUT_AT[0] + d, CUT_AT[1] + d, CUT_AT[2] + d, c0, n]
        q = [_dna(pgs, base + 10 + k, m0 if k == 3 else L) for k in range(5)]
        last = 0
        for k in sorted(range(5), key=lambda k: self.ends[k]):
            e = self.ends[k]
            assert e - len(q[k]) >= last, "copies must not overlap"
            ref[e - len(q[k]):e] = q[k]
            last = e
        self.ref = ref.tobytes()
        self.queries = [v.tobytes() for v in q]
        self.expected = None

    def compute(self):
        if self.expected is None:
            self.expected = affine_ref.locate_batch(self.queries, self.ref, *REF_ARGS)
        return self.expected


_cut = {}


def cut_case(pgs, shape, d):
    if (shape, d) not in _cut:
        _cut[(shape, d)] = CutCase(pgs, shape, d)
    return _cut[(shape, d)]


# ---- C: ties -------------------------------------------------------------------------------------------------------------------
TIE_SHAPE = (16, 2)
TIE_M = 32                                                         # the shape's longest query: its last row lies in lane 15
TIE_HALF = 14                                                      # |a| = |b| of the row ties: MATCH * 14 = 42 is below the cost 4 + 39 of
TIE_SEP = 40                                                       # a gap over the 40 separators, so no alignment joins the two pieces
TIE_TRAILING = (1, 8, 15)
TIE_NAMES = ("same_sub", "trailing_1", "trailing_8", "trailing_15", "two_tiles", "rows_b_a", "rows_a_b", "two_workgroups")


class TieCase:
    """One reference and the queries of a configuration, `batch` (chunk 1024, sub-chunks of 256) or `lone` (chunk 256, sub-chunks
    of 64; four sub-chunks per tile either way).  Each query has two cells that hold its maximum, `first` before `second` in
    column-major order; (row, column), 1-based:
      same_sub      two exact copies ending inside sub-chunk 1 of tile 0
      trailing_k    the first copy ends in the k-th last column of sub-chunk 1 of tile 1 / 2 / 3 (k = 1, 8, 15: all reported with
                    sub-chunk 2 by lane 15), the second in the body of sub-chunk 2
      two_tiles     copies in tiles 4 and 5
      rows_b_a      x = a + b, the reference holds b, 40 separators, a between 40 separators (tile 6): (|x|, earlier column) ties with (|a|, later column)
      rows_a_b      the reference holds a, 40 separators, b (tile 7): (|a|, earlier column) ties with (|x|, later column)
      two_workgroups  lone only: copies in tiles 9 and 17, the second in the range's second workgroup.  The batch form is case A's
                    query 4."""

    def __init__(self, pgs, config):
        self.config = config
        cl, sl = self.geometry = BATCH_GEOMETRY if config == "batch" else LONE_GEOMETRY
        lone = config == "lone"
        self.n = n = (18 * cl + 100) if lone else (8 * cl + 300)
        base = 3000017 + (7 if lone else 0)
        ref = _dna(pgs, base + 1, n)
        self.names = [t for t in TIE_NAMES if lone or t != "two_workgroups"]
        self.queries, self.first, self.second = [], [], []

        def copies(k, e1, e2):
            x = _dna(pgs, base + 10 + k, TIE_M)
            assert e1 - TIE_M >= 0 and e2 - TIE_M >= e1 and e2 <= n
            ref[e1 - TIE_M:e1] = x
            ref[e2 - TIE_M:e2] = x
            self.queries.append(x.tobytes())
            self.first.append((TIE_M, e1))
            self.second.append((TIE_M, e2))

        copies(0, sl + 10, sl + 50)
        for t, k in enumerate(TIE_TRAILING, start=1):
            B = t * cl + 2 * sl
            copies(t, B - k + 1, B + 40)
        copies(4, 4 * cl + 32, 5 * cl + 2 * sl + 40)
        for k, tile, b_first in ((5, 6, True), (6, 7, False)):
            a, b = _dna(pgs, base + 30 + k, TIE_HALF), _dna(pgs, base + 40 + k, TIE_HALF)
            p = tile * cl + 5 + TIE_SEP
            pieces = (b, a) if b_first else (a, b)
            sep = np.full(TIE_SEP, SEP, dtype=np.uint8)                # in front and behind too: no flank extends a piece
            ref[p - TIE_SEP:p + 2 * TIE_HALF + 2 * TIE_SEP] = np.concatenate([sep, pieces[0], sep, pieces[1], sep])
            self.queries.append(np.concatenate([a, b]).tobytes())
            rows = (2 * TIE_HALF, TIE_HALF) if b_first else (TIE_HALF, 2 * TIE_HALF)
            self.first.append((rows[0], p + TIE_HALF))
            self.second.append((rows[1], p + 2 * TIE_HALF + TIE_SEP))
        if lone:
            copies(7, 9 * cl + 40, 17 * cl + 40)
        self.ref = ref.tobytes()
        self.expected = None

    def compute(self):
        if self.expected is None:
            self.expected = affine_ref.locate_batch(self.queries, self.ref, *REF_ARGS)
        return self.expected


_tie = {}


def tie_case(pgs, config):
    if config not in _tie:
        _tie[config] = TieCase(pgs, config)
    return _tie[config]


# ---- D: mixed dispatch in one call ---------------------------------------------------------------------------------------------
MIX_N = 1500
BOUND_SCORING = (8, -5, 6, 2, None)                                # smax * (rows + 1) <= 2040 holds for 100 rows and not for 300
_mixed = {}


def _mixed_case(key, build, args):
    if key not in _mixed:
        ref, qs = build()
        _mixed[key] = (ref, qs, affine_ref.locate_batch(qs, ref, *args))
    return _mixed[key]


def bound_mix(pgs):
    """(reference, queries, expected): three queries of 100 rows (an exact copy, a copy with two reference letters inserted,
    unrelated) and two of 300 (an exact copy, unrelated) under BOUND_SCORING."""
    def build():
        ref = _dna(pgs, 8101, MIX_N)
        q = [_dna(pgs, 8110 + k, m) for k, m in enumerate((100, 300, 100, 300, 100))]
        ref[150:250] = q[0]
        ref[400:450], ref[452:502] = q[2][:50], q[2][50:]
        ref[900:1200] = q[1]
        return ref.tobytes(), [v.tobytes() for v in q]
    return _mixed_case("bound", build, BOUND_SCORING)


def long_and_empty(pgs):
    """(reference, queries, expected): queries of 150, 600, 0, 513 and 150 rows; the 600 rows end in the last column, the 513 are a
    copy with three of their letters missing in the reference."""
    def build():
        ref = _dna(pgs, 8201, MIX_N)
        q = [_dna(pgs, 8210 + k, m) for k, m in enumerate((150, 600, 0, 513, 150))]
        ref[100:250] = q[0]
        ref[350:860] = np.concatenate([q[3][:256], q[3][259:]])
        ref[MIX_N - 600:] = q[1]
        return ref.tobytes(), [v.tobytes() for v in q]
    return _mixed_case("long", build, REF_ARGS)


def gap_open_bound(pgs, gap_open):
    """(reference, queries, expected) under 3 / -3 / gap_open / 1: three queries of 150 rows, an exact copy, a copy with two reference
    letters inserted, unrelated."""
    def build():
        ref = _dna(pgs, 8301, MIX_N)
        q = [_dna(pgs, 8310 + k, 150) for k in range(3)]
        ref[200:350] = q[0]
        ref[700:775], ref[777:852] = q[1][:75], q[1][75:]
        return ref.tobytes(), [v.tobytes() for v in q]
    return _mixed_case(("open", gap_open), build, (3, -3, gap_open, 1, None))


# ---- E: more ranges than one launch group --------------------------------------------------------------------------------------
class ManyRanges:
    """32 771 ranges, range k = distinct[k % 7]: 32768 % 7 = 1, so the second launch group begins at distinct[1] and a decode that
    forgot the group's offset would give it the rows of distinct[0 .. 2].  Four queries of 16 to 32 rows (one bucket of 16 x 2); the
    copy of query 3 lies inside distinct[2], [4] and [5] only, the copy of query 1 inside [0], [2], [3] and [4]."""
    COUNT = GROUP + 3
    DISTINCT = [(1, 1100), (5, 1040), (130, 1700), (403, 1427), (777, 2100), (1203, 2700), (1901, 3000)]

    def __init__(self, pgs):
        n = 3000
        ref = _dna(pgs, 8401, n)
        q = [_dna(pgs, 8410 + k, m) for k, m in enumerate((16, 20, 27, 32))]
        ref[1500:1532] = q[3]
        ref[1050:1070] = q[1]
        self.ref = ref.tobytes()
        self.queries = [v.tobytes() for v in q]
        self.ranges = [self.DISTINCT[k % 7] for k in range(self.COUNT)]
        assert all(hi - lo >= 1024 for lo, hi in self.DISTINCT) and len({lo for lo, _ in self.DISTINCT}) == 7
        self.expected = None

    def compute(self):
        """(maxima of the seven distinct ranges [7, nq], of all ranges [COUNT, nq])."""
        if self.expected is None:
            seven = np.array([affine_ref.locate_batch(self.queries, self.ref[lo:hi], *REF_ARGS)[0] for lo, hi in self.DISTINCT])
            self.expected = (seven, seven[np.arange(self.COUNT) % 7])
        return self.expected


_many = []


def many_ranges(pgs):
    if not _many:
        _many.append(ManyRanges(pgs))
    return _many[0]
