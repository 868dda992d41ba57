"""Inputs and bookkeeping of tests/test_gpu_affine_big_list.py: affine pair lists LONGER THAN ONE LAUNCH of the exact and traceback
kernels (csrc/host_affine.h: 65 536 problems per launch of sw_affine_exact_* and sw_affine_trace_*, 2^24 row words per launch of the
rows instance, 2^30 decision bytes per traceback group), with every field of every pair against the family's checker.

Small per pair, large in count.  One reference of 4000 letters with eight anchor positions, 57 resident reads of 12 to 40 rows, and
per FAMILY (local, band, e2e, extend, extend_band, zdrop, global and global_band) a dictionary of D = 256 pairwise distinct entries
(query, window, band, sub-range, direction, to_end) in eight classes BY INDEX (d mod 8):

  d mod 8   local / band / e2e                               extend / extend_band / zdrop                 global / global_band
  0  zero   an empty window: no job, the zeros stand         an empty sub-range (m = 0): no job          m = n = 0: no job
  1  hit    a copy with one substitution                     the same, anchored                            the same, corner to corner
  2  ins    three letters inserted: "3I" in the CIGAR        the same                                      the same
  3  tie    two equal maxima, the first must win (e2e: a     36 at (12, 12) and at (14, 14)                the ONE pair of the other kind:
            repeat in the window; else 36 twice on a diagonal)                                            banded in `global`, plain in `global_band`
  4  long   40 rows: another instance R (band: a wider       the same, traced to_end (band: a narrower    the same
            band, another instance of the band kernel)       band, another instance)
  5  none   a read of N: no positive cell — local, band:     best extension 0 at the anchor; traced       a negative score, traced
            zeros, no traceback; e2e: negative, traced       to_end it ends in COLUMN 0: no kernel
  6  del    three columns skipped: "3D" in the CIGAR         the same                                      the same
  7  edge   a hit that ends in the window's last column      a sub-range of the read, BACKWARD, to_end    a sub-range, backward

At most two classes of a family produce no traceback job.  A list of n pairs is the dictionary indexed by seq(k) = (A k + B) mod 256 with
A odd, so the checker runs 256 times per family and not n times, and — A being a unit mod 8 — ANY eight consecutive pairs hold all
eight classes: whichever contiguous part of a list a launch loses, it loses pairs of every class.

Every checked call is preceded, on the same context, by the same call on prev(k) = seq(k + STRIDE).  A * STRIDE = 4 mod 8, so the
class of prev(k) is the class of seq(k) plus four: zero <-> long, hit <-> none, ins <-> del, tie <-> edge.  The device buffers
(outs_f, outs_i, hmat, dirs, cons) live on the context across calls, so a problem that a launch skips, or whose pointer is re-based
wrongly, keeps or reads what the preceding call left — by construction never what the checked list expects, and never two empty
results.  tests/test_affine_big_list_ref.py asserts all of this with the checkers alone.

N = 88 001 (odd: no multiple of 16, 64 or 256) gives every exact stage and every traceback pass under test more than 65 536 jobs;
stage_jobs() states the job count of every stage from the checker's values, and launches() what the host's cut makes of them."""
import functools

import numpy as np

from tests import affine_band_ref, affine_e2e_ref, affine_extend_band_ref, affine_extend_ref, affine_global_ref, affine_ref, affine_trace_ref, affine_zdrop_ref
from tests.test_gpu_affine_extend_band import Pair

D = 256
A, B, STRIDE = 77, 5, 52
SHIFT = (A * STRIDE) % D                                             # dictionary index of prev(k) = that of seq(k) + SHIFT
assert A % 2 == 1 and (A * STRIDE) % 8 == 4 and SHIFT % 8 == 4
N = 88001
assert N % 16 and N % 64 and N % 256
LAUNCH = 65536                                                       # problems per launch of an exact or a traceback kernel
ROW_WORDS = 1 << 24                                                  # row words per launch of the rows instance (two per row)
TRACE_BYTES = 1 << 30                                                # decision bytes of one traceback group
CLASSES = ("zero", "hit", "ins", "tie", "long", "none", "del", "edge")
FAMILIES = ("local", "band", "e2e", "extend", "extend_band", "zdrop", "global", "global_band")
SC = dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0)
ZDROP = 10.0
NINF = float("-inf")
BIG = 1 << 40                                                        # a band that covers everything: a plain pair in a banded list
OTHER = {65: 67, 67: 71, 71: 84, 84: 65}                             # a letter that mismatches: A -> C -> G -> T -> A
STRINGS = ("cons_x", "cons_y", "cigar")

PAIRS_RUN = ("score", "end_x", "end_y")
PAIRS_TRACE = PAIRS_RUN + ("begin_x", "begin_y", "pos") + STRINGS
EXT_RUN = ("score", "end_x", "end_y", "to_end_score", "to_end_y")
EXT_TRACE = EXT_RUN + ("pos",) + STRINGS
FIELDS = {
    "local": (PAIRS_RUN, PAIRS_TRACE), "band": (PAIRS_RUN, PAIRS_TRACE), "e2e": (PAIRS_RUN, PAIRS_TRACE),
    "extend": (EXT_RUN, EXT_TRACE), "extend_band": (EXT_RUN, EXT_TRACE),
    "zdrop": (EXT_RUN + ("rows_done",), EXT_TRACE + ("rows_done",)),
    "global": (("score",), ("score", "end_x", "end_y", "pos") + STRINGS), "global_band": (("score",), ("score", "end_x", "end_y", "pos") + STRINGS),
}

NPOS = 8
KINDS = ("hit", "ins", "del", "tie", "long", "edge", "repeat")       # the reads of one position; one read of N serves every position
YLEN = 4000


def anchor(t):
    return 200 + 450 * t


@functools.lru_cache(maxsize=None)
def reference():
    """4000 letters; 200 letters behind every anchor its first 12 letters stand a second time (the end-to-end tie)."""
    rng = np.random.default_rng(20270)
    y = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, YLEN)].tobytes())
    for t in range(NPOS):
        a = anchor(t)
        y[a + 200:a + 212] = y[a:a + 12]
    return bytes(y)


def _sub(s, at):
    return s[:at] + bytes([OTHER[s[at]]]) + s[at + 1:]


@functools.lru_cache(maxsize=None)
def reads():
    """The resident batch: KINDS for each of the 8 positions, then the read of N."""
    y = reference()
    out = []
    for t in range(NPOS):
        a = anchor(t)
        s = y[a:a + 60]
        out += [_sub(s[:30], 13),                                    # hit: 30 rows
                s[:14] + b"NNN" + s[14:28],                          # ins: 31 rows
                s[:15] + s[18:33],                                   # del: 30 rows
                s[:12] + bytes([OTHER[s[12]]]) + s[13:14] + b"N" * 12,  # tie: 26 rows, 36 at (12, 12) and at (14, 14), then it falls: under the
                                                             # z-drop it stops once column 14 has left the band (row 25)
                _sub(s[:40], 21),                                    # long: 40 rows
                s[5:35],                                             # edge: 30 rows
                s[:12]]                                              # repeat: 12 rows, twice in its window
    out.append(b"N" * 25)
    assert len(out) <= 64 and all(12 <= len(x) <= 40 for x in out)
    return out


def rid(kind, t):
    return len(KINDS) * NPOS if kind == "none" else len(KINDS) * t + KINDS.index(kind)


def _entry(family, d):
    c, j = CLASSES[d % 8], d // 8
    t, v = j % NPOS, j // NPOS                                       # position, variant 0..3: what makes the entries of a class distinct
    a = anchor(t)
    xs = reads()
    if family in ("local", "band", "e2e"):
        f = 2 + 3 * v                                                # the flank in front of the read: the hit's diagonal j - i
        kind = "repeat" if (family == "e2e" and c == "tie") else ("hit" if c == "zero" else c)
        q = rid(kind, t)
        lo, hi = a - f, a + 50 + v
        if c == "zero":
            hi = lo
        elif c == "edge":
            hi = a + 35
        elif kind == "repeat":
            hi = a + 215
        blo = bhi = None
        if family == "band":
            blo, bhi = (f - 10, f + 25) if c == "long" else (f - 6, f + 10)   # 36 diagonals, else 17
        return Pair(q, lo, hi, blo, bhi)
    glob = family in ("global", "global_band")
    banded = family in ("extend_band", "zdrop") or (glob and (family == "global") == (c == "tie"))
    kind = "hit" if (c == "zero" or (glob and c == "tie")) else c
    q = rid(kind, t)
    m = len(xs[q])
    q_lo, q_hi, back, lo = 0, m, 0, a
    if glob:
        hi = a + {"hit": 30, "ins": 28, "del": 33, "long": 40, "none": 25, "edge": 30}.get(kind, 30) + v
        te = 0
    else:
        hi = a + m + 12 + 3 * v
        te = 1 if c in ("long", "none", "edge") else 0
    if glob and c == "del":                                          # (a shorter sub-range per variant: no score of `ins` comes back here)
        q_hi, hi = m - 2 * v - 1, a + 33 - 2 * v - 1
    if c == "zero":
        q_lo = q_hi = 5 + v
        if glob:
            lo = hi = a + v
    elif c == "edge":                                                # letters 2 .. 30 of s[5:35] are s[7:35]: backward, anchored behind a + 35
        q_lo, back = 2, 1
        lo, hi = (a + 7 - v, a + 35) if glob else (a + 7 - 10 - 3 * v, a + 35)
    elif c == "none" and family in ("extend_band", "zdrop"):
        q_hi = 8                                                     # the whole of column 0 down to row m stays in the band
    blo = bhi = None
    if banded:
        blo, bhi = (-5, 5) if (c == "long" and not glob) else (-8, 8)
    return Pair(q, lo, hi, blo, bhi, q_lo, q_hi, back, te)


@functools.lru_cache(maxsize=None)
def entries(family):
    """The D entries of a family, class by index."""
    return tuple(_entry(family, d) for d in range(D))


def key(p):
    return (p.q, p.lo, p.hi, p.blo, p.bhi, p.q_lo, p.q_hi, p.back, p.to_end)


def _zeros(fields):
    return {f: ("" if f in STRINGS else 0) for f in fields}


def _pick(rec, fields):
    return {f: rec[f] for f in fields}


def _check(family, p):
    """(run record, trace record) of one entry by the family's checker."""
    xs, y = reads(), reference()
    run_f, trace_f = FIELDS[family]
    w = y[p.lo:p.hi]
    if family in ("local", "band", "e2e"):
        x = xs[p.q]
        if not x or not w:
            return _zeros(run_f), _zeros(trace_f)
        if family == "local":
            loc, tr = affine_ref.locate(x, w, **SC), affine_trace_ref.trace(x, w, **SC)
        elif family == "band":
            loc, tr = affine_band_ref.locate(x, w, p.blo, p.bhi, **SC), affine_band_ref.trace(x, w, p.blo, p.bhi, **SC)
        else:
            loc, tr = affine_e2e_ref.locate(x, w, **SC), affine_e2e_ref.trace(x, w, **SC)
        return dict(zip(run_f, (float(loc[0]), int(loc[1]), int(loc[2])))), _pick(tr, trace_f)
    x = xs[p.q][p.q_lo:p.q_hi]
    back, te = bool(p.back), bool(p.to_end)
    if family == "extend":
        return _pick(affine_extend_ref.locate(x, w, back, **SC), run_f), _pick(affine_extend_ref.trace(x, w, back, te, **SC), trace_f)
    if family == "extend_band":
        return (_pick(affine_extend_band_ref.locate(x, w, p.blo, p.bhi, back, **SC), run_f),
                _pick(affine_extend_band_ref.trace(x, w, p.blo, p.bhi, back, te, **SC), trace_f))
    if family == "zdrop":
        return (_pick(affine_zdrop_ref.locate(x, w, p.blo, p.bhi, ZDROP, back, **SC), run_f),
                _pick(affine_zdrop_ref.trace(x, w, p.blo, p.bhi, ZDROP, back, te, **SC), trace_f))
    return (dict(score=affine_global_ref.score(x, w, p.blo, p.bhi, back, **SC)),
            _pick(affine_global_ref.trace(x, w, p.blo, p.bhi, back, **SC), trace_f))


@functools.lru_cache(maxsize=None)
def records(family):
    """(run records, trace records) of the D entries: computed once, shared and left unchanged."""
    both = [_check(family, p) for p in entries(family)]
    return tuple(b[0] for b in both), tuple(b[1] for b in both)


def seq(n, shift=0):
    """Dictionary index of every pair of a list of n: the checked list (shift 0), the one that precedes it (shift STRIDE)."""
    k = np.arange(n, dtype=np.int64) + shift
    return (A * k + B) % D


def gather(recs, fields, idx):
    """The expectation of a list: numeric fields as float64 arrays, strings as lists."""
    out = {}
    for f in fields:
        col = [r[f] for r in recs]
        out[f] = [col[d] for d in idx] if f in STRINGS else np.array(col, dtype=np.float64)[idx]
    return out


def call_args(family, ps):
    """(query, lefts, rights, keyword arguments of the run call, those of the trace call beyond them) of a list of entries."""
    q, lo, hi = [p.q for p in ps], [p.lo for p in ps], [p.hi for p in ps]
    if family in ("local", "band", "e2e"):
        kw = dict(mode="end_to_end") if family == "e2e" else {}
        if family == "band":
            kw.update(band_lo=[p.blo for p in ps], band_hi=[p.bhi for p in ps])
        return q, lo, hi, kw, {}
    kw = dict(q_lo=[p.q_lo for p in ps], q_hi=[p.q_hi for p in ps], backward=[p.back for p in ps])
    if any(p.blo is not None for p in ps):
        kw.update(band_lo=[-BIG if p.blo is None else p.blo for p in ps], band_hi=[BIG if p.bhi is None else p.bhi for p in ps])
    if family == "zdrop":
        kw.update(zdrop=ZDROP)
    return q, lo, hi, kw, ({} if family.startswith("global") else dict(to_end=[p.to_end for p in ps]))


# ---- what the host makes of a list: jobs per stage, launches ---------------------------------------------------------------------------
def geometry(family, p):
    """(m, n, banded, W): rows, columns, whether the host treats the entry as a banded pair, and the diagonals of its clipped band."""
    xs = reads()
    if family in ("local", "band", "e2e"):
        m, n = len(xs[p.q]), p.hi - p.lo
        if p.blo is None:
            return m, n, False, 0
        lo_e, hi_e = max(p.blo, 1 - m), min(p.bhi, n - 1)
        return m, n, (lo_e, hi_e) != (1 - m, n - 1), hi_e - lo_e + 1
    m, n = p.q_hi - p.q_lo, p.hi - p.lo
    if p.blo is None:
        return m, n, False, 0
    lo_e, hi_e = max(p.blo, -m), min(p.bhi, n)
    return m, n, family == "zdrop" or (lo_e, hi_e) != (-m, n), hi_e - lo_e + 1


def has_job(family, p):
    """Does the entry reach a score kernel (else the host fills it in)?"""
    m, n, banded, W = geometry(family, p)
    if m < 1 or n < 1:
        return False
    if family.startswith("global"):
        return affine_global_ref.reachable(m, n, p.blo, p.bhi)
    return not (p.blo is not None and W < 1)


def has_trace_job(family, p, tr):
    """Does the trace call run a traceback problem for the entry (tr: its trace record)?"""
    if family in ("local", "band"):
        return tr["score"] > 0
    return tr["end_x"] >= 1 and tr["end_y"] >= 1                     # (a cell in column 0 or row 0 is written by the host)


def stage_jobs(family, n=N, shift=0):
    """Jobs of a list of n pairs per stage when every pair goes to the exact kernels: dict(exact={stage: jobs}, trace={pass: jobs}),
    the stages "plain" and "band" (the unbanded and the banded instance; z-drop: "rows" beside "band"), from the checker's values."""
    es, (_, tr) = entries(family), records(family)
    per = np.bincount(seq(n, shift), minlength=D)
    out = dict(exact={}, trace={})
    for d, p in enumerate(es):
        stage = "band" if geometry(family, p)[2] else "plain"
        if has_job(family, p):
            out["exact"][stage] = out["exact"].get(stage, 0) + int(per[d])
        if has_trace_job(family, p, tr[d]):
            out["trace"][stage] = out["trace"].get(stage, 0) + int(per[d])
    if family == "zdrop":
        out["exact"]["rows"] = out["exact"]["band"]
    return out


def launches(jobs):
    """Launches of the stages of one kind: 65 536 problems each (test_affine_big_list_ref.py: no other bound cuts these lists)."""
    return sum(-(-v // LAUNCH) for v in jobs.values())


def dirs_upper(family, n=N):
    """An upper bound of the decision bytes of a list's tracebacks: every entry's whole matrix."""
    per = np.bincount(seq(n), minlength=D)
    return sum(int(per[d]) * dirs_bytes(*geometry(family, p)[:2]) for d, p in enumerate(entries(family)))


def pair_R(R_list, m):
    return min(r for r in R_list if 16 * r >= m)


def list_instances(family, pair_Rs, band_Rs):
    """The distinct (geometry, R) of the list kernels the default dispatch launches for the family's entries."""
    out = set()
    for p in entries(family):
        if has_job(family, p):
            m, n, banded, W = geometry(family, p)
            out.add(("band", pair_R(band_Rs, W)) if banded else ("pair", pair_R(pair_Rs, m)))
    return out


# ---- the word bound of the rows instance: 150-row reads under the z-drop ------------------------------------------------------------
WORD_D = 48
WORD_A, WORD_B = 5, 1
WORD_SHIFT = (WORD_A * STRIDE) % WORD_D                              # kind of entry d: d mod 3; the preceding list's kind is another one
assert np.gcd(WORD_A, WORD_D) == 1 and WORD_SHIFT % 3 != 0
WORD_ROWS = 150
WORD_PER_LAUNCH = ROW_WORDS // (2 * WORD_ROWS)                       # 55 924 problems: the word bound cuts before 65 536
WORD_N = 56001
assert WORD_PER_LAUNCH < WORD_N < LAUNCH and WORD_N % 16 and WORD_N > WORD_PER_LAUNCH
WORD_ZDROP = 20.0


@functools.lru_cache(maxsize=None)
def word_reads():
    """24 reads of 150 rows: per position a copy with substitutions, one that falls after 60 letters and one with a skipped block."""
    y = reference()
    out = []
    for t in range(NPOS):
        s = y[anchor(t):anchor(t) + 220]
        out += [_sub(_sub(s[:150], 40), 111),
                s[:60] + b"N" * 90,                                  # stops early under the z-drop
                s[:70] + s[73:153]]
    assert all(len(x) == WORD_ROWS for x in out)
    return out


@functools.lru_cache(maxsize=None)
def word_entries():
    out = []
    for d in range(WORD_D):
        kind, j = d % 3, d // 3
        t, v = j % NPOS, j // NPOS
        out.append(Pair(3 * t + kind, anchor(t), anchor(t) + 160 + 5 * v, -8, 8, 0, WORD_ROWS, 0, (d // 3) % 2))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def word_records():
    xs, y = word_reads(), reference()
    run_f, trace_f = FIELDS["zdrop"]
    both = [(_pick(affine_zdrop_ref.locate(xs[p.q], y[p.lo:p.hi], p.blo, p.bhi, WORD_ZDROP, False, **SC), run_f),
             _pick(affine_zdrop_ref.trace(xs[p.q], y[p.lo:p.hi], p.blo, p.bhi, WORD_ZDROP, False, bool(p.to_end), **SC), trace_f))
            for p in word_entries()]
    return tuple(b[0] for b in both), tuple(b[1] for b in both)


def word_seq(n, shift=0):
    k = np.arange(n, dtype=np.int64) + shift
    return (WORD_A * k + WORD_B) % WORD_D


def rows_launches(ms):
    """Launches of the rows instance over problems of ms rows, in order: at most 65 536 problems and 2^24 row words each."""
    count, k = 0, 0
    while k < len(ms):
        hi, words = k, 0
        while hi < len(ms) and hi - k < LAUNCH and (hi == k or words + 2 * ms[hi] <= ROW_WORDS):
            words += 2 * ms[hi]
            hi += 1
        count, k = count + 1, hi
    return count


# ---- the byte budget of a traceback group: 22 pairs of about 5000 x 5000 cells ---------------------------------------------------------
BUDGET_PAIRS = 22
BUDGET_ROWS = 4990


def budget_reference(rows=BUDGET_ROWS, pairs=BUDGET_PAIRS):
    rng = np.random.default_rng(20271)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, rows + pairs + 64)].tobytes()


def budget_case(rows=BUDGET_ROWS, pairs=BUDGET_PAIRS):
    """(y, reads, windows): read k is y[k : k + rows + k] with ONE substitution at a position that depends on k, against exactly its own
    window — the answer is known: score 3 (m - 1) - 3, CIGAR mM, the strings are the read and the window (reversed)."""
    y = budget_reference(rows, pairs)
    xs, wins = [], []
    for k in range(pairs):
        m = rows + k
        xs.append(_sub(y[k:k + m], (7 + 13 * k) % (m - 10) + 5))
        wins.append((k, k + m))
    return y, xs, wins


def budget_expected(y, xs, wins):
    """The answers by construction, as the pairs calls and the extension calls return them."""
    rows = []
    for x, (lo, hi) in zip(xs, wins):
        m = len(x)
        rows.append(dict(score=3.0 * (m - 1) - 3.0, end_x=m, end_y=m, begin_x=1, begin_y=1, pos=1, to_end_score=3.0 * (m - 1) - 3.0, to_end_y=m,
                         cons_x=x[::-1].decode(), cons_y=y[lo:hi][::-1].decode(), cigar="%dM" % m))
    return rows


def dirs_bytes(m, nw):
    """Decision bytes of a traceback problem of m rows and nw columns, rounded as a group lays them out."""
    return ((m + nw + 1) * max(1, min(m, nw)) + 16 + 15) & ~15


def trace_groups(sizes):
    """Problems per launch group of a traceback pass over problems of the given decision bytes, in order."""
    out, k = [], 0
    while k < len(sizes):
        hi, total = k, 0
        while hi < len(sizes) and hi - k < LAUNCH and not (hi > k and total + sizes[hi] > TRACE_BYTES):
            total += sizes[hi]
            hi += 1
        out.append(hi - k)
        k = hi
    return out
