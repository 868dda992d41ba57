"""Inputs and bookkeeping of tests/test_gpu_lone_strip_instances.py: the table of compiled sw_score_kernel instances read from
host_score.h, the host's choice for a LONE query and for STRIP-MINED buckets restated from the same inequalities (make_buckets,
pick_shape64, twin_shape / comb_ok, long_shape, score_sub_len, bucket_fast_ok), and seeded (reference, queries, ranges) with planted
hits at the places where a twin tile or a strip-mined tile goes wrong.  No GPU is needed here: everything is a pure function of its
arguments, and the expected values come from the oracle alone."""
import os
import re

import numpy as np

import score_instances as si
from score_instances import F32, U8SAT

CSRC = os.path.join(si.ROOT, "parallel-genomeseq_amd", "csrc")
SCORE_KERNEL_H = os.path.join(CSRC, "sw_score_kernel.h")

R16S = (32,)
R64S = (20, 24, 32)
LISTS = dict(si.LISTS, kR16S=R16S, kR64S=R64S)
K_MAX_ROWS_FAST = 512              # host_common.h kMaxRowsFast
K_PROFILE_LDS_MAX = 120 * 1024     # host_common.h kProfileLdsMax
K_COMB_LDS_MAX = 64 * 1024         # host_score.h kCombLdsMax
K_SEG = 64                         # sw_score_kernel.h kSeg
SEM_OF_CELL = {"i16": "kSemI16", "u8i16": "kSemU8", "f32": "kSemF32", "u8f32": "kSemF32U8", "f16": "kSemF16", "u8f16": "kSemU8H"}


# ---- the instance table, read from the headers -----------------------------------------------------------------------------------
def sems_in_header(path=SCORE_KERNEL_H):
    """{kSemName: value} of sw_score_kernel.h."""
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(kSem\w+)\s*=\s*(\d+)\s*;", f.read())}


def _mask(expr, names, sems):
    """Value of a C mask expression over 0x.., 1u << kSem.., kCells.. and |."""
    total = 0
    for term in expr.split("|"):
        term = term.strip()
        m = re.fullmatch(r"1u\s*<<\s*(kSem\w+)", term)
        if m:
            total |= 1 << sems[m.group(1)]
        elif term in names:
            total |= names[term]
        else:
            total |= int(term.rstrip("u"), 0)
    return total


def instances_in_header(path=si.HOST_SCORE_H):
    """[(R, sem, strips, SL, twin, comb, mk, rowp)] of kScoreShapes in host_score.h, expanded as score_insts() expands it."""
    with open(path) as f:
        text = f.read()
    sems = sems_in_header()
    lists = si.lists_in_header(path)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", text)}
    masks = {}
    for m in re.finditer(r"constexpr\s+unsigned\s+(kCells\w+)\s*=\s*([^;]+);", text):
        masks[m.group(1)] = _mask(m.group(2), masks, sems)
    body = re.search(r"kScoreShapes\[\]\s*=\s*\{(.*?)\n\};", text, re.S).group(1)
    out = []
    rows = re.findall(r"^\s*\{([^{}]*)\}", body, re.M)
    for row in rows:
        f = [v.strip() for v in row.split(",")]
        assert re.fullmatch(r"std::size\((\w+)\)", f[1]).group(1) == f[0], row
        flag = lambda v: {"true": True, "false": False}[v]
        sl = consts[f[3]] if f[3] in consts else int(f[3])
        rowp = flag(f[8]) if len(f) > 8 else False
        mask = _mask(f[7], masks, sems)
        for sem in range(8):
            if mask >> sem & 1:
                out.extend((r, sem, flag(f[2]), sl, flag(f[4]), flag(f[5]), int(f[6]), rowp) for r in lists[f[0]])
    return out, len(rows)


def classify(inst, sems):
    """'a': the two-query one-strip instances of test_gpu_score_instances.py (every cell a batch can get on 8-, 16- and 64-lane tiles
    in one strip, sampled or not);  'b': the prefix tiles (test_gpu_prefix_*);  'c': this module;  None: nobody's."""
    r, sem, strips, sl, twin, comb, mk, rowp = inst
    name = {v: k for k, v in sems.items()}[sem]
    if sl not in (8, 16, 64):
        return "b" if sl == 2 and name == "kSemF16M" and not strips and not twin else None
    if rowp:
        return None
    if strips or twin:
        return "c"
    if name == "kSemF32U8":
        return "c"                                     # the uint8 engine's lone query, one per register
    if mk == 4 and sl == 64 and name == "kSemF32":
        return "c"                                     # (the host samples float32 BATCHES on 8- and 16-lane tiles only: a lone query's)
    if mk == 4 and name in ("kSemF16M", "kSemF16MF") and si.DEFAULT.match * (sl * r + 1) > 1024:
        return "c"                                     # (sampled mirrored tiles beyond mirror_ok's bound at 3 / -3 / 2, the one scoring the
    return "a"                                         # other module samples at: 16 x 24 and 16 x 32, reached at 1 / -1 / 4)


# (d) compiled, but no call can launch it: (instance predicate, the line of the host that keeps it out).  Empty today: every row of
# kScoreShapes has a route (test_every_compiled_instance_has_an_owner fails on a row without one).
UNREACHABLE = []


# ---- the host's choice, restated ---------------------------------------------------------------------------------------------------
def lane_stride(r):
    rp = (r + 3) // 4 * 4
    return rp + 4 if rp % 8 == 0 else rp


def profile_lds_bytes(ncodes, r, sl=16, twin=False, comb=False):
    if comb:
        return ncodes * ncodes * max(16, sl) * lane_stride(r) * 4
    return ncodes * max(16, sl) * lane_stride(r // 2 if twin else r) * 4


def wide_ok(ncodes, opts):
    return profile_lds_bytes(ncodes, 32, 64) <= K_PROFILE_LDS_MAX and "no_wide" not in opts


def pick_shape64(length, strip_r=0):
    """(R, strips) of host_score.h pick_shape64."""
    if length <= 2048:
        return next(r for r in si.R64 if 64 * r >= length), False
    if strip_r in R64S:
        return strip_r, True
    best, pick = -1, 0
    for r in R64S:
        rows = -(-length // (64 * r)) * 64 * r
        if best < 0 or rows <= best:
            best, pick = rows, r
    return pick, True


def long_shape(length, long_r=0):
    """R of host_score.h long_shape where every layout fits LDS (small alphabets, a few strips): the fewest padded rows, ties to the
    lower R."""
    best, pick = -1, 0
    for r in (20, 24, 32):
        if long_r in (20, 24, 32) and r != long_r:
            continue
        rows = -(-length // (64 * r)) * 64 * r
        if best < 0 or rows < best:
            best, pick = rows, r
    return pick


def bucket_shape(length, ncodes, opts, slot=0, strip_r=0):
    """(SL, R, strips) of a query of `length` rows: the first loop of make_buckets."""
    if length <= K_MAX_ROWS_FAST:
        return si.pick_shape(length, slot) + (False,)
    if wide_ok(ncodes, opts):
        r, strips = pick_shape64(length, strip_r)
        return 64, r, strips
    return 16, R16S[0], True


def predicted_bucket(count, maxlen, sem, sc, options, ncodes, n, slot=0, strip_r=0, allow_sample=False, long_r=0):
    """The launch make_buckets gives a bucket of `count` queries, the longest of `maxlen` rows, over ranges of up to n columns:
    dict(cell, SL, R, strips, twin, comb, mirror, idiag, unsat, sampled), or dict(long=1, R, unsat, sampled) for sw_long_kernel."""
    opts = set(options)
    sl, r, strips = bucket_shape(maxlen, ncodes, opts, slot, strip_r)
    smax = sc.smax(sem)
    gap = min(255, int(sc.gap)) if sem == U8SAT else int(sc.gap)
    out = dict(cell=None, SL=sl, R=r, strips=int(strips), twin=0, comb=0, mirror=0, idiag=0, unsat=0, sampled=0)
    twin_ok = count == 1 and sl == 64 and "no_twin" not in opts
    twin16_ok = count == 1 and 1 <= maxlen <= K_MAX_ROWS_FAST and "no_twin" not in opts
    htab = sc.f16_table() if sem == F32 else True
    longp = False

    def twin_shape():
        out.update(SL=16, R=next(v for v in si.R16 if v >= -(-maxlen // 16)))
        out["comb"] = int("no_comb" not in opts and profile_lds_bytes(ncodes, out["R"], 16, True, True) <= K_COMB_LDS_MAX)

    if sem == U8SAT:
        twin = twin_ok
        cell = "u8f32" if count == 1 and not twin else "u8i16"
        if cell == "u8i16" and "no_f16" not in opts:
            cell = "u8f16"
        unsat = False
        if "no_unsat" not in opts and "no_f16" not in opts and gap <= 2040:
            if count >= 2:
                cell, unsat, twin = "f16", True, False
                bound = smax * maxlen + smax
                out["mirror"] = int("no_f16_mirror" not in opts and not strips and sl in (8, 16) and bound <= 1024)
            elif twin16_ok and not strips and sl != 64:
                cell, unsat, twin = "f16", True, True
                twin_shape()
            elif count == 1 and sl == 64 and smax * maxlen < 1.6e7 and "u8_long_twin" not in opts:
                cell, unsat, twin = "f32", True, False
                longp = strips and "no_long" not in opts
            elif twin_ok:
                cell, unsat, twin = "f16", True, True
        out.update(cell=cell, twin=int(twin), unsat=int(unsat))
    else:
        fits = "force_f32" not in opts and smax * min(maxlen, max(n, 1)) + smax <= 32000
        cell, twin = ("i16" if fits else "f32"), False
        small = smax * maxlen + smax <= 2040 and "no_f16" not in opts
        if fits and htab and not strips and count >= 2 and small:
            cell = "f16"
            out["mirror"] = int("no_f16_mirror" not in opts and sl in (8, 16) and smax * maxlen + smax <= 1024 and 0 <= gap <= 2040)
        if count == 1 and cell == "i16":
            if twin16_ok and htab and not strips and sl != 64 and small:
                cell, twin = "f16", True
                twin_shape()
            elif twin_ok and "long_twin" in opts:
                twin = True
            elif smax * maxlen < 1.6e7:
                cell = "f32"
            elif twin_ok:
                twin = True
        longp = cell == "f32" and count == 1 and out["SL"] == 64 and strips and not twin and htab and "no_long" not in opts
        lone_sampled = cell == "f32" and count == 1 and out["SL"] == 64 and not twin and allow_sample and "no_sample" not in opts and \
            (out["R"] in R64S if strips else out["R"] in si.R16M)
        out.update(cell=cell, twin=int(twin), sampled=int(lone_sampled))
    if out["mirror"]:
        out["idiag"] = int("no_f16m_int_diag" not in opts)
    if longp:
        return dict(long=1, R=long_shape(maxlen, long_r), unsat=out["unsat"], sampled=int(allow_sample and sem == F32 and "no_sample" not in opts))
    return out


def predicted_lone(length, sem, sc, options, ncodes, n, slot=0, strip_r=0, allow_sample=False):
    return predicted_bucket(1, length, sem, sc, options, ncodes, n, slot, strip_r, allow_sample)


def predicted_strips(count, maxlen, sem, sc, options, ncodes, n, strip_r=0):
    out = predicted_bucket(count, maxlen, sem, sc, options, ncodes, n, 0, strip_r)
    assert out.get("long") or out["strips"] == 1, out
    return out


def fast_ok(maxlen, sem, sc, out, ncodes, n):
    """bucket_fast_ok for integer scorings (the warm-up margin of the scorings used here is far below its bound)."""
    if not out.get("long") and profile_lds_bytes(ncodes, out["R"], out["SL"]) > K_PROFILE_LDS_MAX:
        return False
    if sem == U8SAT and n <= maxlen + 1:
        return False
    if not out.get("long") and out["strips"] and n < 4096:
        return False
    return n >= 1024


def strip_min_cols(sem, maxlen):
    """The shortest range a strip-mined bucket is swept over: the gate of bucket_fast_ok, 4096 columns; the uint8 engine also wants the
    reference to be the longer side by more than one column."""
    return 4096 if sem == F32 or maxlen + 1 < 4096 else maxlen + 2


def score_sub_len(sem, count, maxlen, out):
    if sem == F32 and count == 1 and not out["strips"] and out["SL"] != 64:
        return K_SEG
    s = si.pow2_at_least(maxlen)
    if sem == U8SAT:
        while s <= maxlen + 64:
            s *= 2
    return s


def sub_len_of(sem, count, maxlen, out, chunk_len):
    """score_launch: the sub-chunk length once the tile length is known."""
    s = score_sub_len(sem, count, maxlen, out)
    if sem == F32 and out["strips"] and chunk_len % (64 * K_SEG) == 0:
        s = chunk_len // 64
    if out["strips"]:
        while chunk_len // s > 64:
            s *= 2
    if s > chunk_len or chunk_len % s:
        s = chunk_len
    return s


TAG_FIELDS = ("cell", "SL", "R", "strips", "twin", "comb", "mirror", "idiag", "unsat")


def tag_key(d):
    if d.get("long"):
        return ("long", 64, int(d["R"]), 1, 0, 0, 0, 0, int(d.get("unsat", 0)))
    return (d["cell"],) + tuple(int(d.get(f, 0)) for f in TAG_FIELDS[1:])


def tag_name(key):
    return "%s[SL=%d,R=%d,strips=%d,twin=%d,comb=%d,mirror=%d,idiag=%d,unsat=%d]" % key


def parse_long(path):
    """The long[...] tags of Context.last_path() as dicts."""
    out = []
    for tag in path:
        m = re.fullmatch(r"long\[(.*)\]", tag)
        if m:
            d = {k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split(","))}
            d["long"] = 1
            out.append(d)
    return out


def instance_of(key, sampled, sems):
    """(R, sem, strips, SL, twin, comb, mk, rowp) of kScoreInsts that a score[...] tag names."""
    cell, sl, r, strips, twin, comb, mirror, idiag, unsat = key
    name = SEM_OF_CELL[cell]
    if mirror:
        name = "kSemF16M" if idiag else "kSemF16MF"
    return (r, sems[name], bool(strips), sl, bool(twin), bool(comb), 4 if sampled else 1, False)


# ---- routes --------------------------------------------------------------------------------------------------------------------------
def lone_lengths(shape):
    """(the longest and the shortest query length that pick_bucket gives `shape`, slot)."""
    lens, slot = si.shape_lengths(shape)
    return lens[-1], lens[0], slot


def strip_lengths(sl, r):
    """Query lengths of a strip-mined batch on (sl, r): (two strips; three strips, ONE row in the last; three full strips)."""
    rows = sl * r
    if sl == 16:
        return (513, 1025, 1100)
    return (max(2049, rows + 1), 2 * rows + 1, 3 * rows)


def natural_strip_length(r):
    """The shortest lone query beyond 2048 rows that pick_shape64 sweeps on R rows per lane by its length alone."""
    return next(n for n in range(2049, 6200) if pick_shape64(n) == (r, True))


LONE_SHORT = [(F32, "twin_comb", ()), (F32, "twin", ("no_comb",)), (F32, "f32", ("no_twin",)),
              (U8SAT, "unsat_twin", ()), (U8SAT, "u8f32", ("no_unsat",))]
SHORT_SHAPES = [s for s in si.SHAPES if s[0] != 64]


def lone_sc(sem, L):
    return si.DEFAULT if sem == F32 or L <= 64 else si.U8_LOW_BACKGROUND


LONE_WIDE = [(F32, "f32", (), "f32", 0, 0), (F32, "i16_twin", ("long_twin",), "i16", 1, 0),
             (U8SAT, "f32_unsat", (), "f32", 0, 1), (U8SAT, "f16_twin_unsat", ("u8_long_twin",), "f16", 1, 1),
             (U8SAT, "u8f16_twin", ("no_unsat",), "u8f16", 1, 0), (U8SAT, "u8i16_twin", ("no_unsat", "no_f16"), "u8i16", 1, 0),
             (U8SAT, "u8f32", ("no_unsat", "no_twin"), "u8f32", 0, 0)]


def wide_sc(sem):
    return si.GAP_ABOVE_MATCH if sem == F32 else si.U8_LOW_BACKGROUND


def forced(sl, r, lens):
    """0 where the lengths alone select R; else the value of option strip_r."""
    return 0 if sl == 16 or all(pick_shape64(m) == (r, True) for m in lens) else r


BATCH_STRIPS = [(F32, "i16", (), "i16", 0), (F32, "f32", ("force_f32",), "f32", 0),
                (U8SAT, "f16_unsat", (), "f16", 1), (U8SAT, "u8f16", ("no_unsat",), "u8f16", 0), (U8SAT, "u8i16", ("no_unsat", "no_f16"), "u8i16", 0)]


def strip_sc(sem, alpha=b"ACGT"):
    base = si.GAP_ABOVE_MATCH if sem == F32 else si.U8_LOW_BACKGROUND
    return si.Scoring(base.name + ("/aa20" if alpha != b"ACGT" else ""), base.match, base.mismatch, base.gap, alpha=alpha)


LONE_STRIPS = [(F32, "f32", ("no_long",), "f32", 0, 0), (F32, "i16_twin", ("no_long", "long_twin"), "i16", 1, 0),
               (U8SAT, "f32_unsat", ("no_long",), "f32", 0, 1), (U8SAT, "f16_twin_unsat", ("u8_long_twin",), "f16", 1, 1),
               (U8SAT, "u8f16_twin", ("no_unsat",), "u8f16", 1, 0), (U8SAT, "u8i16_twin", ("no_unsat", "no_f16"), "u8i16", 1, 0),
               (U8SAT, "u8f32", ("no_unsat", "no_twin"), "u8f32", 0, 0)]


def ncodes(sc):
    return len(sc.alpha) + 1


def route_ids(table):
    return ["%s-%s" % ("u8" if v[0] == U8SAT else "f32", v[1]) for v in table]


# Every run of the GPU module, as data: the GPU tests iterate these, and plan() predicts their launches without a GPU.
def lone_short_runs(sem, name, options):
    """dict(L, sc, slot, chunk_opt, one_letter, one_tile, check_inputs, expect) of test_lone_short: every shape at its longest query,
    two lengths that are no multiple of a tile's rows, the one-letter query, one tile per range, and (float engine) two more scorings."""
    twin = "twin" in name
    cell = {"twin_comb": "f16", "twin": "f16", "f32": "f32", "unsat_twin": "f16", "u8f32": "u8f32"}[name]
    comb = int(name in ("twin_comb", "unsat_twin"))
    for shape in ([(16, r) for r in si.R16] if twin else SHORT_SHAPES):
        L, _, slot = lone_lengths(shape)
        if twin:
            L, slot = 16 * shape[1], 0
        yield dict(L=L, sc=lone_sc(sem, L), slot=slot, expect=dict(cell=cell, SL=shape[0], R=shape[1], twin=int(twin), comb=comb, strips=0,
                                                                  unsat=int(name == "unsat_twin")))
    expect = dict(cell=cell, twin=int(twin), comb=comb)
    for L in (150, 16 * 9 + 1):
        yield dict(L=L, sc=lone_sc(sem, L), expect=expect)
    yield dict(L=160, sc=lone_sc(sem, 160), one_letter=True, expect=expect)
    yield dict(L=160, sc=lone_sc(sem, 160), chunk_opt=2048, one_tile=True, expect=expect)
    if sem == F32:
        for sc in (si.GAP_ABOVE_MATCH, si.MISMATCH_ZERO):
            yield dict(L=320, sc=sc, check_inputs=False, expect=expect)


def lone_wide_runs(sem, name, options, cell, twin, unsat):
    """... of test_lone_wide: every kR64 shape at its longest query (the first also at 513 rows), 3 / -3 / 2, one letter, one tile."""
    for r in si.R64:
        for L in ((513, 64 * r) if r == si.R64[0] else (64 * r,)):
            yield dict(L=L, sc=wide_sc(sem), expect=dict(cell=cell, SL=64, R=r, strips=0, twin=twin, comb=0, unsat=unsat))
    expect = dict(cell=cell, SL=64, twin=twin, unsat=unsat)
    yield dict(L=700, sc=si.DEFAULT if sem == F32 else si.U8_LOW_BACKGROUND, check_inputs=sem == F32, expect=expect)
    yield dict(L=640, sc=wide_sc(sem), one_letter=True, expect=expect)
    yield dict(L=640, sc=wide_sc(sem), chunk_opt=2048, one_tile=True, expect=expect)


def batch_strip_runs(sem, name, options, cell, unsat):
    """dict(shape, lens, sc, strip_r, chunk_opt, check_inputs, expect) of test_batch_strips."""
    expect = dict(cell=cell, twin=0, unsat=unsat, mirror=0, strips=1)
    for r in R64S:
        lens = strip_lengths(64, r)
        yield dict(shape=(64, r), lens=lens, sc=strip_sc(sem), strip_r=forced(64, r, lens), expect=expect)
    yield dict(shape=(16, 32), lens=strip_lengths(16, 32), sc=strip_sc(sem, si.AA20), expect=expect)
    # tiles of more sub-chunks than one, through the aid `chunk` (the uint8 engine's sub-chunk is a power of two beyond |x| + 64; the float
    # engine's is 1/64 of a tile of a multiple of 4096 columns)
    yield dict(shape=(16, 32), lens=strip_lengths(16, 32), sc=strip_sc(sem, si.AA20), chunk_opt=4096, min_subs=64 if sem == F32 else 2, expect=expect)
    if sem == U8SAT:
        yield dict(shape=(64, 20), lens=strip_lengths(64, 20), sc=strip_sc(sem), strip_r=20, chunk_opt=8192, min_subs=2, expect=expect)
    if sem == F32:                       # 3 / -3 / 2 (its background hides the short planted copies): three tiles through the aid `chunk`
        yield dict(shape=(64, 20), lens=strip_lengths(64, 20), sc=si.DEFAULT, strip_r=20, chunk_opt=4096, check_inputs=False, expect=expect)
        yield dict(shape=(16, 32), lens=strip_lengths(16, 32), sc=si.Scoring("3/-3/2/aa20", alpha=si.AA20), check_inputs=False, expect=expect)


def lone_strip_runs(sem, name, options, cell, twin, unsat):
    """... of test_lone_strips; `options` of a run replaces the variant's."""
    expect = dict(cell=cell, twin=twin, unsat=unsat, strips=1)
    for r in R64S:
        yield dict(shape=(64, r), lens=(natural_strip_length(r),), sc=strip_sc(sem), expect=expect)
    for m in (2 * 1280 + 1, 2 * 1280 + 200):                           # three strips (the last of ONE row, and of 200): R through strip_r
        yield dict(shape=(64, 20), lens=(m,), sc=strip_sc(sem), strip_r=20, expect=expect)
    if sem == F32:                                                      # 3 / -3 / 2: the widest warm-up margin, with and without twin tiles
        yield dict(shape=(64, 20), lens=(2049,), sc=si.DEFAULT, chunk_opt=4096, check_inputs=False, min_subs=64, expect=expect)
        yield dict(shape=(64, 20), lens=(2 * 1280 + 200,), sc=si.DEFAULT, strip_r=20, check_inputs=False, expect=expect)
    if sem == U8SAT:                                                    # (its sub-chunk is a power of two beyond |x| + 64: two per tile)
        yield dict(shape=(64, 20), lens=(2049,), sc=strip_sc(sem), chunk_opt=8192, min_subs=2, expect=expect)
    if name in ("f32", "u8f32"):                                       # a 20-letter alphabet: the kR16S shape (the uint8 engine: no option)
        for m in (513, 1025, 1100):
            yield dict(shape=(16, 32), lens=(m,), sc=strip_sc(sem, si.AA20), options=() if name == "u8f32" else options,
                       expect=dict(cell=cell, SL=16, R=32, twin=0, unsat=0, strips=1), **(dict(chunk_opt=4096, min_subs=2) if m == 1100 else {}))


LONG_VARIANTS = [(F32, (), (), 1, 0), (F32, ("no_long_p32",), (), 0, 0), (F32, (), (("long_groups", 2),), 1, 1), (U8SAT, (), (), 1, 0)]


def long_runs(sem, options, ints):
    """(R, rows, int options, scoring, check_inputs) of test_long_kernel: R by length, and (float engine, plain) by long_r on the shortest
    query; the float engine also at 3 / -3 / 2, whose warm-up margin is two and a half query lengths (its background hides the short
    planted copies: every value is compared all the same)."""
    for r in (20, 24, 32):
        yield r, natural_strip_length(r), ints, strip_sc(sem), True
        if sem == F32:
            yield r, natural_strip_length(r), ints, si.DEFAULT, False
        if r != 20 and sem == F32 and not ints and not options:
            yield r, 2049, ints + (("long_r", r),), strip_sc(sem), True


SAMPLED = [("wide", ()), ("strips", ("no_long",)), ("long", ())]


def sampled_runs(name):
    """(kind of case, shape or rows, expect) of test_sampled_lone."""
    if name == "wide":
        for r in si.R16M:
            yield "lone", 64 * r, dict(cell="f32", SL=64, R=r, strips=0, twin=0, sampled=1)
    else:
        for r in R64S:
            yield "strip", r, (dict(cell="f32", SL=64, R=r, strips=1, twin=0, sampled=1) if name == "strips" else dict(long=1, R=r, sampled=1))


SAMPLED_MIRROR = [("f16m", ()), ("f16mf", ("no_f16m_int_diag",))]
SAMPLED_MIRROR_SHAPES = [(16, 24), (16, 32)]


def sampled_mirror_want(shape, options):
    """The sampled launch of a batch on a 16-lane shape of more than 340 rows at 1 / -1 / 4 (within mirror_ok's bound there)."""
    return dict(si.predicted(shape, shape[0] * shape[1], F32, si.GAP_ABOVE_MATCH, options), strips=0, twin=0, comb=0, sampled=1)


def matches(want, expect):
    return all(want.get(k) == v for k, v in expect.items())


def plan():
    """{instance of kScoreInsts: [runs]} of every score_ranges and align run above, predicted on the host's inequalities alone."""
    sems = sems_in_header()
    out = {}

    def add(want, run, what, sampled=0):
        assert matches(want, run if isinstance(run, dict) and "cell" in run else run.get("expect", {})), (what, want, run)
        if not want.get("long"):
            out.setdefault(instance_of(tag_key(want), sampled, sems), []).append(what)

    for sem, name, options in LONE_SHORT:
        for run in lone_short_runs(sem, name, options):
            add(predicted_lone(run["L"], sem, run["sc"], options, ncodes(run["sc"]), 1024, run.get("slot", 0)), run, "lone_short " + name)
    for v in LONE_WIDE:
        for run in lone_wide_runs(*v):
            add(predicted_lone(run["L"], v[0], run["sc"], v[2], ncodes(run["sc"]), 1024), run, "lone_wide " + v[1])
    for v in BATCH_STRIPS:
        for run in batch_strip_runs(*v):
            add(predicted_bucket(len(run["lens"]), max(run["lens"]), v[0], run["sc"], v[2], ncodes(run["sc"]), strip_min_cols(v[0], max(run["lens"])), 0, run.get("strip_r", 0)),
                run, "batch_strips " + v[1])
    for v in LONE_STRIPS:
        for run in lone_strip_runs(*v):
            add(predicted_bucket(1, run["lens"][0], v[0], run["sc"], run.get("options", v[2]), ncodes(run["sc"]), 4096, 0, run.get("strip_r", 0)),
                run, "lone_strips " + v[1])
    add(predicted_bucket(3, 1100, F32, strip_sc(F32), ("no_wide",), 5, 4096), dict(expect=dict(cell="i16", SL=16, R=32, strips=1)), "no_wide")
    for name, options in SAMPLED:
        for kind, v, expect in sampled_runs(name):
            rows = v if kind == "lone" else natural_strip_length(v)
            add(predicted_lone(rows, F32, si.GAP_ABOVE_MATCH, options, 5, 20000, allow_sample=True), dict(expect=expect), "sampled " + name, 1)
    for name, options in SAMPLED_MIRROR:
        for shape in SAMPLED_MIRROR_SHAPES:
            want = sampled_mirror_want(shape, options)
            add(want, dict(expect=dict(cell="f16", mirror=1, idiag=int(name == "f16m"))), "sampled mirrored " + name, 1)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _odd(x):
    return x + (x % 4 == 0)


class LoneCase:
    """One lone query of L rows against a reference cut into ranges relative to the tile length CL.  T = tiles one workgroup holds
    (256 / SL, twice that on twin tiles); tiles 2k and 2k + 1 of a range share a register on twin tiles.  All ranges >= 1024 columns.
      A   starts at column 2; a multiple of CL and ONE column: an even number of tiles, the last of one column; the first two thirds
          of the query (uint8 engine: at most 200 units' worth, below the cap) end in its last column.
      B   adjacent to A (start = 3 mod CL), a multiple of CL, an even number of tiles: the whole query ends in an ODD tile, on the last
          column of a 64-column sub-chunk; its first two thirds, a lesser hit, end in front of it in an EVEN tile.
      C   the reverse: the whole query STARTS on the first column of a sub-chunk and ends in an EVEN tile; the lesser hit ends in front
          of it in an ODD tile.
      D   overlaps C by 2 L columns (make_string_range); holds no hit of its own.
      O   an ODD number of tiles; the whole query ends seven columns before the range's end, in the last tile (no second half).
      P   the whole query centred on a boundary between tiles 2 j | 2 j + 1 (the two halves of one register).
      Q   ... between tiles 2 j + 1 | 2 j + 2 (two registers of one workgroup).
      F   more than 2 T tiles: the whole query centred on the boundary between tiles j T - 1 | j T: two workgroups.
      G   ends at the reference's last column; a run of one letter for the one-letter query.
    one_tile=True: every range is ONE tile (cpr == 1: no warm-up)."""
    NAMES = ("A", "B", "C", "D", "O", "P", "Q", "F", "G")

    def __init__(self, pgs, L, sem, sc, CL, per_wg, one_letter=False, one_tile=False, seed=0):
        self.L, self.sem, self.sc, self.chunk, self.per_wg, self.one_tile = L, sem, sc, CL, per_wg, one_tile
        base = 7000003 * L + 104729 * seed + (31 if sem == U8SAT else 0) + (5 if one_letter else 0)
        q = si.letters(pgs, base + 1, L, sc.alpha).copy()
        if one_letter:
            q[:] = sc.alpha[0]
        part = -(-2 * L // 3)
        if sem == U8SAT and sc.match * part >= 255:
            part = int(200 // sc.match)                                  # (a lesser hit the cap of 255 does not hide)
        if one_tile:
            W = CL
            assert CL >= 1024 and CL > L + 1
            starts = [2]
            for _ in range(3):
                starts.append(_odd(starts[-1] + W + 13))
            n = starts[-1] + W
            self.ranges = [(s, s + W) for s in starts[:3]] + [(n - W, n)]
            self.names = ("A", "B", "C", "G")
            ref = si.letters(pgs, base + 2, n, sc.alpha).copy()
            self.plants = [("whole in A from its first column", 0, 2, L), ("two thirds at B's end", 1, self.ranges[1][1] - part, part),
                           ("whole at G's end", 3, n - L, L)]
        else:
            up = lambda cols: -(-cols // CL)                            # tiles that hold `cols` columns
            even = lambda t: t + t % 2
            k = max(1, -(-max(1100, L + 100) // (4 * CL)))             # every range below is at least 4 k tiles >= 1024 columns
            half = L // 2 + 8
            A = (2, 2 + (4 * k + 1) * CL + 1)
            tb0 = even(up(part + 8))                                     # B: the lesser hit ends in the middle of EVEN tile tb0 ...
            tb = even(tb0 + 1 + up(L + 8)) + 1                          # ... and the whole copy, behind it, in ODD tile tb
            B = (A[1], A[1] + max(4 * k, tb + 1) * CL)
            c0 = _odd(B[1] + 37)
            to = even(up(part + 8)) + 1                                  # C, the reverse: the lesser hit ends in ODD tile to ...
            te = even(to + 1 + up(L + 64))                               # ... and the whole copy in EVEN tile te
            C = (c0, c0 + max(4 * k, even(te + 1 + up(2 * L))) * CL + L)
            D = (C[1] - 2 * L, C[1] - 2 * L + 4 * k * CL + L)
            o0 = _odd(D[1] + 11)
            O = (o0, o0 + (4 * k + 1) * CL - 7)
            p0 = _odd(O[1] + 5)
            tp = even(up(half)) + 1                                      # P: the boundary between tiles tp - 1 | tp, tp odd: one register
            P = (p0, p0 + max(4 * k, tp + up(half)) * CL + 9)
            q0 = _odd(P[1] + 21)
            tq = even(up(half) + 1)                                      # Q: tq even: two registers
            Q = (q0, q0 + max(4 * k, tq + up(half)) * CL + CL // 2)
            f0 = _odd(Q[1] + 3)
            tf = per_wg * up(-(-half // per_wg))                         # F: a multiple of T: two workgroups
            F = (f0, f0 + max(4 * k, 2 * per_wg + 3, tf + up(half) + 1) * CL - 5)
            g0 = _odd(F[1] + 23)
            n = g0 + 4 * k * CL + 9
            G = (g0, n)
            self.ranges = [A, B, C, D, O, P, Q, F, G]
            self.names = self.NAMES
            ref = si.letters(pgs, base + 2, n, sc.alpha).copy()
            b_end = B[0] + (tb * CL + CL // 2) // 64 * 64               # one past the last column of a 64-column sub-chunk of B
            c_at = C[0] + -(-(te * CL + CL // 4 - L) // 64) * 64         # the first column of a sub-chunk of C
            b_part, c_part = B[0] + tb0 * CL + CL // 2 - part, C[0] + to * CL + CL // 2 - part
            self.cuts = dict(tb0=tb0, tb=tb, to=to, te=te, tp=tp, tq=tq, tf=tf, b_end=b_end, c_at=c_at, b_part=b_part, c_part=c_part)
            self.plants = [("whole, ends in odd tile tb of B on a sub-chunk's last column", 1, b_end - L, L),
                           ("first two thirds, ends in even tile tb0 of B", 1, b_part, part),
                           ("first two thirds, ends in odd tile to of C", 2, c_part, part),
                           ("whole, starts on a sub-chunk's first column of C, ends in even tile te", 2, c_at, L),
                           ("whole, ends in O's last tile", 4, O[1] - 7 - L, L),
                           ("whole across tiles tp - 1 | tp of P", 5, P[0] + tp * CL - L // 2, L),
                           ("whole across tiles tq - 1 | tq of Q", 6, Q[0] + tq * CL - L // 2, L),
                           ("whole across tiles tf - 1 | tf of F", 7, F[0] + tf * CL - L // 2, L),
                           ("two thirds at A's end", 0, A[1] - part, part)]
            if one_letter:
                self.plants = [("run in G", 8, G[0] + 50, L)]
            for what, r, at, ln in self.plants:
                assert self.ranges[r][0] <= at and at + ln <= self.ranges[r][1], (what, self.ranges[r], at, ln)
            assert b_part >= B[0] and b_end - L >= b_part + part + 8 and c_part >= C[0] and c_at >= c_part + part + 8 and c_at + L <= C[1] - 2 * L, (self.cuts, B, C)
            assert (b_end - 1 - B[0]) // CL == tb and (c_at + L - 1 - C[0]) // CL == te and (b_end - B[0]) % 64 == 0 and (c_at - C[0]) % 64 == 0
            assert (b_part + part - 1 - B[0]) // CL == tb0 and (c_part + part - 1 - C[0]) // CL == to
        for what, r, at, ln in self.plants:
            ref[at:at + ln] = q[:ln]                                     # (always the first ln rows)
        self.ref = ref.tobytes()
        self.queries = [q.tobytes()]
        assert all(r[1] - r[0] >= 1024 and r[1] - r[0] > L + 1 and 0 <= r[0] and r[1] <= len(self.ref) for r in self.ranges), self.ranges
        self.expected = None

    def key(self):
        return ("lone", self.L, self.sem, self.sc.name, self.chunk, self.per_wg, self.one_tile, len(set(self.queries[0])) == 1)

    def tiles(self, r):
        return -(-(self.ranges[r][1] - self.ranges[r][0]) // self.chunk)

    def compute(self, oracle, pool):
        if self.expected is None:
            kw = self.sc.kw()
            vals = list(pool.map(lambda rg: oracle.score_only(self.queries[0], self.ref[rg[0]:rg[1]], self.sem, **kw), self.ranges))
            self.expected = np.array(vals, dtype=np.float64).reshape(len(self.ranges), 1)
            own = float(self.sc.match) * self.L if self.sc.lut is None else float(sum(self.sc.lut[c, c] for c in self.queries[0]))
            self.perfect = min(255.0, own) if self.sem == U8SAT else own
        return self.expected

    def input_faults(self):
        """What the inputs must hold, from the oracle's values alone."""
        e, p = self.expected[:, 0], self.perfect
        rn = {n: i for i, n in enumerate(self.names)}
        out = []
        if len(set(self.queries[0])) == 1:
            if e[rn["G"]] < p:
                out.append("the run in G scores %g, perfect %g" % (e[rn["G"]], p))
            return out
        whole = ("A", "G") if self.one_tile else ("B", "C", "O", "P", "Q", "F")
        for n in whole:
            if e[rn[n]] < p:
                out.append("range %s: %g, below the perfect score %g" % (n, e[rn[n]], p))
        if self.sem == F32 or p < 255:
            part = "B" if self.one_tile else "A"
            if not 0.4 * p < e[rn[part]] < p:
                out.append("range %s: the two-thirds copy scores %g (perfect %g)" % (part, e[rn[part]], p))
            if not self.one_tile and not e[rn["D"]] < 0.5 * p and self.L >= 64:
                out.append("range D: %g is not background (perfect %g)" % (e[rn["D"]], p))
        return out

    def geometry_faults(self):
        """The cuts are where the class says they are."""
        if self.one_tile:
            return [] if all(self.tiles(r) == 1 for r in range(len(self.ranges))) else ["a range of more than one tile"]
        CL = self.chunk
        rn = {n: i for i, n in enumerate(self.names)}
        A, B, C, D, O, P, Q, F, G = self.ranges
        out = []
        if not ((A[1] - A[0]) % CL == 1 and self.tiles(rn["A"]) % 2 == 0 and A[0] == 2):
            out.append("A")
        if not (B[0] == A[1] and (B[1] - B[0]) % CL == 0 and self.tiles(rn["B"]) % 2 == 0):
            out.append("B")
        if C[1] - D[0] != 2 * self.L:
            out.append("C | D overlap")
        if self.tiles(rn["O"]) % 2 != 1:
            out.append("O has an even number of tiles")
        if self.tiles(rn["F"]) <= 2 * self.per_wg:
            out.append("F fits two workgroups' tiles")
        if G[1] != len(self.ref):
            out.append("G")
        if any(r[0] % 4 == 0 for r in (A, B, C, O, P, Q, F, G)):
            out.append("a start on a multiple of 4")
        return out


class StripCase:
    """A strip-mined batch on (SL, R) — rows = SL R per strip — against ranges of >= 4096 columns cut relative to the tile length CL.
    Queries in upload order (sorted by length the pairs are (0, 1) and (2, alone): the halves of the first register differ in strip
    count, the last workgroup has no second query):
      0  two strips                       1  three strips, ONE row in the last                2  three full strips, the bucket's longest
    or the one query of the single length given.  Ranges:
      A  starts at column 2, exactly 4096 columns, the gate (uint8 engine, queries of 4095 rows and more: two columns more than the query)
      B  adjacent; three tiles, two whole ones and a part (more where that is below A's length)
      C  as long as A: one tile where CL allows             G  ends at the reference's last column
    Planted (flank = 100 rows either side of a strip boundary row, cut = 10):
      in B  query 2 whole, across the boundary between tiles 0 | 1 (every strip boundary, and the boundary row's warm-up part)
      in A  the LAST rows / 2 rows of query 2 (the path lives in the last strip), and the FIRST rows / 2 rows of query 0
            and the last flank + 1 rows of query 1, whose last row is its one-row strip's
      in C  queries 1 and 2 with `cut` rows deleted across strip boundary rows `rows` and 2 rows (a gap carried through the boundary row)
      in G  queries 1 and 0 with `cut` reference letters inserted at strip boundary row `rows`; the last 200 rows of query 2 in the
            reference's last 200 columns, G's best hit: it ends in G's second tile of 77 columns where CL is A's length — on twin tiles
            the high half of the last register
    A lone query (a range shows ONE value per query) has the deletion across its LAST strip boundary row; in G its best hit is the
    200-row tail, which outscores the insertion there.
    """
    NAMES = ("A", "B", "C", "G")
    FLANK, CUT = 100, 10

    def __init__(self, pgs, shape, lens, sem, sc, CL, seed=0):
        sl, r = shape
        rows = sl * r
        self.shape, self.rows, self.sem, self.sc, self.chunk = shape, rows, sem, sc, CL
        base = 9000011 * (sl * 100 + r) + 7919 * seed + sum(lens) + (17 if sem == U8SAT else 0)
        qs = [si.letters(pgs, base + 10 + k, m, sc.alpha).copy() for k, m in enumerate(lens)]
        long_q = len(qs) - 1
        L = len(qs[long_q])
        assert CL % 64 == 0
        W = strip_min_cols(sem, L)                                    # 4096, the gate (the uint8 engine: more than the longest query)
        self.mincols = W
        A = (2, 2 + W)
        B = (A[1], A[1] + 2 * CL + max(CL // 2, W - 2 * CL) + 1)
        c0 = _odd(B[1] + 37)
        C = (c0, c0 + W)
        g0 = _odd(C[1] + 11)
        n = g0 + W + 77
        G = (g0, n)
        self.ranges = [A, B, C, G]
        ref = si.letters(pgs, base + 1, n, sc.alpha).copy()
        f, cut = self.FLANK, self.CUT
        ins = si.letters(pgs, base + 2, 2 * cut, sc.alpha)

        def deleted(x, row):
            return np.concatenate([x[row - f:row - cut // 2], x[row + cut - cut // 2:row + f]])

        def inserted(x, row, extra):
            return np.concatenate([x[row - f:row], extra, x[row:min(len(x), row + f)]])

        self.plants = []
        self.checks = []                                                # (range, query, what, a score the oracle must exceed, and reach)
        m, g = float(sc.match), float(sc.gap)

        def put(what, rg, k, at, piece, above=None, reach=None):
            assert self.ranges[rg][0] <= at and at + len(piece) <= self.ranges[rg][1], (what, rg, at, len(piece), self.ranges[rg])
            ref[at:at + len(piece)] = piece
            self.plants.append((what, rg, at, len(piece)))
            self.checks.append((rg, k, what, above, m * len(piece) if reach is None else reach))

        def gap_at(what, rg, k, at, row, extra=None):
            """Query k around strip boundary row `row` with `cut` rows deleted, or `extra` inserted: worth more than either flank alone."""
            x = qs[k]
            if len(x) < row + f // 2:                                     # (the strip below the boundary has one row: the copy ends in it)
                return put(what + ": the last flank + 1 rows", rg, k, at, x[row - f:], m * f)
            piece = deleted(x, row) if extra is None else inserted(x, row, extra)
            lo, hi = (f - cut // 2, min(len(x), row + f) - row - (cut - cut // 2)) if extra is None else (f, min(len(x), row + f) - row)
            put(what, rg, k, at, piece, m * max(lo, hi), m * (lo + hi) - g * cut)

        if L <= 2 * CL:
            put("whole across tiles 0 | 1", 1, long_q, B[0] + CL - L // 2, qs[long_q])
        else:
            put("whole from B's first column", 1, long_q, B[0], qs[long_q][:B[1] - B[0]])
        put("last rows / 2 rows", 0, long_q, A[0] + 40, qs[long_q][L - rows // 2:])
        if len(qs) > 1:
            put("first rows / 2 rows", 0, 0, A[0] + 40 + rows // 2 + 300, qs[0][:rows // 2])
            put("the last flank + 1 rows (the last is its one-row strip's)", 0, 1, A[0] + 40 + rows + 600, qs[1][2 * rows - f:], m * f)
            gap_at("deletion across strip boundary row `rows`", 2, 1, C[0] + 500, rows)
            gap_at("deletion across strip boundary row 2 rows", 2, 2, C[0] + 500 + 2 * f + 200, 2 * rows)
            gap_at("insertion at strip boundary row `rows`", 3, 1, G[0] + 300, rows, ins[:cut])
            gap_at("insertion at strip boundary row `rows`", 3, 0, G[0] + 300 + 2 * f + 200, rows, ins[cut:])
        else:
            # (one value per range: the deletion lies at the LAST strip boundary row, the insertion at the first)
            gap_at("deletion across the last strip boundary row", 2, 0, C[0] + 500, (L - 1) // rows * rows)
            gap_at("insertion at strip boundary row `rows`", 3, 0, G[0] + 300, rows, ins[:cut])
        tail = 200                                # ends in G's last tile (77 columns, an odd tile, where CL is A's length); G's best hit
        put("the last %d rows, ending in the reference's last column" % tail, 3, long_q, n - tail, qs[long_q][L - tail:])
        self.ref = ref.tobytes()
        self.queries = [v.tobytes() for v in qs]
        assert all(rg[1] - rg[0] >= W and rg[1] <= n for rg in self.ranges) and A[1] - A[0] == W
        self.expected = None

    def key(self):
        return ("strip", self.shape, tuple(len(q) for q in self.queries), self.sem, self.sc.name, self.chunk)

    def tiles(self, r):
        return -(-(self.ranges[r][1] - self.ranges[r][0]) // self.chunk)

    def compute(self, oracle, pool):
        if self.expected is None:
            kw = self.sc.kw()
            jobs = [(r, k) for r in range(len(self.ranges)) for k in range(len(self.queries))]
            vals = list(pool.map(lambda rk: oracle.score_only(self.queries[rk[1]], self.ref[self.ranges[rk[0]][0]:self.ranges[rk[0]][1]],
                                                              self.sem, **kw), jobs))
            self.expected = np.array(vals, dtype=np.float64).reshape(len(self.ranges), len(self.queries))
        return self.expected

    def input_faults(self):
        """From the oracle alone: every planted copy scores what its length gives, and a copy with a gap at a strip boundary row scores
        MORE than its longer flank — its path crosses the boundary row with the gap.  (Only where the background stays below the hits:
        a gap above the match.  A saturated uint8 value cannot tell two hits apart.)"""
        e = self.expected
        cap = (lambda v: min(255.0, v)) if self.sem == U8SAT else (lambda v: v)
        out = []
        for rg, k, what, above, reach in self.checks:
            if e[rg, k] < cap(reach) or (above is not None and cap(reach) < 255 and not e[rg, k] > above):
                out.append("range %s query %d, %s: %g (to exceed %r, to reach %g)" % (self.NAMES[rg], k, what, e[rg, k], above, cap(reach)))
        return out

    def geometry_faults(self):
        out = []
        if self.tiles(1) != 3 and (2 * self.chunk + self.chunk // 2 >= self.mincols or self.tiles(1) < 3):
            out.append("B has %d tiles" % self.tiles(1))
        if self.tiles(2) != 1 and self.chunk >= self.mincols:
            out.append("C has %d tiles" % self.tiles(2))
        if self.ranges[3][1] != len(self.ref):
            out.append("G")
        return out
