"""CPU side of tests/test_gpu_lone_strip_instances.py: the table of compiled sw_score_kernel instances, read from host_score.h, is
partitioned among the modules that pin raw maxima — a row added to kScoreShapes without a case fails here, without a GPU — and the
inputs hold what their classes say, from the oracle alone."""
import re

import lone_strip_instances as ls
import score_instances as si
from score_instances import F32, U8SAT


def _header():
    with open(si.HOST_SCORE_H) as f:
        return f.read()


def test_instance_table_read_from_the_header():
    """The expansion of kScoreShapes has score_inst_count() entries — the sum over its rows of (cells in the mask) x (rows-per-lane
    values in the list), counted here from the text a second way — no entry twice, and the lists this module iterates are the header's."""
    insts, nrows = ls.instances_in_header()
    text = _header()
    body = re.search(r"kScoreShapes\[\]\s*=\s*\{(.*?)\n\};", text, re.S).group(1)
    assert nrows == body.count("std::size(") and nrows >= 16
    lists = si.lists_in_header()
    for name, mine in ls.LISTS.items():
        assert lists.get(name) == mine, "%s: host_score.h has %r, the tests iterate over %r" % (name, lists.get(name), mine)
    per_list = {}
    for inst in insts:
        per_list[inst[2:]] = per_list.get(inst[2:], 0) + 1
    count = 0                                            # score_inst_count(): for every row, for every set bit, g.n
    masks = {"kCellsPlain": 6, "kCellsMirror": 2, "kCellsTwin": 4, "kCellsF16": 1, "kCellsSampled": 2}
    for row in re.findall(r"^\s*\{([^{}]*)\}", body, re.M):
        f = [v.strip() for v in row.split(",")]
        bits = sum(masks[t.strip()] if t.strip() in masks else 1 for t in f[7].split("|"))
        count += bits * len(lists[f[0]])
    assert len(insts) == count == len(set(insts)), (len(insts), count, len(set(insts)))
    sems = ls.sems_in_header()
    assert sorted(sems.values()) == list(range(8)) and set(ls.SEM_OF_CELL.values()) | {"kSemF16M", "kSemF16MF"} == set(sems)
    for name, bits in masks.items():                     # the popcounts above are the header's masks
        m = re.search(r"constexpr\s+unsigned\s+%s\s*=\s*([^;]+);" % name, text).group(1)
        assert bin(ls._mask(m, {}, sems)).count("1") == bits, name


def test_every_compiled_instance_has_an_owner():
    """(a) the two-query one-strip instances of test_gpu_score_instances.py, (b) the prefix tiles of the test_gpu_prefix_* modules,
    (c) a run of test_gpu_lone_strip_instances.py, (d) declared unreachable: every instance is in exactly one."""
    insts, _ = ls.instances_in_header()
    sems = ls.sems_in_header()
    plan = ls.plan()
    text = _header() + open(ls.SCORE_KERNEL_H).read()
    for pred, line in ls.UNREACHABLE:
        assert line in text, "the line that keeps an instance out is no longer in the host's code: %r" % line
    sets = {"a": set(), "b": set(), "c": set(), "d": set()}
    for inst in insts:
        owners = [ls.classify(inst, sems)] if not any(pred(inst) for pred, _ in ls.UNREACHABLE) else ["d"]
        assert owners[0] in sets, "no module pins %r (R, sem, strips, SL, twin, comb, mk, rowp)" % (inst,)
        sets[owners[0]].add(inst)
    assert sum(len(v) for v in sets.values()) == len(insts)
    # (a) is, instance by instance, what the existing module iterates: score_instances.plan() at its scorings, and the loop of
    # test_sampled_instances at 3 / -3 / 2
    import test_gpu_score_instances as two

    def inst(want, sampled):
        key = ls.tag_key(dict(want, strips=0, twin=0, comb=0))
        return ls.instance_of(key, sampled, sems)

    theirs = set()
    for sem, scorings in ((F32, (si.DEFAULT, si.GAP_ABOVE_MATCH, si.MISMATCH_ZERO, si.CHEAP_GAP)), (U8SAT, (si.DEFAULT, si.U8_LOW_BACKGROUND))):
        for sc in scorings:
            theirs |= {inst(want, 0) for _, _, _, want in si.plan(sem, sc)}
    for sem, _, options in two.SAMPLED_VARIANTS:
        for shape in si.SAMPLED_SHAPES:
            want = si.predicted(shape, shape[0] * shape[1], sem, si.DEFAULT, options, allow_sat=True)
            if not (want["cell"] == "f32" and shape[0] == 64):
                theirs.add(inst(want, 1))
    assert sets["a"] == theirs, "set (a) and what test_gpu_score_instances.py runs differ: %r" % sorted(sets["a"] ^ theirs)
    # (b) is the list of prefix heights at its three folds
    assert {(i[0], i[6], i[7]) for i in sets["b"]} == {(r, mk, rowp) for r in si.R8M for mk, rowp in ((4, False), (4, True), (1, True))}
    # (c) is planned, instance by instance; what the plan runs beyond (c) is the lone route onto an instance of (a)
    missing = sorted(sets["c"] - set(plan))
    assert not missing, "compiled, and no run of test_gpu_lone_strip_instances.py reaches: %r" % missing
    beyond = set(plan) - sets["c"]
    assert beyond <= sets["a"] and all(i[1] == sems["kSemF32"] and i[6] == 1 for i in beyond), sorted(beyond - sets["a"])
    # the sampled mirrored tiles that set (a) cannot hold are the two shapes beyond the mirror bound at match 3
    tall = {i for i in sets["c"] if i[6] == 4 and i[1] in (sems["kSemF16M"], sems["kSemF16MF"])}
    assert {(i[3], i[0]) for i in tall} == set(ls.SAMPLED_MIRROR_SHAPES) and len(tall) == 4
    # (d) holds nothing a run can launch
    assert not sets["d"] & set(plan)
    print("\n(a) %d  (b) %d  (c) %d  (d) %d  of %d" % (len(sets["a"]), len(sets["b"]), len(sets["c"]), len(sets["d"]), len(insts)))


def test_routes_of_the_issue():
    """The host's choice for the routes the module is there for, on the restated inequalities."""
    dna, aa = 5, 21
    p = ls.predicted_lone
    assert ls.matches(p(150, F32, si.DEFAULT, (), dna, 1 << 20), dict(cell="f16", SL=16, R=10, twin=1, comb=1))
    assert ls.matches(p(150, F32, si.DEFAULT, ("no_comb",), dna, 1 << 20), dict(cell="f16", twin=1, comb=0))
    assert ls.matches(p(150, F32, si.DEFAULT, ("no_twin",), dna, 1 << 20), dict(cell="f32", SL=8, R=19, twin=0))
    assert ls.matches(p(512, F32, si.DEFAULT, (), dna, 1 << 20), dict(cell="f16", SL=16, R=32, twin=1, comb=1))
    assert ls.matches(p(512, F32, si.DEFAULT, (), 7, 1 << 20), dict(cell="f16", SL=16, R=32, twin=1, comb=0)), "six letters: no room for pairs"
    assert ls.matches(p(700, F32, si.DEFAULT, (), dna, 1 << 20), dict(cell="f16", SL=16, R=32)) is False
    assert ls.matches(p(700, F32, si.DEFAULT, (), dna, 1 << 20), dict(cell="f32", SL=64, R=12, strips=0, twin=0))
    assert ls.matches(p(700, F32, si.DEFAULT, ("long_twin",), dna, 1 << 20), dict(cell="i16", SL=64, R=12, twin=1))
    assert p(2049, F32, si.DEFAULT, (), dna, 1 << 20) == dict(long=1, R=20, unsat=0, sampled=0)
    assert p(2561, F32, si.DEFAULT, (), dna, 1 << 20)["R"] == 24 and p(3841, F32, si.DEFAULT, (), dna, 1 << 20)["R"] == 32
    assert ls.matches(p(2049, F32, si.DEFAULT, ("no_long",), dna, 1 << 20), dict(cell="f32", SL=64, R=20, strips=1, twin=0))
    assert ls.matches(p(2049, F32, si.DEFAULT, ("no_long", "long_twin"), dna, 1 << 20), dict(cell="i16", SL=64, R=20, strips=1, twin=1))
    assert ls.matches(p(600, F32, si.DEFAULT, (), aa, 1 << 20), dict(cell="f32", SL=16, R=32, strips=1, twin=0))
    assert ls.matches(p(600, F32, si.DEFAULT, ("no_wide",), dna, 1 << 20), dict(cell="f32", SL=16, R=32, strips=1))
    assert ls.matches(p(600, U8SAT, si.DEFAULT, (), aa, 1 << 20), dict(cell="u8f32", SL=16, R=32, strips=1, unsat=0))
    assert ls.matches(p(150, U8SAT, si.DEFAULT, (), dna, 1 << 20), dict(cell="f16", SL=16, R=10, twin=1, comb=1, unsat=1))
    assert ls.matches(p(150, U8SAT, si.DEFAULT, ("no_unsat",), dna, 1 << 20), dict(cell="u8f32", SL=8, R=19, twin=0, unsat=0))
    assert ls.matches(p(700, U8SAT, si.DEFAULT, (), dna, 1 << 20), dict(cell="f32", SL=64, R=12, unsat=1, twin=0))
    assert p(2049, U8SAT, si.DEFAULT, (), dna, 1 << 20) == dict(long=1, R=20, unsat=1, sampled=0)
    b = ls.predicted_strips
    assert ls.matches(b(3, 3840, F32, si.DEFAULT, (), dna, 1 << 20, 20), dict(cell="i16", SL=64, R=20, strips=1, twin=0))
    assert ls.matches(b(3, 3840, F32, si.DEFAULT, ("force_f32",), dna, 1 << 20, 20), dict(cell="f32", SL=64, R=20, strips=1))
    assert ls.matches(b(3, 3840, U8SAT, si.DEFAULT, (), dna, 1 << 20, 20), dict(cell="f16", unsat=1, strips=1, mirror=0))
    assert ls.matches(b(3, 3840, U8SAT, si.DEFAULT, ("no_unsat",), dna, 1 << 20, 20), dict(cell="u8f16", unsat=0, strips=1))
    assert ls.matches(b(3, 3840, U8SAT, si.DEFAULT, ("no_unsat", "no_f16"), dna, 1 << 20, 20), dict(cell="u8i16", unsat=0, strips=1))
    assert ls.matches(b(3, 1100, F32, si.DEFAULT, (), aa, 1 << 20), dict(cell="i16", SL=16, R=32, strips=1))
    # lengths alone select every strip shape; the batches need strip_r where one of their lengths would go elsewhere
    assert [ls.natural_strip_length(r) for r in ls.R64S] == [2049, 2561, 3841]
    assert [ls.forced(64, r, ls.strip_lengths(64, r)) for r in ls.R64S] == [20, 24, 32] and ls.forced(16, 32, ls.strip_lengths(16, 32)) == 0
    for r in ls.R64S:
        two, one_row, full = ls.strip_lengths(64, r)
        assert [-(-m // (64 * r)) for m in (two, one_row, full)] == [2, 3, 3] and one_row % (64 * r) == 1 and two > 2048
    assert [-(-m // 512) for m in ls.strip_lengths(16, 32)] == [2, 3, 3]
    # the gate of bucket_fast_ok: strips only on ranges of at least 4096 columns
    want = b(3, 3840, F32, si.DEFAULT, (), dna, 4095, 20)
    assert not ls.fast_ok(3840, F32, si.DEFAULT, want, dna, 4095) and ls.fast_ok(3840, F32, si.DEFAULT, want, dna, 4096)
    # sub-chunks: 64 columns for a lone short float-engine query; 1/64 of the tile on float-engine strips; a power of two beyond
    # |x| + 64 for the uint8 engine
    assert ls.sub_len_of(F32, 1, 150, p(150, F32, si.DEFAULT, (), dna, 4096), 128) == 64
    assert ls.sub_len_of(F32, 3, 3840, want, 8192) == 128 and ls.sub_len_of(F32, 3, 3840, want, 4096) == 64
    assert ls.sub_len_of(U8SAT, 3, 3840, b(3, 3840, U8SAT, si.DEFAULT, (), dna, 4096, 20), 8192) == 4096
    assert ls.sub_len_of(U8SAT, 1, 150, p(150, U8SAT, si.DEFAULT, (), dna, 4096), 256) == 256


def test_cuts_are_where_the_cases_say(pgs):
    """Geometry of the lone and strip cases at the tile lengths the host gives them and at others."""
    for L, per_wg in ((32, 32), (150, 32), (152, 32), (512, 32), (512, 16), (640, 8), (2048, 8)):
        for CL in (128, 256, 1024, 2048, 3 * 512):
            c = ls.LoneCase(pgs, L, F32, si.DEFAULT, CL, per_wg)
            assert c.geometry_faults() == [], (L, CL, c.geometry_faults())
            t = c.cuts
            assert t["tb0"] % 2 == 0 and t["to"] % 2 == 1 and t["tb0"] < t["tb"] and t["to"] < t["te"]
            assert t["tb"] % 2 == 1 and t["te"] % 2 == 0 and t["tp"] % 2 == 1 and t["tq"] % 2 == 0 and t["tf"] % per_wg == 0 and t["tf"] > 0
            assert c.tiles(c.names.index("F")) > 2 * per_wg and c.tiles(c.names.index("O")) % 2 == 1
    c = ls.LoneCase(pgs, 160, F32, si.DEFAULT, 2048, 32, one_tile=True)
    assert c.geometry_faults() == [] and all(c.tiles(r) == 1 for r in range(4))
    for shape in [(64, r) for r in ls.R64S] + [(16, 32)]:
        for CL in (1024, 2048, 4096, 8192):
            sc = ls.strip_sc(F32, si.AA20 if shape[0] == 16 else b"ACGT")
            c = ls.StripCase(pgs, shape, ls.strip_lengths(*shape), F32, sc, CL)
            assert c.geometry_faults() == [], (shape, CL, c.geometry_faults())
            assert c.ranges[0][1] - c.ranges[0][0] == 4096 and all(b - a >= 4096 for a, b in c.ranges) and len(c.queries) % 2 == 1
            assert c.tiles(1) >= 3 and (CL < 4096 or c.tiles(2) == 1)


def test_inputs_hold_planted_hits(pgs, oracle):
    """Conditions on the inputs, from the oracle alone, at the tile lengths the host gives these cases on 256 CUs (the GPU cases check
    again at the one it chose): whole copies are perfect, partial ones are not, the overlap range holds background, and a copy with a
    gap at a strip boundary row scores more than its longer flank."""
    failures = []
    with si.make_pool() as pool:
        for L, CL, per_wg in ((32, 128, 32), (150, 128, 32), (512, 128, 32), (152, 128, 32), (640, 1024, 8), (2048, 2048, 8)):
            for sem in (F32, U8SAT):
                sc = ls.lone_sc(sem, L) if L <= 512 else ls.wide_sc(sem)
                for kw in ({}, {"one_letter": True}):
                    c = ls.LoneCase(pgs, L, sem, sc, CL, per_wg, **kw)
                    c.compute(oracle, pool)
                    failures.extend("lone %d rows sem %d %r: %s" % (L, sem, kw, f) for f in c.input_faults())
        for sem in (F32, U8SAT):
            c = ls.LoneCase(pgs, 160, sem, ls.lone_sc(sem, 160), 2048, 32, one_tile=True)
            c.compute(oracle, pool)
            failures.extend("one tile sem %d: %s" % (sem, f) for f in c.input_faults())
            for shape, CL in (((64, 20), 4096), ((64, 24), 8192), ((64, 32), 8192), ((16, 32), 2048)):
                sc = ls.strip_sc(sem, si.AA20 if shape[0] == 16 else b"ACGT")
                for lens in (ls.strip_lengths(*shape), (ls.natural_strip_length(shape[1]) if shape[0] == 64 else 1025,)):
                    c = ls.StripCase(pgs, shape, lens, sem, sc, CL)
                    c.compute(oracle, pool)
                    assert len(c.checks) >= 4
                    failures.extend("strips %r %r sem %d: %s" % (shape, lens, sem, f) for f in c.input_faults())
    assert not failures, "\n".join(failures)
