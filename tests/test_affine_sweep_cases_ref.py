"""The conditions on the inputs of tests/affine_sweep_cases.py, from tests/affine_ref.py and arithmetic alone (no GPU): that every
case puts its maximum where the case says, that the geometry it was built for is the one the host's expressions give, and that a
build with either of the two mutations named in affine_sweep_cases.py would return something else than the expected values."""
import pytest

from tests import affine_ref, affine_sweep_cases as sc, score_instances as si


# ---- A: tiles beyond the first workgroup ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.WORKGROUP_SHAPES, ids=lambda s: "SL%d_R%d" % s)
def test_workgroup_case_geometry(pgs, shape):
    c = sc.workgroup_case(pgs, shape)
    N = sc.nslot(shape[0])
    r0, r1, r2 = c.ranges
    assert all(si.pick_shape(len(q), c.slot) == shape for q in c.queries)        # one bucket of five: pairs (1, 0) (2, 3) (4)
    assert [len(q) for q in c.queries] == [c.L, c.l, c.L, c.L, c.L] and c.l < c.L
    assert r0[0] == 1 and sc.tiles(r0[1] - r0[0], sc.CL) == 2 * N + 3 > 2 * N
    assert sc.tiles(r1[1] - r1[0], sc.CL) == 5 <= N
    assert r2[1] == len(c.ref) and r2[1] - r2[0] == N * sc.CL + 1
    longest = max(b - a for a, b in c.ranges)
    assert longest == r0[1] - r0[0] and c.geometry(longest) == (sc.CL, sc.CL, 2 * N + 3, 3)
    assert c.geometry(len(c.ref))[3] == 3                           # the batch call over the whole reference: three workgroups too
    # where the planted maxima lie: workgroup = tile // N
    assert sc.tile_of(c.q2_end, sc.CL) == 2 * N + 1
    assert sc.tile_of(c.q4_ends[0], sc.CL) // N == 0 and sc.tile_of(c.q4_ends[1], sc.CL) // N == 2
    assert sc.tile_of(r2[1] - r2[0], sc.CL) == N                    # query 1's copy ends in range 2's tile of one column
    # query 0's inserted letters: the last column of tile N - 1 and the first two of tile N
    ins = c.ref.find(c.queries[0][:c.L // 2]) + c.L // 2 - r0[0] + 1            # 1-based column of the first inserted letter
    assert [sc.tile_of(ins + k, sc.CL) for k in range(3)] == [N - 1, N, N]


@pytest.mark.parametrize("shape", sc.WORKGROUP_SHAPES, ids=lambda s: "SL%d_R%d" % s)
def test_workgroup_case_maxima_lie_behind_the_first_workgroup(pgs, shape):
    c = sc.workgroup_case(pgs, shape)
    mx, (es, ei, ej) = c.compute()
    chk = c.conditions()
    r0 = c.ranges[0]
    # a kernel that sweeps only the first NSLOT tiles of a range (`slot` for `cg * NSLOT + slot`) returns less for queries 1 and 2
    for k, (head, whole) in chk["first_tiles"].items():
        assert head < whole, (shape, k, head, whole)
    assert mx[2, 1] == sc.MATCH * c.l and mx[0, 2] == sc.MATCH * c.L
    assert (es[1], ei[1], ej[1]) == (sc.MATCH * c.l, c.l, len(c.ref))
    assert (es[2], ei[2], ej[2]) == (sc.MATCH * c.L, c.L, r0[0] + c.q2_end)
    assert not chk["faults"], chk["faults"]                         # query 0's gap matters
    # query 4: two copies of one score, the earlier one is the end cell
    assert chk["copies"] == [(sc.MATCH * c.L, c.L, e) for e in c.q4_ends], chk["copies"]
    assert sc.occurrences(c.queries[4], c.ref) == 2
    assert (es[4], ei[4], ej[4]) == (sc.MATCH * c.L, c.L, c.q4_end_whole) and mx[0, 4] == sc.MATCH * c.L
    assert es[3] < 0.5 * sc.MATCH * c.L                             # unrelated


# ---- B: the end column around every cut ----------------------------------------------------------------------------------------
def test_cuts_are_what_the_configurations_make_of_them():
    assert sc.CUT_OFFSETS == tuple(range(-17, 2))
    for config, (cl, sl) in (("batch", sc.BATCH_GEOMETRY), ("lone", sc.LONE_GEOMETRY)):
        assert cl // sl == 4 and sc.CUT_N % cl != 0
        B = sc.CUT_AT[sc.CUT_KINDS[config]["sub"]]
        assert B % sl == 0 and B % cl != 0
        assert sc.CUT_AT[sc.CUT_KINDS[config]["tile"]] % cl == 0
    for shape in sc.CUT_SHAPES:
        L = shape[0] * shape[1]
        assert sc.sub_len(5, L, 1024) == 256 and sc.sub_len(1, L, sc.CL) == 64
        assert min(b - a for a, b in zip(sorted(sc.CUT_AT.values()), sorted(sc.CUT_AT.values())[1:])) >= L + 19   # copies keep off the next cut


@pytest.mark.parametrize("shape", sc.CUT_SHAPES, ids=lambda s: "SL%d_R%d" % s)
def test_cut_copies_are_unique_maxima_inside_the_host_window_only(pgs, shape):
    SL, R = shape
    outside = {"batch": set(), "lone": set()}
    clamp_cols = set()
    for d in sc.CUT_OFFSETS:
        c = sc.cut_case(pgs, shape, d)
        assert all(si.pick_shape(len(q)) == shape for q in c.queries)
        es, ei, ej = c.compute()
        for k, q in enumerate(c.queries):
            assert sc.occurrences(q, c.ref) == 1                    # only an exact copy scores MATCH * rows: the unique maximum
            assert (es[k], ei[k], ej[k]) == (sc.MATCH * len(q), len(q), c.ends[k]), (shape, d, k)
            for config, (cl, sl) in (("batch", sc.BATCH_GEOMETRY), ("lone", sc.LONE_GEOMETRY)):
                first = sc.reported_sub(len(q), c.ends[k], R, cl, sl)
                assert sc.in_window(c.ends[k], sc.locate_window(first, sl, sc.CUT_N)), (shape, d, k, config)
                narrowed = sc.in_window(c.ends[k], sc.locate_window(first, sl, sc.CUT_N, widen=0))
                kinds = sc.CUT_KINDS[config]
                if k == kinds["sub"]:
                    # the last lane lags SL - 1 columns: the last SL - 1 columns of the sub-chunk are reported with the next one
                    late = -(SL - 1) < d <= 0
                    assert first == (c.ends[k] - 1) // sl + late and narrowed == (not late), (shape, d, k, config)
                    if late:
                        outside[config].add(d)
                elif k == kinds["tile"]:
                    assert first == (c.ends[k] - 1) // sl and narrowed   # a tile drains every lane before its last sub-chunk is reported
                elif k == 3:
                    # own_lo clamps to 0; column 63 of a lone call is reported with sub-chunk 1 (the lane lags), where own_lo = 1
                    late = config == "lone" and c.ends[k] == 63
                    assert (first, sc.locate_window(first, sl, sc.CUT_N)[0]) == ((1, 2) if late else (0, 1)), (shape, d, config)
                    clamp_cols.add(c.ends[k])
                elif k == 4:
                    assert c.ends[k] == sc.CUT_N and first == (sc.CUT_N - 1) // sl
    # without the `- 63` these copies are outside the window: such a build cannot return the expected end cell
    for config in outside:
        assert outside[config] == set(range(-(SL - 2), 1)), (config, sorted(outside[config]))
    m0 = min(clamp_cols)
    assert clamp_cols == {m0, m0 + 1, 63}


# ---- C: ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["batch", "lone"])
def test_ties_exist_and_the_first_cell_is_known(pgs, config):
    c = sc.tie_case(pgs, config)
    cl, sl = c.geometry
    SL, R = sc.TIE_SHAPE
    assert sc.MATCH * sc.TIE_HALF < sc.REF_ARGS[2] + (sc.TIE_SEP - 1) * sc.REF_ARGS[3]      # no alignment joins a and b
    assert all(si.pick_shape(len(q)) == sc.TIE_SHAPE for q in c.queries)
    assert sc.sub_len(len(c.queries), sc.TIE_M, cl) == sl if config == "batch" else sc.sub_len(1, sc.TIE_M, cl) == sl
    es, ei, ej = c.compute()
    for k, name in enumerate(c.names):
        x = c.queries[k]
        (i1, j1), (i2, j2) = c.first[k], c.second[k]
        assert j1 < j2
        rows = name.startswith("rows")
        score = sc.MATCH * (sc.TIE_HALF if rows else sc.TIE_M)
        assert (es[k], ei[k], ej[k]) == (score, i1, j1), (config, name)         # the first maximum of the whole matrix
        # the second cell: the matrix of any slice of the reference is below the whole one cell by cell, so a slice behind column j1
        # whose own maximum is the score at (i2, j2) shows H(i2, j2) >= score, and the whole maximum is the score
        assert affine_ref.locate(x, c.ref[j1:j2], *sc.REF_ARGS) == (score, i2, j2 - j1), (config, name)
        assert sc.occurrences(x, c.ref) == (0 if rows else 2)
        if rows:                                                   # the plain three loops agree on the tile that holds both pieces
            lo = (j1 - 1) // cl * cl
            piece = c.ref[lo:min(lo + cl, lo + 300)]
            assert affine_ref.locate_loops(x, piece, *sc.REF_ARGS) == (score, i1, j1 - lo) == affine_ref.locate(x, piece, *sc.REF_ARGS)
            assert {i1, i2} == {sc.TIE_HALF, 2 * sc.TIE_HALF}
        col_sub = lambda j: (j - 1) // sl
        tile1, tile2 = sc.tile_of(j1, cl), sc.tile_of(j2, cl)
        if name == "same_sub":
            assert col_sub(j1) == col_sub(j2)
        elif name.startswith("trailing"):
            kth = int(name.split("_")[1])
            assert j1 == (col_sub(j1) + 1) * sl - kth + 1 and col_sub(j2) == col_sub(j1) + 1 and tile1 == tile2
            assert sc.reported_sub(i1, j1, R, cl, sl) == sc.reported_sub(i2, j2, R, cl, sl) == col_sub(j2)
            assert not sc.in_window(j1, sc.locate_window(col_sub(j2), sl, c.n, widen=0))       # without the `- 63`: the second copy
        elif name == "two_tiles":
            assert tile1 != tile2 and tile1 // sc.nslot(SL) == tile2 // sc.nslot(SL)
        elif name == "two_workgroups":
            assert tile1 // sc.nslot(SL) == 0 and tile2 // sc.nslot(SL) == 1
    assert ("two_workgroups" in c.names) == (config == "lone")
    assert sc.cgroups(c.n, cl, SL) == (2 if config == "lone" else 1)


# ---- D: mixed dispatch ---------------------------------------------------------------------------------------------------------
def test_mixed_dispatch_inputs(pgs):
    ref, qs, (es, ei, ej) = sc.bound_mix(pgs)
    smax = sc.BOUND_SCORING[0]
    assert sorted(len(q) for q in qs) == [100, 100, 100, 300, 300]
    assert smax * 101 <= 2040 < smax * 301 and si.pick_shape(100) != si.pick_shape(300)
    assert (es[0], ei[0], ej[0]) == (800, 100, 250) and (es[1], ei[1], ej[1]) == (2400, 300, 1200)
    assert es[2] == 800 - (6 + 2) and es[3] < 1200 and es[4] < 400             # the inserted pair costs open + extend
    ref, qs, (es, ei, ej) = sc.long_and_empty(pgs)
    assert [len(q) for q in qs] == [150, 600, 0, 513, 150]
    assert (es[2], ei[2], ej[2]) == (0, 0, 0)
    assert (es[1], ei[1], ej[1]) == (1800, 600, sc.MIX_N) and (es[0], ei[0], ej[0]) == (450, 150, 250)
    assert es[3] == 3 * 510 - (4 + 2) and ei[3] == 513 and ej[3] == 860
    for go in (2040, 2041):
        ref, qs, (es, ei, ej) = sc.gap_open_bound(pgs, go)
        assert (es[0], ei[0], ej[0]) == (450, 150, 350) and 225 <= es[1] < 300 and es[2] < 150   # no gap is worth gap_open: one half of query 1 and what its flank adds


# ---- E: more ranges than one launch group --------------------------------------------------------------------------------------
def test_many_ranges_rows_differ(pgs):
    c = sc.many_ranges(pgs)
    seven, every = c.compute()
    assert len(c.ranges) == sc.GROUP + 3 == 32771 == every.shape[0] and sc.GROUP % 7 == 1
    assert c.ranges[sc.GROUP] == c.DISTINCT[1] and (every[sc.GROUP] == seven[1]).all()
    assert all(si.pick_shape(len(q)) == (16, 2) for q in c.queries) and [len(q) for q in c.queries] == [16, 20, 27, 32]
    assert [r for r in range(7) if seven[r, 3] == 96] == [2, 4, 5]
    assert [r for r in range(7) if seven[r, 1] == 60] == [0, 2, 3, 4]
    # a decode without the group's offset gives range GROUP + k the row of range k: every one of them would be wrong
    assert all((seven[(sc.GROUP + k) % 7] != seven[k % 7]).any() for k in range(3))
