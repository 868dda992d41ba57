"""The thin stage of the prefix filter inside the chain (host_pipeline.h prefix_bucket round 2) on the device:
the batch of tests/prefix_thin_flow_case.py, 1040 reads of 150 bp against 60 133 columns with the filter engaged by prefix_min_cols and
its thin stage by prefix_thin_min_cols (without the second option a range this short keeps the parent's flow).

Every field of every read equals the library's own result under no_prefix and under no_prefix_thin, and a fixed sample of 64 reads (the
hand-built ones among them) equals the oracle.  Counters and notes are compared with the numpy emulation of tests/prefix_thin.py:
  * on the tiles the library chooses, the counters that do not depend on how the range is cut into tiles;
  * with option chunk = 61 440 (one tile per read, the range as the emulation takes it) prefix_thin_items, the kept sub-chunks of every
    thin launch and `candidates` as well.  The sweep of the bucket's offenders adds its own candidates, which no emulation here knows:
    a batch without offenders is compared exactly, with and without the stage; one with offenders — the same reads in both flows, so
    the same sweep — by the difference between the two runs.
At m = 150 the bound of P2 = 38, 336, lies below the bound of every pass (372 at P = 26, 354 at P = 32): a read with B0 under it is an
offender of the pass before the thin stage is asked, and takes the parent's path — the sweep of all rows (c)."""
from concurrent.futures import ThreadPoolExecutor

import pytest

from prefix_cascade import Read, bound, emulate_chain as emulate_parent_chain
from prefix_thin import MIN_FLAGS, P2, emulate_chain, thin_cap
from prefix_thin_flow_case import COUNT, FAMILY, HEIGHTS, M, QCAP, SCORING, build

pytestmark = pytest.mark.gpu

FIELDS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
ONE_TILE = 61_440
FLIP = ord("G") ^ ord("T")


def _low(oracle, case, h, lo, hi):
    """Planted stretch h with substitutions below row 40, four rows apart, as many as leave lo < B0 <= hi (the oracle decides)."""
    site, at = case["stretches"][h]
    for k in range(8, 26):
        x = bytearray(site)
        for j in range(k):
            x[42 + 4 * j] ^= FLIP
        score = oracle.align(bytes(x), case["y"][at - 32:at + M + 32], oracle.F32)["score"]
        if lo < score <= hi:
            return bytes(x)
    raise AssertionError((h, lo, hi))


def _batch(case, hand):
    reads, st = list(case["drawn"]), list(case["state"])
    for pos, x in hand.items():
        reads[pos], st[pos] = x, Read(x, case["y"], SCORING, HEIGHTS)
    return reads, st


def _one(pgs, reads, y, prefix_thin_min_cols=50_000, **options):
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 50_000)
        ctx.set_option("prefix_thin_min_cols", prefix_thin_min_cols)
        for key, value in options.items():
            ctx.set_option(key, value)
        res = ctx.align_batch(reads, y, semantics=pgs.F32)
        return res, " ".join(ctx.last_path()), ctx.last_counters(), ctx.last_kernel()
    finally:
        ctx.close()


def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert a[f] == b[f], (what, k, f, a[f], b[f])


def _run(pgs, oracle, reads, st, y, must_sample):
    """Results against no_prefix, no_prefix_thin and the oracle; then (emulation with the stage, without it, the two one-tile runs)."""
    res, path, cnt, kernel = _one(pgs, reads, y)
    plain = _one(pgs, reads, y, no_prefix=True)
    assert "prefix[" not in plain[1]
    _same(res, plain[0], "no_prefix")
    parent = _one(pgs, reads, y, no_prefix_thin=True)
    assert "prefix_thin[" not in parent[1] and (parent[2]["prefix_thinned"], parent[2]["prefix_thin_items"]) == (0, 0), parent[1:3]
    _same(res, parent[0], "no_prefix_thin")
    short = _one(pgs, reads, y, prefix_thin_min_cols=None)           # (the gate at its default, 4 Mi columns: no thin stage either)
    assert "prefix_thin[" not in short[1] and short[2] == parent[2] and short[1] == parent[1], (short[1:3], parent[1:3])
    sample = sorted(set(must_sample) | set(list(range(0, len(reads), 17))[:64 - len(must_sample)]))
    assert len(sample) <= 64 and set(must_sample) <= set(sample)
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda k: oracle.align(reads[k], y, pgs.F32), sample))
    for k, e in zip(sample, exp):
        for f in FIELDS:
            assert res[k][f] == e[f], ("oracle", k, f, res[k][f], e[f])
    emu, old = emulate_chain(st, 19, QCAP), emulate_chain(st, 19, QCAP, thin=False)
    ref = emulate_parent_chain(st, 19, QCAP)
    assert (old["launches"], old["second"], old["offenders"]) == (ref["launches"], ref["second"], ref["offenders"])   # (thin=False IS the parent's chain)
    print(path, cnt, emu["passes"], emu["thinned"], emu["thin_items"], emu["candidates"], sorted(emu["offenders"]))
    # the tiles the library chooses: what does not depend on the cut
    off = len(emu["offenders"])
    assert emu["outcome"] == "chain" and emu["start"] == 13, emu
    assert "prefix_height[R=13,start]" in path and "whole_again" not in path, path
    assert (cnt["prefix_certified"], cnt["prefix_second_pass"], cnt["requeried"], cnt["prefix_thinned"]) == \
        (COUNT - off, len(emu["second"]), off, emu["thinned"]), (cnt, emu["second"], sorted(emu["offenders"]))
    # (items: >= only.  On these tiles a flag near a tile's end shows again in the next tile's first sub-chunk, DESIGN.md L19 row-P
    # variant, so the device may list more; equality is asserted below, where one tile holds the range)
    assert cnt["prefix_thin_items"] >= emu["thin_items"] and ("prefix_thin[P2=%d," % P2 in path) == (emu["thin_items"] > 0), (cnt, path)
    assert all(count >= 2 for _, count, _, _ in emu["passes"]), emu["passes"]     # (a pass of one read has sub-chunks of 64 columns)
    offp = len(old["offenders"])
    assert (parent[2]["prefix_certified"], parent[2]["prefix_second_pass"], parent[2]["requeried"]) == (COUNT - offp, len(old["second"]), offp), parent[2]
    # one tile per read: every counter, and every thin launch's note
    tile = _one(pgs, reads, y, chunk=ONE_TILE)
    tile_parent = _one(pgs, reads, y, chunk=ONE_TILE, no_prefix_thin=True)
    assert tile[3]["chunk_len"] == ONE_TILE, tile[3]
    _same(tile[0], res, "one tile")
    _same(tile_parent[0], res, "one tile, no_prefix_thin")
    for key in ("prefix_certified", "prefix_second_pass", "requeried", "prefix_thinned"):
        assert tile[2][key] == cnt[key] and tile_parent[2][key] == parent[2][key], (key, tile[2], tile_parent[2])
    assert tile[2]["prefix_thin_items"] == emu["thin_items"], (tile[2], emu["passes"])
    for R, count, items, kept in emu["passes"]:
        if items:
            assert "prefix_thin[P2=%d,items=%d,kept=%d]" % (P2, items, kept) in tile[1], (R, count, items, kept, tile[1])
    return emu, old, tile[2], tile_parent[2]


def test_family_is_thinned_and_certified(pgs, oracle):
    """(a), with more flags in the pass than kThinMinFlags: the twelve family reads draw 212 flags each at P = 26 and keep one to three
    sub-chunks; they are certified where the parent's flow sends them through a second pass at P = 32.  Everybody else's flags take the
    thin stage too.  No read is swept in either flow: `candidates` is the chain's, and the thin stage lowers it."""
    case = build()
    hand = {100 + 70 * k: x for k, x in enumerate(case["family"])}
    reads, st = _batch(case, hand)
    emu, old, cnt, cnt_parent = _run(pgs, oracle, reads, st, case["y"], sorted(hand))
    assert not emu["offenders"] and not emu["second"], emu
    assert set(old["second"]) == set(hand) and not old["offenders"], old
    rest = emu["passes"][1]
    assert rest[2] > 2 * MIN_FLAGS and emu["thinned"] == COUNT - 64 and FAMILY <= rest[3] - (rest[1] - FAMILY) <= 3 * FAMILY, emu["passes"]
    assert (cnt["candidates"], cnt_parent["candidates"]) == (emu["candidates"], old["candidates"]), (cnt, cnt_parent, emu["candidates"], old["candidates"])
    assert cnt["candidates"] < cnt_parent["candidates"], (cnt, cnt_parent)


def test_offender_after_thinning_and_below_the_bound(pgs, oracle):
    """(b) `stays_over` draws 201 flags at P = 26 and keeps them all: an offender after the thin stage, again after the second pass at
    P = 32 (thinned there as well), then swept on all rows — with fewer flags in the pass than kThinMinFlags, so nobody else is thinned.
    (c) B0 <= 336, under the bound of P2 and of every pass: never thinned, never in a second pass, swept on all rows.  A third read,
    354 < B0 <= 372, offends at P = 26 by its bound and shares the second pass: there its threshold of a few units drowns in the
    planted stretches, with the stage and without (and a pass of two reads keeps sub-chunks of 256 columns, which the emulation
    assumes).  All three offend without the thin stage too, so the sweep adds the same candidates to both runs: the DIFFERENCE of
    `candidates` between the two runs is the chain's, and equals the emulation's."""
    case = build()
    under, mid = _low(oracle, case, 1, 300, 336), _low(oracle, case, 0, 354, 372)
    hand = {300: case["stays_over"], 700: under, 950: mid}
    reads, st = _batch(case, hand)
    assert bound(M, 13, 3.0, 2.0) == 372 and bound(M, 16, 3.0, 2.0) == 354 and 3.0 * max(M - P2, P2) == 336
    emu, old, cnt, cnt_parent = _run(pgs, oracle, reads, st, case["y"], sorted(hand))
    assert emu["offenders"] == old["offenders"] == set(hand) and emu["second"] == old["second"] == [300, 950], (emu, old)
    assert emu["thinned"] == 3 and emu["passes"][0][2:] == (0, 0) and emu["passes"][1][2:] == (202, 201), emu["passes"]
    assert emu["passes"][2][:2] == (16, 2) and emu["passes"][2][2] == emu["passes"][2][3] > 2 * 201, emu["passes"]
    assert emu["passes"][1][2] < MIN_FLAGS // 2 and thin_cap(QCAP) > 2 * emu["passes"][2][2]
    assert cnt["candidates"] - cnt_parent["candidates"] == emu["candidates"] - old["candidates"] > 0, \
        (cnt, cnt_parent, emu["candidates"], old["candidates"])
    # ... and what the sweep of the three reads added is at most query_flag_cap + 1 each
    assert 0 <= cnt["candidates"] - emu["candidates"] <= len(hand) * (QCAP + 1), (cnt, emu["candidates"])
