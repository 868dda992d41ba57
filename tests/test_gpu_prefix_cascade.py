"""The prefix filter's heights as a chain (host_pipeline.h prefix_chain) on the device: 1040 reads of 150 bp against
about 60 k columns, the filter engaged by prefix_min_cols.  The probe of the first 64 reads runs at R = 13 on tiles that fold row P at
every step (no slack); the rest starts at the lowest height the probe's offender count pays for, and the offenders of that pass take
one pass at the next height before the sweep of all rows.

The reference is over A / C, and the hand-built reads — copies of planted G / T stretches with substitutions below row 40 — are over
G / T: their thresholds are a few units, which prefix rows over the reference's own letters would reach in most sub-chunks
(tests/test_gpu_prefix_probe_height.py does the same).  k substitutions leave B0 = 450 - 6 k or a little more (the oracle picks k); the bounds with no slack are 372 at
P = 26, 354 at P = 32 and 336 at P = 38.

Every field of every read is compared with the library's own result under no_prefix, a fixed sample of 64 reads (the hand-built ones
among them) with the oracle, and the path, the counters and last_kernel().cells with the numpy emulation of the rule
(tests/prefix_cascade.py emulate_chain)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from prefix_cascade import CHAIN, LANES, PROBE, Read, bound, emulate_chain, emulate_parent
from row_sampled_fold import MK

pytestmark = pytest.mark.gpu

M = 150
N = 60_000 + 133
COUNT = 1040
HEIGHTS = (13, 16, 19)
SCORING = (3.0, -3.0, 2.0)
FIELDS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
SITES = 16                                                           # planted G / T stretches, 13 sub-chunks apart


def _cap(count):
    return 64 + 1024 // count


@pytest.fixture(scope="module")
def base(pgs):
    """(reference with the planted stretches, the stretches, the drawn reads and their emulation state)."""
    rng = np.random.default_rng(2601)
    y = bytearray(rng.choice(list(b"AC"), N).astype(np.uint8))
    sites = []
    for h in range(SITES):
        letters = bytes(rng.choice(list(b"GT"), M).astype(np.uint8))
        at = (10 + 13 * h) * 256 + 7 * h
        y[at:at + M] = letters
        sites.append((letters, at))
    ya = np.frombuffer(bytes(y), dtype=np.uint8)
    drawn, _ = pgs.synth.fast_reads_from_ref(ya, 2602, COUNT, M, sub_rate=0.001)
    y = bytes(y)
    drawn = [r.tobytes() for r in drawn]
    # The emulation takes the range as one tile.  The device cuts it into tiles whose warm-up columns count for their first sub-chunk,
    # so a flag near a tile's end may show twice: results do not depend on it, but whether a read is over its cap does when its count
    # is close to the cap.  The drawn reads stay clear of that: at most half the cap, or at least twice the cap, at every height.
    def make(x):
        r = Read(x, y, SCORING, HEIGHTS)
        B0 = r.emulate(HEIGHTS[0], 1 << 30)["B0"]
        for mk in (1, MK):
            for R in HEIGHTS[mk > 1:]:                               # (no test emulates R = 13 on the tiles that fold every 4th step)
                if B0 > bound(M, R, SCORING[0], SCORING[2], mk):
                    flags = int(np.count_nonzero(r.val[R, mk] >= B0 - SCORING[0] * (M - LANES * R) - (mk - 1) * SCORING[2]))
                    assert not 32 < flags < 128, (x, mk, R, B0, flags)
        return r

    with ThreadPoolExecutor(8) as ex:
        state = list(ex.map(make, drawn))
    return y, sites, drawn, state


def _mid(oracle, base, h, lo, hi):
    """Planted stretch h with substitutions (G <-> T) below row 40, five rows apart, as many as leave lo < B0 <= hi.  k of them leave
    450 - 6 k or, where a pair of gaps does better over two letters, a little more: the oracle decides."""
    y, (site, at) = base[0], base[1][h]
    for k in range(8, 22):
        x = bytearray(site)
        for j in range(k):
            x[42 + 5 * j] ^= ord("G") ^ ord("T")
        score = oracle.align(bytes(x), y[at - 32:at + M + 32], oracle.F32)["score"]
        if lo < score <= hi:
            return bytes(x)
    raise AssertionError((h, lo, hi))


def _batch(base, hand, count=COUNT):
    """reads (hand: position -> read, replacing the drawn one) and their emulation state."""
    y, _, drawn, state = base
    reads, st = list(drawn[:count]), list(state[:count])
    for pos, x in hand.items():
        reads[pos], st[pos] = x, Read(x, y, SCORING, HEIGHTS)
    return reads, st


def _run(pgs, oracle, reads, y, must_sample=(), **options):
    """(results, path, counters, kernel) with the filter engaged, after checking every read against no_prefix and 64 against the oracle."""
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_min_cols", 50_000)
        for key, value in options.items():
            ctx.set_option(key, value)
        res = ctx.align_batch(reads, y, semantics=pgs.F32)
        path, cnt, kernel = " ".join(ctx.last_path()), ctx.last_counters(), ctx.last_kernel()
        ctx.set_option("no_prefix")
        plain = ctx.batch_run(semantics=pgs.F32)
        assert "prefix[" not in " ".join(ctx.last_path())
        cnt["plain_requeried"] = ctx.last_counters()["requeried"]     # (the plain sweep's own: reads over the cap of its sampled maximum)
    finally:
        ctx.close()
    print(path, cnt, kernel["name"], kernel["cells"])
    for k, (got, want) in enumerate(zip(res, plain)):
        for f in FIELDS:
            assert got[f] == want[f], ("no_prefix", k, f, got[f], want[f])
    must_sample = list(must_sample)
    sample = sorted(set(must_sample) | set(list(range(0, len(reads), 17))[:64 - len(must_sample)]))
    assert len(sample) <= 64 and set(must_sample) <= set(sample)
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda k: oracle.align(reads[k], y, pgs.F32), sample))
    for k, e in zip(sample, exp):
        for f in FIELDS:
            assert res[k][f] == e[f], ("oracle", k, f, res[k][f], e[f])
    return res, path, cnt, kernel


def _check(emu, path, cnt, kernel, n, y, step=True):
    """Path notes, counters and swept cells against the emulated chain."""
    tag = ",fold=rowP,step=1]" if step else ",fold=rowP]"
    for R, _ in emu["launches"]:
        assert "prefix[SL=2,R=%d,P=%d%s" % (R, LANES * R, tag) in path, (R, path)
    for R in HEIGHTS:
        if R not in [r for r, _ in emu["launches"]]:
            assert "prefix[SL=2,R=%d," % R not in path, (R, path)
    off = len(emu["offenders"])
    if emu["outcome"] == "probe_failed":
        assert "prefix_probe_failed" in path and "whole_again" in path and "prefix_height" not in path and "prefix_second" not in path, path
        # the sweep decides for everybody: what it sweeps again by itself is what it sweeps again without the filter
        assert (cnt["prefix_certified"], cnt["prefix_second_pass"], cnt["requeried"], cnt["whole_batch_again"]) == \
            (0, 0, cnt["plain_requeried"], 1), cnt
        return
    note = "prefix_height[R=%d,start%s]" % (emu["start"], ",riders=%d" % len(emu["riders"]) if emu["riders"] else "")
    assert note in path and "prefix_probe_failed" not in path and "whole_again" not in path, (note, path)
    if emu["second"]:
        assert "prefix_second[R=%d,n=%d]" % (emu["launches"][-1][0], len(emu["second"])) in path, path
    else:
        assert "prefix_second" not in path, path
    assert (cnt["prefix_certified"], cnt["prefix_second_pass"], cnt["requeried"], cnt["whole_batch_again"]) == \
        (n - off, len(emu["second"]), off, 0), (cnt, sorted(emu["offenders"]), emu["second"])
    assert kernel["lanes"] == LANES and kernel["rows_per_lane"] == emu["start"], kernel
    assert kernel["cells"] == len(y) * (sum(LANES * R * c for R, c in emu["launches"]) + M * off), (kernel["cells"], emu["launches"], off)
    assert ("row P folded every step" if step else "row P folded every 4th step") in kernel["name"], kernel["name"]


def test_starts_low_and_offenders_take_a_second_pass(pgs, oracle, base):
    """(a) A low-error batch starts at R = 13.  Six reads in the rest carry 13 to 15 substitutions, 354 < B0 <= 372: they offend at
    P = 26, the second pass at P = 32 certifies them.  Two more, B0 = 354 and 348, skip it and are swept on all rows."""
    y = base[0]
    mids = {100 + 90 * h: _mid(oracle, base, h, 372 - 6 * (h % 3 + 1), 372 - 6 * (h % 3)) for h in range(6)}
    lows = {700: _mid(oracle, base, 6, 348, 354), 900: _mid(oracle, base, 7, 342, 348)}
    reads, st = _batch(base, {**mids, **lows})
    assert bound(M, 13, 3.0, 2.0) == 372 and bound(M, 16, 3.0, 2.0) == 354 and bound(M, 19, 3.0, 2.0) == 336
    emu = emulate_chain(st, 19, _cap(COUNT))
    assert emu["outcome"] == "chain" and emu["start"] == 13 and not emu["riders"], emu
    assert set(mids) <= set(emu["second"]) and not set(mids) & emu["offenders"] and set(lows) <= emu["offenders"] and not set(lows) & set(emu["second"]), emu
    assert emu["launches"] == [(13, PROBE), (13, COUNT - PROBE), (16, len(emu["second"]))], emu["launches"]
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, must_sample=sorted({**mids, **lows}))
    for pos in mids:
        assert 354 < res[pos]["score"] <= 372, (pos, res[pos]["score"])
    for pos in lows:
        assert res[pos]["score"] <= 354, (pos, res[pos]["score"])
    _check(emu, path, cnt, kernel, COUNT, y)


def test_start_moves_up_with_riders(pgs, oracle, base):
    """(b) 12 of the first 64 reads are such mid-score reads: more than the 10 that R = 13 pays for.  The rest starts at R = 16 with
    them as riders; reads with 336 < B0 <= 354 offend that pass and take their second pass at R = 19; B0 <= 336 is swept on all rows."""
    y = base[0]
    mids = {5 * h + 2: _mid(oracle, base, h, 372 - 6 * (h % 3 + 1), 372 - 6 * (h % 3)) for h in range(12)}
    second = {300: _mid(oracle, base, 12, 348, 354), 640: _mid(oracle, base, 13, 342, 348), 1000: _mid(oracle, base, 14, 336, 342)}
    lows = {820: _mid(oracle, base, 15, 324, 336)}
    reads, st = _batch(base, {**mids, **second, **lows})
    emu = emulate_chain(st, 19, _cap(COUNT))
    assert emu["outcome"] == "chain" and emu["start"] == 16 and emu["o"][0] >= 12 and set(mids) <= set(emu["riders"]), emu
    assert set(second) <= set(emu["second"]) and set(lows) <= emu["offenders"] and not (set(mids) | set(second)) & emu["offenders"], emu
    assert emu["launches"] == [(13, PROBE), (16, COUNT - PROBE + len(emu["riders"])), (19, len(emu["second"]))], emu["launches"]
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, must_sample=sorted({**mids, **second, **lows}))
    _check(emu, path, cnt, kernel, COUNT, y)


def test_probe_without_hits(pgs, oracle, base):
    """(c) 40 of the first 64 reads are random: no height certifies them, the probe fails at the price of its one launch at R = 13."""
    y = base[0]
    hand = {(k * 8) % PROBE + k // 8: pgs.synth.dna(7100 + k, M).tobytes() for k in range(40)}
    reads, st = _batch(base, hand)
    emu = emulate_chain(st, 19, _cap(COUNT))
    assert emu["outcome"] == "probe_failed" and emu["launches"] == [(13, PROBE)], emu
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, must_sample=range(0, 16))
    _check(emu, path, cnt, kernel, COUNT, y)


def test_options_give_the_parents_flow_and_the_sampled_fold(pgs, oracle, base):
    """(d) no_prefix_cascade: the flow of the smaller buckets (probe at R = 16 on the tiles that fold every 4th step, the rest low).
    no_prefix_step: the chain on those tiles, with their slack of three gaps in every bound and threshold (over this reference's two
    letters that slack puts some reads' flag counts near the cap, where the one-tile emulation is no guide: notes and totals only)."""
    y = base[0]
    reads, st = _batch(base, {})
    old = emulate_parent(st, 19, _cap(COUNT))
    assert old["outcome"] == "low" and old["launches"] == [(16, PROBE), (16, COUNT - PROBE)], old
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, no_prefix_cascade=True)
    assert "prefix[SL=2,R=16,P=32,fold=rowP]" in path and "prefix_height[R=16,low]" in path and "step=1" not in path and "prefix_second" not in path, path
    off = len(old["offenders"])
    assert (cnt["prefix_certified"], cnt["prefix_second_pass"], cnt["requeried"]) == (COUNT - off, 0, off), cnt
    assert kernel["rows_per_lane"] == 16 and kernel["cells"] == len(y) * (32 * COUNT + M * off), kernel
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, no_prefix_step=True)
    assert "prefix[SL=2,R=13,P=26,fold=rowP]" in path and "prefix_height[R=" in path and ",start" in path and "step=1" not in path, path
    assert cnt["prefix_certified"] + cnt["requeried"] == COUNT and cnt["whole_batch_again"] == 0, cnt
    assert "row P folded every 4th step" in kernel["name"], kernel["name"]


@pytest.mark.parametrize("count", [CHAIN - 1, CHAIN])
def test_gate(pgs, oracle, base, count):
    """(e) 1023 reads take the flow of the smaller buckets, 1024 the chain."""
    y = base[0]
    reads, st = _batch(base, {}, count)
    if count < CHAIN:
        old = emulate_parent(st, 19, _cap(count))
        assert old["outcome"] == "low", old
        res, path, cnt, kernel = _run(pgs, oracle, reads, y)
        assert "prefix[SL=2,R=16,P=32,fold=rowP]" in path and "prefix_height[R=16,low]" in path and "step=1" not in path, path
        off = len(old["offenders"])
        assert (cnt["prefix_certified"], cnt["prefix_second_pass"], cnt["requeried"]) == (count - off, 0, off), cnt
        assert kernel["cells"] == len(y) * (32 * count + M * off), kernel
    else:
        emu = emulate_chain(st, 19, _cap(count))
        assert emu["outcome"] == "chain" and emu["start"] == 13, emu
        res, path, cnt, kernel = _run(pgs, oracle, reads, y)
        _check(emu, path, cnt, kernel, count, y)
