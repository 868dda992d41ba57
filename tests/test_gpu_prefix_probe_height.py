"""How a probed bucket picks the height of its prefix filter (host_pipeline.h align_range_core) on the device: 520
reads of 150 bp against about 60 k columns, the filter engaged by prefix_min_cols.  The probe of the first 64 reads runs at R = 16 on
tiles that fold row P alone; the rest follows at R = 16 (at most 4 probe reads offend), at the bucket's own R = 19 with the row-P
fold (more offend, and R = 19 can certify them), or not at all (most of the probe has no hit, or thresholds that drown at R = 19 too).

Every field of every read is compared with the library's own result under no_prefix, a fixed sample of 64 reads (the hand-built ones
among them) with the oracle, and the path and the counters with the numpy emulation of the rule (tests/prefix_rowp.py emulate_bucket)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from prefix_rowp import PROBE, bound, emulate_bucket

pytestmark = pytest.mark.gpu

M = 150
N = 60_000 + 133
COUNT = 520
R_OWN, R_LOW = 19, 16
SCORING = (3.0, -3.0, 2.0)
CAP = 64 + 1024 // COUNT
FIELDS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
LOW_NOTE, OWN_ROWP_NOTE, OWN_NOTE = "prefix[SL=2,R=16,P=32,fold=rowP]", "prefix[SL=2,R=19,P=38,fold=rowP]", "prefix[SL=2,R=19,P=38]"


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
    finally:
        ctx.close()
    print(path, cnt, kernel["name"])
    for k, (got, want) in enumerate(zip(res, plain)):
        for f in FIELDS:
            assert got[f] == want[f], ("no_prefix", k, f, got[f], want[f])
    must_sample = list(must_sample)
    sample = sorted(set(must_sample) | set(list(range(0, COUNT, 9))[:64 - len(must_sample)]))
    assert len(sample) <= 64 and set(must_sample) <= set(sample)
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda k: oracle.align(reads[k], y, pgs.F32), sample))
    for k, e in zip(sample, exp):
        for f in FIELDS:
            assert res[k][f] == e[f], ("oracle", k, f, res[k][f], e[f])
    return res, path, cnt, kernel


def _emulated(reads, y, low=True):
    with ThreadPoolExecutor(8) as ex:
        return emulate_bucket(reads, y, R_OWN, *SCORING, CAP, low=low, run=ex.map)


@pytest.fixture(scope="module")
def low_error_batch(pgs):
    y = pgs.synth.dna(811, N)
    reads, _ = pgs.synth.fast_reads_from_ref(y, 812, COUNT, M, sub_rate=0.01)
    return [r.tobytes() for r in reads], y.tobytes()


def test_low_height_accepted(pgs, oracle, low_error_batch):
    reads, y = low_error_batch
    emu = _emulated(reads, y)
    assert emu["outcome"] == "low" and emu["launches"] == [(R_LOW, True, PROBE), (R_LOW, True, COUNT - PROBE)], emu
    res, path, cnt, kernel = _run(pgs, oracle, reads, y)
    assert LOW_NOTE in path and "R=19" not in path.split("score[")[0] and "prefix_height[R=16,low]" in path, path
    off = len(emu["offenders"])
    assert (cnt["prefix_certified"], cnt["requeried"], cnt["whole_batch_again"]) == (COUNT - off, off, 0), (cnt, emu["offenders"])
    assert kernel["lanes"] == 2 and kernel["rows_per_lane"] == R_LOW and kernel["cells"] == len(y) * (2 * R_LOW * COUNT + M * off), kernel


def test_no_prefix_low_keeps_the_own_height(pgs, oracle, low_error_batch):
    reads, y = low_error_batch
    emu = _emulated(reads, y, low=False)
    assert emu["outcome"] == "own" and emu["launches"] == [(R_OWN, False, PROBE), (R_OWN, False, COUNT - PROBE)], emu
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, no_prefix_low=True)
    assert OWN_NOTE in path and "fold=" not in path and "prefix_height" not in path, path
    off = len(emu["offenders"])
    assert (cnt["prefix_certified"], cnt["requeried"], cnt["whole_batch_again"]) == (COUNT - off, off, 0), (cnt, emu["offenders"])
    assert kernel["rows_per_lane"] == R_OWN and kernel["cells"] == len(y) * (2 * R_OWN * COUNT + M * off), kernel


def test_low_height_rejected(pgs, oracle):
    """Six of the first 64 reads score between the two bounds (342 < B <= 360): 118 or 119 matching bases, then letters the reference
    does not hold.  Such a read's threshold at R = 19 is 12 to 15, which prefix rows over the read's own letters reach in most
    sub-chunks, so the reference is over A / C and these reads over G / T (tests/test_gpu_prefix_filter.py does the same)."""
    rng = np.random.default_rng(4321)
    y = bytearray(rng.choice(list(b"AC"), N).astype(np.uint8))
    hand = {}
    for h, pos in enumerate((2, 9, 21, 33, 47, 60)):
        k = 118 + h % 2
        letters = bytes(rng.choice(list(b"GT"), k).astype(np.uint8))
        at = (20 + 35 * h) * 256 + 7 * h
        y[at:at + k] = letters
        hand[pos] = letters + b"N" * (M - k)
    y = np.frombuffer(bytes(y), dtype=np.uint8)
    drawn, _ = pgs.synth.fast_reads_from_ref(y, 4322, COUNT, M, sub_rate=0.004)
    reads = [hand.get(k, drawn[k].tobytes()) for k in range(COUNT)]
    y = y.tobytes()
    assert bound(M, R_OWN, 3.0, 2.0) == 342 and bound(M, R_LOW, 3.0, 2.0) == 360
    emu = _emulated(reads, y)
    assert emu["outcome"] == "own_rowp" and set(hand) <= set(emu["riders"]) and not set(hand) & emu["offenders"], emu
    assert emu["launches"] == [(R_LOW, True, PROBE), (R_OWN, True, COUNT - PROBE + len(emu["riders"]))], emu["launches"]
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, must_sample=sorted(hand))
    for pos, x in hand.items():
        assert 342 < res[pos]["score"] == 3 * (len(x) - x.count(b"N")) <= 360, (pos, res[pos]["score"])
    assert LOW_NOTE in path and OWN_ROWP_NOTE in path and "prefix_height[R=19,own,riders=%d]" % len(emu["riders"]) in path, path
    off = len(emu["offenders"])
    assert (cnt["prefix_certified"], cnt["requeried"], cnt["whole_batch_again"]) == (COUNT - off, off, 0), (cnt, emu["offenders"])
    assert kernel["rows_per_lane"] == R_OWN, kernel


def test_probe_of_reads_whose_threshold_drowns(pgs, oracle, low_error_batch):
    """40 of the first 64 reads keep 118 or 119 of their bases and score about 354, above the bound 342 of R = 19 — but over the
    reference's own four letters their threshold there, about 12, is reached in most sub-chunks: the probe's vote counts them as not
    certifiable at R = 19 either (the flags of that threshold on the probe's own values exceed the cap), and the probe fails instead
    of sending the bucket through a second prefix sweep that would certify nothing.  (10 % substitutions on the 50 Mbp bench reference do the same: CHANGELOG.md.)"""
    reads, y = low_error_batch
    reads = list(reads)
    for k in range(40):
        pos = (k * 8) % PROBE + k // 8
        keep = 118 + k % 2
        reads[pos] = reads[pos][:keep] + b"N" * (M - keep)
    emu = _emulated(reads, y)
    assert emu["outcome"] == "probe_failed" and emu["launches"] == [(R_LOW, True, PROBE)], emu
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, must_sample=range(0, 16))
    assert LOW_NOTE in path and "prefix_probe_failed" in path and "whole_again" in path, path
    assert "R=19,P=38" not in path and "prefix_height" not in path, path
    assert (cnt["prefix_certified"], cnt["requeried"], cnt["whole_batch_again"]) == (0, 0, 1), cnt


def test_probe_without_hits(pgs, oracle, low_error_batch):
    """40 of the first 64 reads are random: no height certifies them, the probe fails at the price of its one launch at R = 16, and the
    sweep decides for everybody."""
    reads, y = low_error_batch
    reads = list(reads)
    for k in range(40):
        reads[(k * 8) % PROBE + k // 8] = pgs.synth.dna(7000 + k, M).tobytes()
    emu = _emulated(reads, y)
    assert emu["outcome"] == "probe_failed" and emu["launches"] == [(R_LOW, True, PROBE)], emu
    res, path, cnt, kernel = _run(pgs, oracle, reads, y, must_sample=range(0, 16))
    assert LOW_NOTE in path and "prefix_probe_failed" in path and "whole_again" in path, path
    assert "R=19,P=38" not in path and "prefix_height" not in path, path
    assert (cnt["prefix_certified"], cnt["requeried"], cnt["whole_batch_again"]) == (0, 0, 1), cnt
