"""How the prefix tiles of sw_score_kernel (SL = 2 lanes x R = 19 rows) get their reference codes (stage_load: 32 codes per lane and
segment, as dword and 16-byte loads with an edge patch), on the device: one range [lo, hi) of the reference per case.

The kernel pads every column outside [lo, hi), so the range's raw key of a read is that of the sub-reference y[lo:hi]; it is compared,
exactly, with the numpy emulation of what the tiles publish (tests/prefix_filter.py prefix_values), as tests/test_gpu_prefix_tiles.py
does for whole references.  The ranges put lo on every byte of a dword and hi in mid dword, in mid vector and at the end of the buffer;
the reads sit at both ends, one copy lies across hi with its better part behind it, one ends just in front of lo
(tests/prefix_stage_cases.py; tests/test_prefix_stage_ref.py checks on the oracle's matrices that the columns do what is said there).
A kernel that read past hi, or in front of lo, would report more than the emulation for those two."""
import pytest

from prefix_filter import LANES, prefix_values
from prefix_stage_cases import NAMES, P, PAIRS, R, SCORING, batch
from row_sampled_fold import SUB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_prefix_stage_range_keys(pgs, pair):
    lo, hi = pair
    match, mismatch, gap = SCORING
    reads, y = batch(lo, hi)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_tiles")
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        got = ctx.score_ranges([(lo, hi)], semantics=pgs.F32, match=match, mismatch=mismatch, gap=gap)[0]
        path = " ".join(ctx.last_path())
        kernel = ctx.last_kernel()
    finally:
        ctx.close()
    assert "prefix[SL=2,R=19,P=38]" in path, path
    assert kernel["chunk_len"] == SUB == 256, kernel
    assert kernel["lanes"] == LANES and kernel["rows_per_lane"] == R, kernel
    assert hi - lo > 128 * kernel["chunk_len"], "a second workgroup must run"
    assert len(reads) % 2 == 1
    for k, (name, x) in enumerate(zip(NAMES, reads)):
        val = prefix_values(x, y[lo:hi], R, match, mismatch, gap)
        print("[%d, %d) read %d (%s): key %g, emulated %g of at most %g" % (lo, hi, k, name, got[k], val.max(), match * P))
        assert got[k] == val.max(), (name, got[k], float(val.max()))
