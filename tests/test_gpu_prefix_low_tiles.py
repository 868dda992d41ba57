"""The LOW prefix tiles of sw_score_kernel that fold row P at every step (ROWP with MK = 1; host_score.h kR2Step) on the device: R = 8
and 10 rows per lane, P = 16 and 20.

As tests/test_gpu_prefix_step_tiles.py does for R = 13, 16 and 19: option prefix_rowp_step = R makes score_ranges sweep the bucket of
150 bp reads with that instance, and prefix_values reads back what every tile published per sub-chunk.  Both are compared, exactly,
with the numpy emulation (tests/prefix_cascade.py tile_values with mk = 1) on the warm-up the library reports: the maximum of row P
over the sub-chunk's columns, shifted by the one column that lane 1 lags lane 0.  The range is a little over one tile of 1024 columns,
so a second tile runs behind its warm-up and its last sub-chunk is partial; range starts are no multiples of 4 (the staging's byte
shift); one read has its mismatch in row P itself, one copy's row P ends in the second tile."""
import numpy as np
import pytest

from prefix_cascade import LANES, tile_values
from row_sampled_fold import SUB

pytestmark = pytest.mark.gpu

M = 150
CHUNK = 1024
N = CHUNK + SUB + 77 + 17
SCORING = (3.0, -3.0, 2.0)
RANGES = [(0, N - 17), (1, N - 17), (13, N), (3, N - 5)]
NAMES = ["starts_at_lo", "across_the_tiles", "ends_at_hi", "mismatch_in_row_P", "mismatch_above_row_P", "prefix_across_the_tiles", "no_hit"]
LOW = (8, 10)                                                        # kR2Step of host_score.h


def _batch(R, lo, hi):
    P = LANES * R
    rng = np.random.default_rng(9700 + 64 * R + lo)
    y = bytearray(rng.choice(list(b"ACGT"), N).astype(np.uint8))
    other = lambda c: b"ACGT"[(b"ACGT".index(c) + 1) % 4]

    def copy(at, change=None):
        x = bytearray(y[at:at + M])
        if change is not None:
            x[change] = other(x[change])
        return bytes(x)

    reads = [copy(lo),
             copy(lo + CHUNK - 60),                                  # rows 1 .. P end in the first tile, the copy in the second
             bytes(y[hi - P:hi]) + b"N" * (M - P),                    # row P ends in the range's last column
             copy(lo + 300, P - 1),                                  # the read's letter of row P is wrong
             copy(lo + 600, P - 2),                                  # ... of the row above it
             copy(lo + CHUNK - P // 2),                              # row P of the copy ends P / 2 columns into the second tile
             bytes(rng.choice(list(b"ACGT"), M).astype(np.uint8))]
    return reads, bytes(y)


@pytest.mark.parametrize("rng_", RANGES, ids=lambda p: "%d_%d" % p)
@pytest.mark.parametrize("R", LOW)
def test_low_step_tile_keys_and_values(pgs, R, rng_):
    lo, hi = rng_
    P = LANES * R
    match, mismatch, gap = SCORING
    reads, y = _batch(R, lo, hi)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_rowp_step", R)
        ctx.set_option("chunk", CHUNK)
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        got = ctx.score_ranges([(lo, hi)], semantics=pgs.F32, match=match, mismatch=mismatch, gap=gap)[0]
        values = ctx.prefix_values()
        path, kernel = " ".join(ctx.last_path()), ctx.last_kernel()
    finally:
        ctx.close()
    assert "prefix[SL=2,R=%d,P=%d,fold=rowP,step=1]" % (R, P) in path, path
    assert kernel["lanes"] == LANES and kernel["rows_per_lane"] == R and kernel["chunk_len"] == CHUNK and kernel["sub_len"] == SUB, kernel
    assert kernel["cells"] == len(reads) * P * (hi - lo), kernel["cells"]
    assert "row P folded every step" in kernel["name"], kernel["name"]
    # the warm-up of a prefix pass is L1's margin for P rows in whole 64-column segments: P + ceil(3 P / 2) = 40 and 50 columns
    assert kernel["warm"] == 64, kernel["warm"]
    # the cost model's 3 R + fold + 1 + 3 ops per step with fold = 1, over two cells per register row: (3 R + 5) / (2 R)
    assert kernel["valu_ops_per_cell"] == (3.0 * R + 5.0) / (2 * R), kernel["valu_ops_per_cell"]
    assert CHUNK < hi - lo < CHUNK + 2 * SUB and (hi - lo) % SUB != 0 and len(reads) % 2 == 1
    assert values is not None and values.shape == (len(reads), 2 * CHUNK // SUB), None if values is None else values.shape
    for k, (name, x) in enumerate(zip(NAMES, reads)):
        emu = tile_values(x, y[lo:hi], R, CHUNK, kernel["warm"], match, mismatch, gap, mk=1)
        print("R=%d [%d, %d) %-24s key %g, emulated %s" % (R, lo, hi, name, got[k], emu.astype(int).tolist()))
        assert values[k].tolist() == emu.tolist(), (name, values[k].tolist(), emu.tolist())
        assert got[k] == emu.max(), (name, got[k], float(emu.max()))
    # a full prefix scores 3 P in row P and is seen as that; with the wrong letter in row P itself the best cell of row P is a gap
    # below the full row above it, or all P letters matched around one gap
    full = match * P
    assert all(got[k] == full for k in (0, 1, 2, 5)) and full - match - gap <= got[3] <= full - gap, got


def test_an_unlisted_height_is_no_hook(pgs):
    """R = 9 is compiled on no prefix tile: the option is ignored and the bucket is swept as ever."""
    reads, y = _batch(8, 0, N)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_rowp_step", 9)
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        ctx.score_ranges([(0, N)], semantics=pgs.F32, match=3.0, mismatch=-3.0, gap=2.0)
        path, values = " ".join(ctx.last_path()), ctx.prefix_values()
    finally:
        ctx.close()
    assert "prefix[" not in path and values is None, path
