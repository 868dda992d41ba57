"""Prefix tiles of sw_score_kernel that fold row P at EVERY step (ROWP with MK = 1; DESIGN.md §3.3 L19, row-P variant) on the device,
for R = 13, 16 and 19 rows per lane.

Option prefix_rowp_step = R makes score_ranges sweep the bucket of 150 bp reads with that instance, and prefix_values reads back what
every tile published per sub-chunk.  Both are compared, exactly, with the numpy emulation (tests/prefix_cascade.py tile_values with
mk = 1): the maximum of row P over the sub-chunk's columns, shifted by the one column that lane 1 lags lane 0, the steps of a tile's
warm-up counted for its first sub-chunk.  The range is a little over one tile of 1024 columns, so a second tile runs and its last
sub-chunk is partial; range starts are no multiples of 4 (the staging's byte shift); one read has its mismatch in row P itself."""
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


def _batch(R, lo, hi):
    P = LANES * R
    rng = np.random.default_rng(9500 + 64 * R + lo)
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
@pytest.mark.parametrize("R", [13, 16, 19])
def test_step_tile_keys_and_values(pgs, R, rng_):
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
    # the cost model's 3 R + fold + 1 + 3 ops per step with fold = 1 (one packed minimum, row P alone), over two cells per register row
    assert kernel["valu_ops_per_cell"] == (3.0 * R + 1.0 + 1 + 3.0) / (2 * R), kernel["valu_ops_per_cell"]
    assert CHUNK < hi - lo < CHUNK + 2 * SUB and (hi - lo) % SUB != 0 and len(reads) % 2 == 1
    assert values is not None and values.shape == (len(reads), 2 * CHUNK // SUB), None if values is None else values.shape
    for k, (name, x) in enumerate(zip(NAMES, reads)):
        emu = tile_values(x, y[lo:hi], R, CHUNK, kernel["warm"], match, mismatch, gap, mk=1)
        print("R=%d [%d, %d) %-24s key %g, emulated %s" % (R, lo, hi, name, got[k], emu.astype(int).tolist()))
        assert values[k].tolist() == emu.tolist(), (name, values[k].tolist(), emu.tolist())
        assert got[k] == emu.max(), (name, got[k], float(emu.max()))
    # the hand-made reads do what their names say, with no slack: a full prefix scores 3 P in row P and is seen as that; with the
    # wrong letter in row P itself the best cell of row P is a gap below the full row above it, or — where the wrong letter meets
    # the reference's next one — all P letters matched around one gap
    full = match * P
    assert all(got[k] == full for k in (0, 1, 2, 5)) and full - match - gap <= got[3] <= full - gap, got
