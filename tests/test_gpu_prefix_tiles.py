"""Prefix tiles of sw_score_kernel (SL = 2 lanes x R rows: the first P = 2 R rows of longer reads) on the device.

Option prefix_tiles makes score_ranges sweep a bucket of the prefix shape with its prefix instance, so the raw maxima are the sampled
keys of the TRUNCATED reads.  They are compared, exactly, with the numpy emulation of what the tiles publish (tests/row_sampled_fold.py
on the oracle's cell rule): the fold takes the same cells in every tile (tile starts and warm-up are multiples of 64 columns, so the
step phase of a column is the same in every tile), the warm-up makes every own cell exact, and padding behind a tile's last column
only holds decayed copies of real cells — so the range's key is the maximum of the emulated sub-chunk values."""
import numpy as np
import pytest

from prefix_filter import LANES, prefix_values
from row_sampled_fold import SUB, slack

pytestmark = pytest.mark.gpu

R = 19
P = LANES * R


def _batch(pgs, n, seed, tile):
    rng = np.random.default_rng(seed)
    y = bytearray(pgs.synth.dna(seed, n).tobytes())

    def plant(rows, end_col, m=150):
        """A read whose first `rows` letters end at 0-based column end_col; the rest is a letter the reference does not hold."""
        x = bytes(rng.choice(list(b"ACGT"), rows).astype(np.uint8)) + b"N" * (m - rows)
        y[end_col - rows + 1:end_col + 1] = x[:rows]
        return x

    reads = [plant(R, 3 * tile + 90),                                # ends in the last row of lane 0
             plant(R + 1, 5 * tile + 131),                           # ... in the first row of lane 1
             plant(P, 7 * tile - 1),                                 # last column of a sub-chunk and of a tile
             plant(P, 7 * tile + P - 1),                             # ... its neighbour: starts in the tile's first column
             plant(P, n - 1, m=140),                                 # last column of the reference; a shorter read in the pair
             plant(P - 3, 129 * tile + 200),                         # beyond the first workgroup's 128 tiles
             bytes(y[40:40 + 150]),                                  # a whole copy at the first columns
             pgs.synth.dna(seed + 1, 150).tobytes(),                 # no hit
             plant(7, 11 * tile + 5, m=133)]                         # odd count: the last workgroup holds one read
    return reads, bytes(y)


@pytest.mark.parametrize("scoring", [(3.0, -3.0, 2.0), (5.0, -4.0, 3.0)], ids=lambda s: "%g_%g_%g" % s)
@pytest.mark.parametrize("geometry", [(40_000 + 77, None), (140_000 + 77, 1024)], ids=["tile256", "tile1024"])
def test_prefix_tile_keys(pgs, geometry, scoring):
    n, chunk = geometry
    match, mismatch, gap = scoring
    reads, y = _batch(pgs, n, 4242 + n % 1000, chunk or SUB)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_tiles")
        if chunk:
            ctx.set_option("chunk", chunk)
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        got = ctx.score_ranges([(0, n)], semantics=pgs.F32, match=match, mismatch=mismatch, gap=gap)[0]
        path = " ".join(ctx.last_path())
        kernel = ctx.last_kernel()
    finally:
        ctx.close()
    assert "prefix[SL=2,R=19,P=38]" in path, path
    assert kernel["lanes"] == LANES and kernel["rows_per_lane"] == R and kernel["chunk_len"] == (chunk or SUB), kernel
    assert n > 128 * kernel["chunk_len"], "a second workgroup must run"
    assert kernel["cells"] == sum(P * n for _ in reads), kernel["cells"]
    for k, x in enumerate(reads):
        val = prefix_values(x, y, R, match, mismatch, gap)
        print("read %d: key %g, emulated %g, exact prefix maximum within %g" % (k, got[k], val.max(), slack(R, gap)))
        assert got[k] == val.max(), (k, got[k], float(val.max()))
