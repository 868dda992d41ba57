"""The warm-up of a prefix pass (host_score.h score_launch): a tile of a pass over the first P = LANES * R rows starts cols(P) =
P + ceil(P * match / gap) columns in front of its own, rounded up to whole segments of 64 — lemma L1 of DESIGN.md §3.3 on the prefix
matrix — and not the margin of the whole read (150 rows at 3 / -3 / 2: 384 columns; P = 26, 32, 38: 128).

Option prefix_rowp_step = R sweeps the bucket with the tiles that fold row P at every step and prefix_values reads back what every
tile published per sub-chunk, as in tests/test_gpu_prefix_step_tiles.py.  Here the reference is all T except for what is planted, and
the reads' prefixes hold no T, so that row P is 0 wherever nothing is planted.  The planted path is the longest whose END is what its
sub-chunk shows (_plant): h letters of the prefix, k reference columns to delete that leave a point or two of those letters, then the
other P - h letters — P + k columns.  It ends in the second tile's first own column (or six columns further in), so that tile sees
its first part only through its warm-up: the value there is match P - gap k, and match (P - h) for a tile that starts behind the
first part.

Exact comparisons: the device's values with the tile-by-tile emulation at the warm-up the launch reports; that emulation with the
one at the margin of all 150 rows (what a pass swept before); for the planted reads its value of the second tile's first sub-chunk
with the range as ONE tile (the truth); and the reported warm-up with the rule above.  Where the path is longer than a warm-up one
segment shorter — R = 19 only: 72 columns; 49 and 61 at R = 13 and 16 — the emulation at that shorter warm-up must miss the truth,
so the case would show a margin that is too short."""
import math

import numpy as np
import pytest

from prefix_cascade import LANES, tile_values
from row_sampled_fold import SEG, SUB

pytestmark = pytest.mark.gpu

M = 150
CHUNK = 1024
N = CHUNK + SUB + 77 + 17
SCORING = (3.0, -3.0, 2.0)
NAMES = ["ends_in_first_own_column", "ends_6_columns_in", "ends_in_last_column_of_tile_0", "prefix_across_the_tiles", "no_hit"]
PLANTED = (0, 1)                                                     # reads whose device values must be the truth, sub-chunk by sub-chunk


def _batch(R, lo):
    """Every read has a reference of its own (the planted paths would overlap): [(read, reference)]."""
    P = LANES * R
    match, _, gap = SCORING
    h, k = _plant(P)
    rng = np.random.default_rng(9700 + 64 * R + lo)
    out = []

    def gapped(end):
        """The prefix's first h letters, k columns of T, its other letters, the last of them in reference column `end`."""
        x = bytes(rng.choice(list(b"ACG"), P).astype(np.uint8))
        y = bytearray(b"T" * (lo + N))
        y[end + 1 - (P - h):end + 1] = x[h:]
        y[end + 1 - (P - h) - k - h:end + 1 - (P - h) - k] = x[:h]
        return x + b"N" * (M - P), bytes(y)

    for end in (lo + CHUNK, lo + CHUNK + 6, lo + CHUNK - 1):
        out.append(gapped(end))
    x = bytes(rng.choice(list(b"ACG"), P).astype(np.uint8))           # a full-score prefix, half of it on either side of the cut
    y = bytearray(b"T" * (lo + N))
    y[lo + CHUNK - P // 2:lo + CHUNK - P // 2 + P] = x
    out.append((x + b"N" * (M - P), bytes(y)))
    out.append((bytes(rng.choice(list(b"ACG"), M).astype(np.uint8)), b"T" * (lo + N)))
    return out, h, k


def _plant(P):
    """The longest planted path whose END is what its sub-chunk shows: h letters, k deleted columns, P - h letters.  The first part
    must pay for the gap (match h > gap k), and the path's last cell, match P - gap k, must beat what row P holds under the first
    part's end, match h - gap (P - h) — a cell of row P is never more than a gap per row below the cell above it."""
    match, _, gap = SCORING
    best = (0, 0)
    for h in range(1, P):
        k = int((match * h - 1) // gap)
        if match * P - gap * k > max(0.0, match * h - gap * (P - h)) and k > best[1]:
            best = (h, k)
    return best


@pytest.mark.parametrize("lo", [0, 3])
@pytest.mark.parametrize("R", [13, 16, 19])
def test_prefix_tiles_warm_up_of_P_rows(pgs, R, lo):
    P = LANES * R
    match, mismatch, gap = SCORING
    hi = lo + N
    batch, h, kdel = _batch(R, lo)
    span = P + kdel
    want_warm = -(-(P + math.ceil(P * match / gap)) // SEG) * SEG
    warm_m = -(-(M + math.ceil(M * match / gap)) // SEG) * SEG
    assert span < P + math.ceil(P * match / gap) <= want_warm < warm_m
    runs = []
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_rowp_step", R)
        ctx.set_option("chunk", CHUNK)
        for x, y in batch:
            ctx.set_reference(y)
            ctx.batch_upload([x, x, x])                             # (a bucket of at least two reads; an odd count: one half-filled register)
            got = ctx.score_ranges([(lo, hi)], semantics=pgs.F32, match=match, mismatch=mismatch, gap=gap)[0]
            runs.append((got, ctx.prefix_values(), " ".join(ctx.last_path()), ctx.last_kernel()))
    finally:
        ctx.close()
    for k, (name, (x, y)) in enumerate(zip(NAMES, batch)):
        got, values, path, kernel = runs[k]
        assert "prefix[SL=2,R=%d,P=%d,fold=rowP,step=1]" % (R, P) in path, path
        assert kernel["rows_per_lane"] == R and kernel["chunk_len"] == CHUNK and kernel["sub_len"] == SUB, kernel
        assert kernel["warm"] == want_warm, (kernel["warm"], want_warm)
        assert values is not None and values.shape == (3, 2 * CHUNK // SUB), None if values is None else values.shape
        emu = tile_values(x, y[lo:hi], R, CHUNK, kernel["warm"], match, mismatch, gap, mk=1)
        full = tile_values(x, y[lo:hi], R, CHUNK, warm_m, match, mismatch, gap, mk=1)
        truth = tile_values(x, y[lo:hi], R, 2 * CHUNK, 0, match, mismatch, gap, mk=1)
        print("R=%d lo=%d %-30s warm %d, path of %d columns: device %s, one tile %s" %
              (R, lo, name, kernel["warm"], span, values[0].astype(int).tolist(), truth.astype(int).tolist()))
        for r in range(3):
            assert values[r].tolist() == emu.tolist(), (name, r, values[r].tolist(), emu.tolist())
            assert got[r] == emu.max(), (name, r, got[r], float(emu.max()))
        assert emu.tolist() == full.tolist(), (name, emu.tolist(), full.tolist())
        if k in PLANTED:
            first = CHUNK // SUB                                     # the second tile's first sub-chunk
            assert emu[first] == truth[first], (name, emu.tolist(), truth.tolist())
            assert truth[first] == truth.max() == match * P - gap * kdel > match * (P - h), (name, truth.tolist())
            if span > want_warm - SEG:
                short = tile_values(x, y[lo:hi], R, CHUNK, want_warm - SEG, match, mismatch, gap, mk=1)
                assert short[first] == match * (P - h) < truth[first], (name, short.tolist(), truth.tolist())
        if name == "prefix_across_the_tiles":
            assert got[0] == match * P, got
