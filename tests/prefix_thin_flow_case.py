"""Shared by tests/test_prefix_thin_ref.py and tests/test_gpu_prefix_thin_flow.py: 1040 reads of 150 bp against 60 133 columns, the
shape of tests/test_gpu_prefix_cascade.py, with planted near-copies of some reads' prefixes.

The reference is over A / C; what is planted is over G / T.  Round 1 of a pass takes B0 from the FIRST sub-chunk with the read's best
prefix value, so a read's own copy must beat its decoys there: every decoy differs from the read's prefix in one letter, and the read
differs from its own copy in two letters below row 60 (B0 = 438: thresholds 66 at P = 26, 84 at P = 32, 102 at P2 = 38).
  * `family` (a), twelve reads: their first 26 letters are the letters `stem` with one substitution each, in different rows.  Sub-chunks
    8 .. 207 each hold `stem`, 20 columns in, followed by background: row 26 reads 72 there, row 38 far less.  A family read draws a flag
    per decoy and per family copy, and keeps its own copy's sub-chunk.
  * `stays_over` (b): the same sub-chunks hold its first 45 letters with one substitution in row 10, 120 columns in.  Row 26 reads 72
    there, row 32 reads 90, row 38 reads 108: 201 flags at either height, and all of them survive.
  * two more stretches for the reads with many substitutions (c), as in tests/test_gpu_prefix_cascade.py.
Full copies lie in sub-chunks 215 .. 229, 40 columns in.  The 1040 drawn reads are copies of the reference that start 170 .. 218 columns
into a sub-chunk below 215: their first 38 letters are background and occur nowhere in front of the read's origin, and every eighth has one substitution further down (B0 = 444)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from prefix_cascade import LANES, Read, bound
from prefix_thin import thin_cap
from row_sampled_fold import SUB

M = 150
N = 60_000 + 133
COUNT = 1040
HEIGHTS = (13, 16, 19)
SCORING = (3.0, -3.0, 2.0)
QCAP = 64 + 1024 // COUNT
DECOYS = range(8, 208)
FAMILY = 12
FLIP = ord("G") ^ ord("T")


def _letters(rng, alphabet, k):
    return bytes(rng.choice(list(alphabet), k).astype(np.uint8))


def _flipped(x, rows):
    x = bytearray(x)
    for r in rows:                                                   # (1-based rows of a G / T read)
        x[r - 1] ^= FLIP
    return bytes(x)


@functools.lru_cache(maxsize=None)
def build():
    """dict(y, drawn, state (prefix_cascade.Read per drawn read), stays_over, family, stretches=[(letters, at)])."""
    rng = np.random.default_rng(3801)
    y = bytearray(_letters(rng, b"AC", N))
    stem = _letters(rng, b"GT", 26)
    copies = [_letters(rng, b"GT", M)] + [_flipped(stem, [2 + 2 * k]) + _letters(rng, b"GT", M - 26) for k in range(FAMILY)]
    for s in DECOYS:
        y[s * SUB + 20:s * SUB + 46] = stem
        y[s * SUB + 120:s * SUB + 165] = _flipped(copies[0][:45], [10])
    stretches = []
    for k, x in enumerate(copies + [_letters(rng, b"GT", M), _letters(rng, b"GT", M)]):
        at = (215 + k) * SUB + 40
        y[at:at + M] = x
        stretches.append((x, at))
    y = bytes(y)
    reads = [_flipped(x, [61 + k, 101 + k]) for k, x in enumerate(copies)]
    drawn = []
    while len(drawn) < COUNT:
        k = len(drawn)
        at = int(rng.integers(0, 215)) * SUB + int(rng.integers(170, 219))
        if y.find(y[at:at + 26]) < at:                               # (an earlier copy of the prefix: round 1 would look there)
            continue
        x = bytearray(y[at:at + M])
        if k % 8 == 7:
            x[60 + k % 50] ^= ord("A") ^ ord("C")
        drawn.append(bytes(x))
    with ThreadPoolExecutor(8) as ex:
        state = list(ex.map(lambda x: Read(x, y, SCORING, HEIGHTS), drawn))
    return dict(y=y, drawn=drawn, state=state, stays_over=reads[0], family=reads[1:], stretches=stretches[1 + FAMILY:])


def flag_counts(read):
    """{R: flags the read draws at R rows per lane on the step tiles}, for the heights whose bound its B0 exceeds."""
    B0 = read.emulate(HEIGHTS[0], 1 << 30)["B0"]
    return {R: int(np.count_nonzero(read.val[R, 1] >= B0 - SCORING[0] * (M - LANES * R)))
            for R in HEIGHTS if B0 > bound(M, R, SCORING[0], SCORING[2])}


def clear_of_the_caps(flags):
    """Is a flag count further than a factor of two from query_flag_cap and from the thin cap?  The emulation takes the range as one
    tile; on the device a flag near a tile's end may show again in the next tile's first sub-chunk, which must not move a read across
    a cap."""
    return not any(cap / 2 < flags < 2 * cap for cap in (QCAP, thin_cap(QCAP)))
