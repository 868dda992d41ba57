"""sw_prefix_thin_kernel through its test hook (Context.prefix_thin_items): every value of every item equals the
oracle's maximum of row P2 = 38 of x[:P2] over the item's window (tests/prefix_thin.py item_values), on a reference of 41 003 columns
(the size of tests/prefix_stage_cases.py), 3 / -3 / 2, a pass at P = 26: W12 = 30, 95 warm-up columns, three values per item."""
import numpy as np
import pytest

from prefix_thin import P2, geometry, item_values
from row_sampled_fold import SUB

pytestmark = pytest.mark.gpu

N = 41_003
P = 26
SCORING = (3.0, -3.0, 2.0)
RANGES = [(0, N), (13, N - 1), (0, N - 17)]
LO, HI = RANGES[1]                                                   # the range the planted hits are built for
S_END, S_OUT = 40, 90                                                # items whose hit ends in / one column behind the window's last column


@pytest.fixture(scope="module")
def case():
    """(reads, reference): three reads of 150 letters, one of exactly P2 + 1, one of 60; copies of the first P2 letters of reads 0 and 1
    that end in the last column of item S_END's window and one column behind item S_OUT's (range RANGES[1])."""
    rng = np.random.default_rng(4100)
    y = bytearray(rng.choice(list(b"ACGT"), N).astype(np.uint8))
    reads = [bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)) for k in (150, 150, 150, P2 + 1, 60)]
    W12 = geometry(150, P, SCORING[0], SCORING[2])["W12"]
    for x, s, beyond in ((reads[0], S_END, 0), (reads[1], S_OUT, 1)):
        end = LO + (s + 1) * SUB + W12 - 1 + beyond                  # column of the copy's last letter in the reference
        y[end - P2 + 1:end + 1] = x[:P2]
    return reads, bytes(y)


@pytest.fixture(scope="module")
def hook(pgs, case):
    reads, y = case
    ctx = pgs.Context(0)
    ctx.set_option("prefix_thin_items", 1)
    ctx.set_reference(y)
    ctx.batch_upload(reads)
    yield ctx
    ctx.close()


def _compare(hook, case, items, lo, hi, sub=SUB):
    reads, y = case
    got = hook.prefix_thin_items(items, P, lo, hi, sub_len=sub, match=SCORING[0], mismatch=SCORING[1], gap=SCORING[2])
    want = np.array([item_values(reads[q], y[lo:hi], s, P, SCORING, sub) for q, s in items], dtype=np.float32)
    assert got.shape == want.shape == (len(items), 3)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(tuple(items[k]), t, float(got[k, t]), float(want[k, t])) for k, t in bad[:8]]
    return got


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("lo,hi", RANGES)
def test_lists_of_every_length(hook, case, count, lo, hi):
    """Lists that end inside, at and behind a wavefront's 64 lanes and fill more than two; runs of two and of three queries inside one
    wavefront (the list is sorted by query, as the host's); the read of P2 + 1 rows and the one of 60 among them."""
    nsub = -(-(hi - lo) // SUB)
    rng = np.random.default_rng(count)
    items = sorted((int(q), int(s)) for q, s in zip(rng.integers(0, 5, count) if count > 1 else [3], rng.integers(0, nsub, count)))
    if count >= 63:
        per = np.bincount([q for q, _ in items[:64]], minlength=5)
        assert np.count_nonzero(per) >= 3
    _compare(hook, case, items, lo, hi)


@pytest.mark.parametrize("split,in_first", [(((0, 40), (1, 24)), 2), (((0, 20), (3, 22), (4, 22)), 3), (((2, 63), (3, 1), (4, 30)), 2)],
                         ids=["two_queries", "three_queries", "boundary_at_lane_63"])
def test_queries_that_share_a_wavefront(hook, case, split, in_first):
    """Fixed lists, sorted by query as the host's: one wavefront of exactly two queries (40 items of read 0, then 24 of read 1), one of
    exactly three (20 / 22 / 22 of read 0, the read of P2 + 1 rows and the read of 60), and one whose query changes in its last lane,
    with a third query in 30 lanes of the next.  Every lane has its own query bytes, length and sub-chunk."""
    nsub = -(-(HI - LO) // SUB)
    rng = np.random.default_rng(sum(k for _, k in split))
    items = [(q, int(s)) for q, k in split for s in sorted(rng.choice(nsub, k, replace=False))]
    assert items == sorted(items) and len({q for q, _ in items[:64]}) == in_first
    _compare(hook, case, items, LO, HI)


@pytest.mark.parametrize("lo,hi", RANGES)
def test_first_and_last_sub_chunk(hook, case, lo, hi):
    """Sub-chunk 0: the window is cut at the range's first column and value 0 (the left neighbour) stays -1.  The last sub-chunk: the
    window is cut at hi, 1 and 17 columns in front of the buffer's end, and has no column of the right neighbour."""
    last = (hi - lo - 1) // SUB
    items = [(q, s) for q in (0, 3, 4) for s in (0, 1, last - 1, last)]
    got = _compare(hook, case, items, lo, hi)
    for k, (q, s) in enumerate(items):
        assert (got[k, 0] == -1.0) == (s == 0) and (got[k, 2] == -1.0) == (s == last), (q, s, got[k])


def test_hit_in_the_windows_last_column_and_one_behind(hook, case):
    """Row P2 of read 0 reaches 3 P2 in the last column of item S_END's window: the item shows it in its right neighbour's value, and
    so does the item to its right, as its own.  Read 1's copy ends one column behind item S_OUT's window: that item stays below, the next
    sees it."""
    items = [(0, S_END), (0, S_END + 1), (1, S_OUT), (1, S_OUT + 1)]
    got = _compare(hook, case, items, LO, HI)
    top = 3.0 * P2
    assert got[0, 2] == top and got[1, 1] == top and got[0, :2].max() < top
    assert got[2].max() < top and got[3, 1] == top


@pytest.mark.parametrize("lo,hi", RANGES)
def test_quarter_sub_chunks(hook, case, lo, hi):
    """The geometry the library runs: an item of 256 columns is cut into four lanes on sub-chunks of 64 columns (kThinSplit), each with
    its own 63 columns of front, W12 behind and the warm-up.  The four quarters of the sub-chunks that hold the planted hits, the
    range's first and last quarters, and 130 more; then the quarters' values give back the whole item's."""
    nq4 = -(-(hi - lo) // 64)
    rng = np.random.default_rng(64)
    items = [(q, 4 * s + h) for q, s in ((0, S_END), (0, S_END + 1), (1, S_OUT), (1, S_OUT + 1)) for h in range(4)]
    items += [(q, s) for q in (0, 3, 4) for s in (0, 1, nq4 - 2, nq4 - 1)]
    items += sorted((int(q), int(s)) for q, s in zip(rng.integers(0, 5, 130), rng.integers(0, nq4, 130)))
    got = _compare(hook, case, items, lo, hi, sub=64)
    whole = _compare(hook, case, [(0, S_END), (1, S_OUT + 1)], lo, hi)
    for k, base in ((0, 0), (1, 12)):
        # sub-chunk t' of 64 columns lies in sub-chunk t' // 4 of 256: the quarters' maxima per whole sub-chunk are the item's values
        fold = {}
        for h in range(4):
            s4 = items[base + h][1]
            for t, v in enumerate(got[base + h]):
                if v >= 0:
                    fold[(s4 - 1 + t) // 4] = max(fold.get((s4 - 1 + t) // 4, -1.0), float(v))
        s = items[base][1] // 4
        assert [fold.get(s - 1 + t, -1.0) for t in range(3)] == [float(v) for v in whole[k]], (k, fold, whole[k])
