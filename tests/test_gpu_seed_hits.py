"""The seed scan of the chained prefix filter (sw_seed_kernel.h sw_seed_scan_kernel; test hook Context.seed_hits) against a numpy
brute force: every k-letter seed of every read, at the read's offsets 0, k, 2k, ..., at every position of the range where the
reference holds the same letters.  Hits are compared as sorted (start, offset) lists, start = position - offset relative to the
range; the count of a read is exact whatever the cap of 32 listed hits.

Sizes sit on the kernel's own edges: a thread owns STRETCH = 64 positions, a workgroup 256 threads = 16384 positions, and the last
position probed is n - k."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 12
STRETCH = 64                                                         # kSeedStretch
SPAN = 256 * STRETCH                                                 # one workgroup
CAP = 32                                                             # kSeedHitCap


def _dna(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(list(letters), n).astype(np.uint8))


def periodic(s):
    """seed_periodic of sw_seed_kernel.h: the seed repeats itself with a period of at most k / 2 letters; such seeds are left out."""
    return any(s[:-p] == s[p:] for p in range(1, len(s) // 2 + 1))


def brute(reads, y, lo, hi, k):
    """Per read: every hit of the range as a sorted list of (start, offset)."""
    index = {}
    for p in range(lo, hi - k + 1):
        index.setdefault(y[p:p + k], []).append(p)
    out = []
    for x in reads:
        hits = []
        for off in range(0, len(x) - k + 1, k):
            if not periodic(x[off:off + k]):
                hits += [(p - lo - off, off) for p in index.get(x[off:off + k], [])]
        out.append(sorted(hits))
    return out


def run(pgs, reads, y, lo, hi, k):
    ctx = pgs.Context(0)
    try:
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        return ctx.seed_hits(lo, hi, k)
    finally:
        ctx.close()


def check(got, want):
    used, counts, hits = got
    assert len(hits) == len(want)
    for q, (h, w) in enumerate(zip(hits, want)):
        assert int(counts[q]) == len(w), (q, int(counts[q]), len(w))
        if len(w) <= CAP:
            assert h == w, (q, h, w)
        else:
            assert len(h) == CAP and len(set(h)) == CAP and set(h) <= set(w), (q, h)


def planted(rng, n, k, places, nreads=3, per_read=4):
    """A random reference of n columns and reads whose seeds are cut from it at `places` (those that fit), the rest random."""
    y = _dna(rng, n)
    fit = list(dict.fromkeys(p for p in places if 0 <= p <= n - k))
    assert len(fit) <= nreads * per_read
    reads = []
    for r in range(nreads):
        parts = []
        for j in range(per_read):
            at = fit[r * per_read + j] if r * per_read + j < len(fit) else None
            parts.append(y[at:at + k] if at is not None else _dna(rng, k))
        reads.append(b"".join(parts) + _dna(rng, r))                 # (a tail shorter than a seed holds none)
    return reads, y


# n - K + 1 positions are probed: around one seed, one stretch, one workgroup; and some 200 k columns
SIZES = [K - 1, K, K + 1, STRETCH + K - 2, STRETCH + K - 1, STRETCH + K, SPAN + K - 2, SPAN + K - 1, SPAN + K, 200_003]


@pytest.mark.parametrize("n", SIZES)
def test_hits_equal_the_brute_force(pgs, n):
    rng = np.random.default_rng(4100 + n)
    places = [0, n - K, STRETCH - K // 2, STRETCH - 1, STRETCH, SPAN - K // 2, SPAN - 1, SPAN, n // 2, 3 * SPAN + 5 * STRETCH - 3]
    reads, y = planted(rng, max(n, 1), K, places)
    want = brute(reads, y, 0, n, K)
    got = run(pgs, reads, y, 0, n, K)
    print("n=%d hits per read %s" % (n, [len(w) for w in want]))
    if n >= K:
        assert sum(len(w) for w in want) > 0                         # (the planted seeds are there)
        assert any((0, 0) in w or any(s + o == 0 for s, o in w) for w in want)            # ... one of them at column 0
        assert any(any(s + o == n - K for s, o in w) for w in want)                        # ... and one at n - k
    else:
        assert all(len(w) == 0 for w in want)
    if n > SPAN + K:
        assert any(any(s + o < SPAN < s + o + K for s, o in w) for w in want)              # a seed across the workgroups
    if n > STRETCH + K:
        assert any(any(s + o < STRETCH < s + o + K for s, o in w) for w in want)           # a seed across two threads' stretches
    check(got, want)


def test_nothing_outside_the_range(pgs):
    rng = np.random.default_rng(4201)
    n, lo, hi = 5000, 1237, 4321
    assert lo % 4 != 0
    y = _dna(rng, n)
    cut = lambda at: y[at:at + K]
    # read 0: seeds at lo, at hi - k, and inside; read 1: seeds across lo, across hi, and before / behind the range (not reported)
    reads = [cut(lo) + cut(hi - K) + cut(2000) + cut(3000), cut(lo - 5) + cut(hi - K + 1) + cut(100) + cut(hi + 40)]
    want = brute(reads, y, lo, hi, K)
    whole = brute(reads, y, 0, n, K)
    assert [len(w) for w in want][0] >= 4 and len(whole[1]) >= 4 and len(want[1]) < len(whole[1])
    assert (0, 0) in want[0] and (hi - K - lo - K, K) in want[0]
    check(run(pgs, reads, y, lo, hi, K), want)


def test_same_seed_in_two_reads_and_a_seed_at_forty_places(pgs):
    rng = np.random.default_rng(4302)
    n = 40_000
    y = bytearray(_dna(rng, n))
    rep = _dna(rng, K)
    spots = [700 * (j + 1) + j for j in range(40)]
    for at in spots:
        y[at:at + K] = rep
    y = bytes(y)
    shared = y[20_000:20_000 + K]
    reads = [shared + _dna(rng, K) + y[30_000:30_000 + K] + _dna(rng, K),
             _dna(rng, K) + shared + _dna(rng, 2 * K),
             y[5:5 + K] + rep + y[39_000:39_000 + K] + _dna(rng, K),      # the repeat: 40 hits of one seed, two more seeds
             y[100:100 + 4 * K]]
    want = brute(reads, y, 0, n, K)
    assert (20_000, 0) in want[0] and (20_000 - K, K) in want[1]
    assert len(want[2]) >= 42 and sum(1 for s, o in want[2] if o == K) >= 40
    assert len(want[3]) >= 4
    got = run(pgs, reads, y, 0, n, K)
    check(got, want)
    assert int(got[1][2]) == len(want[2]) > CAP                      # counted exactly beyond the cap


def test_runs_of_one_letter(pgs):
    """Seeds of period <= k / 2 are left out: a poly-A read and a microsatellite read against runs of their kind have no seed at all.
    A read that holds ONE run-like seed among others keeps the others; a seed planted at 3000 places is still counted exactly, its
    further hits held back per thread once the list is full."""
    rng = np.random.default_rng(4350)
    n = 100_000
    y = bytearray(_dna(rng, n))
    for j in range(30):
        y[3000 * j + 500:3000 * j + 800] = b"A" * 300
        y[3000 * j + 1500:3000 * j + 1900] = b"ACG" * 133 + b"A"
    many = _dna(rng, K)
    assert not periodic(many)
    for j in range(3000):
        y[30 * j + 7:30 * j + 7 + K] = many                           # (over the runs too: what matters is what y holds in the end)
    y = bytes(y)
    reads = [b"A" * (4 * K), b"ACG" * (4 * K // 3), y[95_011:95_011 + K] + b"A" * K + y[95_100:95_100 + 2 * K], many + y[99_000:99_000 + 3 * K]]
    assert periodic(b"A" * K) and periodic((b"ACG" * K)[:K]) and periodic((b"ACGT" * K)[1:K + 1]) and not periodic(b"AAAAAACAAAAA")
    want = brute(reads, y, 0, n, K)
    assert want[0] == [] and want[1] == [] and all(o != K for _, o in want[2]) and len(want[2]) >= 3
    assert sum(1 for _, o in want[3] if o == 0) >= 2900 and len(want[3]) > 90 * CAP      # 3000 places: far over the list's 32
    got = run(pgs, reads, y, 0, n, K)
    check(got, want)


def test_256_letters_and_the_k_rule(pgs):
    rng = np.random.default_rng(4403)
    n, m = 20_000, 48
    y = bytes(rng.integers(0, 256, n, dtype=np.uint8))
    assert len(set(y)) == 256
    reads = [y[at:at + m] for at in (0, 7777, n - m)] + [bytes(rng.integers(0, 256, m, dtype=np.uint8))]
    k = pgs.capi.seed_k(256, m, n)
    assert k == 3                                                     # 256^3 >= 16 * 20 000 > 256^2
    got = run(pgs, reads, y, 0, n, 0)
    assert got[0] == k
    want = brute(reads, y, 0, n, k)
    assert all(len(w) >= m // k for w in want[:3])
    check(got, want)


def test_a_batch_of_4096_seeds(pgs):
    rng = np.random.default_rng(4504)
    n, per_read, nreads = 200_000, 8, 512
    y = _dna(rng, n)
    reads = []
    for r in range(nreads):
        at = int(rng.integers(0, n - per_read * K))
        x = bytearray(y[at:at + per_read * K])
        if r % 3 == 0:
            x[int(rng.integers(0, len(x)))] = ord("N")                 # a letter the reference does not hold: that seed is left out
        reads.append(bytes(x))
    want = brute(reads, y, 0, n, K)
    assert sum(1 for w in want if len(w) >= per_read - 1) == nreads
    check(run(pgs, reads, y, 0, n, K), want)
