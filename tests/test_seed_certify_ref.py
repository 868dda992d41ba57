"""Lemma L21 (host_pipeline.h prefix_seeded, "settled") on the oracle's full matrices, no GPU: for a read with u seeds
in the table and an exact alignment score B0 of deficit d = smax m - B0 with floor(d / min(g, smax)) < u, EVERY cell with H >= B0 lies
in the end-column interval of one of the read's seed hits.  The rule, the interval and u are the library's own host functions
(sw_seed_kernel.h seed_certify_ok, seed_certify_window, seed_usable behind the C-ABI); the hit list is brute force, the matrix the
oracle's.  Every valid B0 is tried — each value of the matrix the rule admits, not only the maximum."""
import numpy as np
import pytest

from oracle import binding as ob

LETTERS = b"ACGT"
# (match, mismatch, gap): the last has g > smax, so c = smax
SCORINGS = [(3.0, -3.0, 2.0), (2.0, -1.0, 1.0), (5.0, -4.0, 3.0), (2.0, -2.0, 3.0)]
SHAPES = [(36, 4, 2500), (50, 6, 3000), (60, 5, 4100)]                  # (read letters, seed letters, reference letters)


def _dna(rng, n):
    return bytes(rng.choice(list(LETTERS), n).astype(np.uint8))


def _other(rng, c):
    return LETTERS[(LETTERS.index(c) + 1 + int(rng.integers(0, 3))) % 4]


def periodic(s):
    return any(s[:-p] == s[p:] for p in range(1, len(s) // 2 + 1))


def usable_offsets(x, k):
    """Offsets of the seeds that enter the table: every letter known to the reference, not periodic (seed_table_build)."""
    return [o for o in range(0, len(x) - k + 1, k) if all(c in LETTERS for c in x[o:o + k]) and not periodic(x[o:o + k])]


def all_hits(x, y, k):
    index = {}
    for p in range(len(y) - k + 1):
        index.setdefault(y[p:p + k], []).append(p)
    return [(p - o, o) for o in usable_offsets(x, k) for p in index.get(x[o:o + k], [])]


def plant(rng, m, k, n):
    """A reference of n letters and reads of m letters planted in it, by name."""
    y = bytearray(_dna(rng, n))
    spot = iter(range(200, n - 200, (n - 400) // 14))
    copy = lambda at, length=m: bytearray(y[at:at + length])
    reads = {}

    def sub(x, places):
        for p in places:
            x[p] = _other(rng, x[p])
        return bytes(x)

    tail = list(range((m // k) * k, m))                               # letters of no seed (none when k divides m)
    reads["exact"] = bytes(copy(next(spot)))
    reads["sub_in_a_seed"] = sub(copy(next(spot)), [k + 1])
    reads["subs_in_two_seeds"] = sub(copy(next(spot)), [1, 3 * k + 2])
    reads["two_subs_in_one_seed"] = sub(copy(next(spot)), [2 * k, 2 * k + 2])
    reads["sub_between_seeds"] = sub(copy(next(spot)), tail[:1] or [m - 1])
    at = next(spot)
    longer = copy(at, m + 1)
    reads["deletion_in_a_seed"] = bytes(longer[:k + 2] + longer[k + 3:])       # a reference letter the read lacks, inside the second seed
    shorter = copy(next(spot), m - 1)
    reads["insertion_in_a_seed"] = bytes(shorter[:2 * k + 1] + bytes([_other(rng, shorter[2 * k + 1])]) + shorter[2 * k + 1:])
    at = next(spot)
    reads["clipped_head"] = bytes(sub(copy(at), [0, 1, 2]))             # three wrong letters in front: cheaper to clip than to pay
    at = next(spot)
    reads["clipped_tail"] = bytes(sub(copy(at), [m - 3, m - 2, m - 1]))
    reads["cut_by_column_0"] = _dna(rng, 3) + bytes(y[0:m - 3])         # its first letters hang over the reference's first column
    reads["cut_by_last_column"] = bytes(y[n - (m - 3):n]) + _dna(rng, 3)
    # two copies of equal score: the same stretch twice
    a, b = next(spot), next(spot)
    y[b:b + m] = y[a:a + m]
    reads["two_equal_copies"] = bytes(y[a:a + m])
    # a copy and a worse copy elsewhere: a B0 below B that the rule may still admit
    a, b = next(spot), next(spot)
    y[b:b + m] = sub(copy(a), [k // 2])
    reads["near_copy_elsewhere"] = bytes(y[a:a + m])
    reads["random"] = _dna(rng, m)
    return bytes(y), reads


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(2107)
    return [(m, k, *plant(rng, m, k, n)) for m, k, n in SHAPES]


def check_read(pgs, name, x, y, k, scoring):
    """Every cell with H >= B0 in some hit's interval, for every B0 the rule admits.  Returns the number of B0 values tried."""
    match, mismatch, gap = scoring
    smax, g = int(match), int(gap)
    m, n = len(x), len(y)
    u = len(usable_offsets(x, k))
    assert pgs.capi.seed_usable(x, k, LETTERS) == u, (name, u)
    H = ob.fill(x, y, ob.F32, match, mismatch, gap)
    hits = all_hits(x, y, k)
    tried = 0
    for B0 in sorted({float(v) for v in np.unique(H) if v > 0}, reverse=True):
        d = int(smax * m - B0)
        ok = pgs.capi.seed_certify_ok(d, smax, g, u)
        assert ok == (d // min(g, smax) < u), (name, d, u)
        if not ok:
            break                                                     # (lower values have larger deficits)
        inside = np.zeros(n, dtype=bool)
        for start, off in hits:
            w = pgs.capi.seed_certify_window(start, m, d, smax, g, n)
            lo, hi = max(0, start + m - 1 - d // min(g, smax)), min(n - 1, start + m - 1 + d // g)
            assert w == ((lo, hi) if lo <= hi else None), (name, start, d, w)
            if w:
                inside[w[0]:w[1] + 1] = True
        rows, cols = np.nonzero(H >= B0)
        assert len(cols) > 0
        missed = [(int(i), int(j)) for i, j in zip(rows, cols) if not inside[j - 1]]
        assert not missed, (name, scoring, B0, d, u, missed[:4], sorted(hits)[:6])
        tried += 1
    return tried


@pytest.mark.parametrize("scoring", SCORINGS)
def test_every_cell_at_b0_or_above_ends_in_a_hit_window(pgs, cases, scoring):
    match, mismatch, gap = scoring
    for m, k, y, reads in cases:
        tried = {}
        for name, x in reads.items():
            assert len(x) == m
            tried[name] = check_read(pgs, name, x, y, k, scoring)
        print(scoring, m, k, tried)
        # the planted reads the rule must admit at their best score: one or two substitutions cost little against u seeds
        for name in ("exact", "sub_in_a_seed", "sub_between_seeds", "two_equal_copies", "near_copy_elsewhere", "cut_by_column_0", "cut_by_last_column"):
            assert tried[name] >= 1, (name, scoring, m, k)
        assert tried["exact"] >= 2                                    # more than one B0 for the same read: other cells' scores
        assert tried["random"] == 0                                   # no alignment of a random read comes near smax m


def test_two_equal_copies_are_both_covered(pgs, cases):
    m, k, y, reads = cases[1]
    x = reads["two_equal_copies"]
    H = ob.fill(x, y, ob.F32, 3.0, -3.0, 2.0)
    ends = sorted(int(j) - 1 for i, j in np.argwhere(H == 3.0 * m))
    assert len(ends) == 2
    starts = {s for s, o in all_hits(x, y, k)}
    for e in ends:
        assert e - m + 1 in starts and pgs.capi.seed_certify_window(e - m + 1, m, 0, 3, 2, len(y)) == (e, e)


def test_unknown_and_periodic_seeds_lower_u(pgs):
    rng = np.random.default_rng(2108)
    for k in (4, 5, 6):
        m = 10 * k + 3
        while True:
            x = bytearray(_dna(rng, m))
            if len(usable_offsets(bytes(x), k)) == 10:
                break
        assert pgs.capi.seed_usable(bytes(x), k, LETTERS) == 10
        x[3 * k + 1] = ord("N")                                        # a letter the reference does not hold
        assert pgs.capi.seed_usable(bytes(x), k, LETTERS) == 9 == len(usable_offsets(bytes(x), k))
        x[5 * k:6 * k] = (b"AC" * k)[:k]                              # period 2 <= k / 2
        assert pgs.capi.seed_usable(bytes(x), k, LETTERS) == 8 == len(usable_offsets(bytes(x), k))
        x[0:k] = b"T" * k
        assert pgs.capi.seed_usable(bytes(x), k, LETTERS) == 7
        assert pgs.capi.seed_usable(bytes(x), k, b"ACGTN") == 8           # ... unless the reference holds it
        assert pgs.capi.seed_usable(bytes(x[:k - 1]), k, LETTERS) == 0
    # with fewer seeds the same deficit is no longer admitted
    assert pgs.capi.seed_certify_ok(14, 3, 2, 8) and not pgs.capi.seed_certify_ok(14, 3, 2, 7)
    assert pgs.capi.seed_certify_ok(5, 2, 3, 3) and not pgs.capi.seed_certify_ok(6, 2, 3, 3)      # g > smax: c = smax
    assert not pgs.capi.seed_certify_ok(0, 3, 2, 0) and not pgs.capi.seed_certify_ok(-1, 3, 2, 5)


def test_options_are_on_the_abi_list(pgs):
    names = pgs.capi.option_names()
    assert "no_seed_certify" in names and "seed_certify_min_cols" in names and "seed_ride" in names


def test_window_is_clipped_to_the_range(pgs):
    w = pgs.capi.seed_certify_window
    assert w(100, 50, 0, 3, 2, 1000) == (149, 149)
    assert w(100, 50, 7, 3, 2, 1000) == (146, 152)                     # floor(7 / 2) left and right
    assert w(100, 50, 7, 2, 3, 1000) == (146, 151)                     # c = smax = 2 left, g = 3 right
    assert w(-45, 50, 6, 3, 2, 1000) == (1, 7) and w(-49, 50, 2, 3, 2, 1000) == (0, 1)
    assert w(-60, 50, 6, 3, 2, 1000) is None                           # ends in front of column 0 whatever is clipped
    assert w(953, 50, 6, 3, 2, 1000) == (999, 999) and w(954, 50, 6, 3, 2, 1000) is None
    assert w(948, 50, 6, 3, 2, 1000) == (994, 999)
