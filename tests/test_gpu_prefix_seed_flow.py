"""The seeded flow of the chained prefix filter on the device (host_pipeline.h prefix_seeded), with its size gates lowered
to a reference of about 1 Mi columns: a bucket of 1030 reads of 150 bp — planted copies with 0 .. 5 substitutions (deficits 0 .. 30),
copies with a foreign letter in every seed (no seed at all), reads of a repeat planted 40 times (every seed over the hit cap), random
reads — gives, field for field, what the probed chain (no_prefix_seed) and the full sweep (no_prefix) give, and the oracle's answer on
a dozen reads' windows.  The number of seeded reads is what a numpy count of the seeds' occurrences says; a batch whose larger half has
no seed falls back to the probed chain's path; a second call on the same context measures no background table again."""
import numpy as np
import pytest

from oracle import binding as ob

pytestmark = pytest.mark.gpu

M = 150
N = (1 << 20) + 333
HIT_CAP = 32
FIELDS = ("score", "pos", "end_x", "end_y")
GATES = (("prefix_min_cols", 1), ("prefix_seed_min_cols", 1), ("prefix_thin_min_cols", 1))
# (substitutions, reads): a substitution away from the read's ends costs 6, so the deficits are 0, 6, ..., 30.  On 1 Mi columns the
# background (tools/prefix_cascade_model.py --per-read, scaled by 1 / 48) leaves deficits up to 12 to P = 16, 18 to P = 20 and 24 - 30
# to P = 26: the middle group is the 320 reads with three substitutions, above the 256 reads a pass of its own takes (kSeedGroupMin)
COUNTS = ((0, 180), (1, 140), (2, 140), (3, 320), (4, 70), (5, 50))
N_FOREIGN, N_REPEAT, N_RANDOM, N_DECOY = 50, 40, 40, 8
NOTES = ("prefix_seed[", "prefix_seed_failed", "prefix_calibrated[")


def _dna(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def occurrences(y, k):
    """Sorted 2-bit codes of every k-mer of y (k <= 15)."""
    lut = np.zeros(256, dtype=np.int64)
    for c, v in zip(b"ACGT", range(4)):
        lut[c] = v
    d = lut[np.frombuffer(y, dtype=np.uint8)]
    code = np.zeros(len(y) - k + 1, dtype=np.int64)
    for i in range(k):
        code = code * 4 + d[i:len(y) - k + 1 + i]
    return np.sort(code), lut


def hit_counts(reads, y, k):
    """Hits of every read: occurrences in y of its seeds at offsets 0, k, 2k, ...; a seed with a letter outside ACGT has none."""
    codes, lut = occurrences(y, k)
    out = []
    for x in reads:
        total = 0
        for off in range(0, len(x) - k + 1, k):
            s = x[off:off + k]
            if any(c not in b"ACGT" for c in s) or any(s[:-p] == s[p:] for p in range(1, k // 2 + 1)):
                continue                                              # (seeds of period <= k / 2 are left out: sw_seed_kernel.h seed_periodic)
            v = 0
            for c in s:
                v = v * 4 + int(lut[c])
            total += int(np.searchsorted(codes, v, "right") - np.searchsorted(codes, v, "left"))
        out.append(total)
    return out


@pytest.fixture(scope="module")
def batch(pgs):
    rng = np.random.default_rng(8107)
    y = bytearray(_dna(rng, N))
    repeat = _dna(rng, M)
    spots = [20_000 + 25_013 * j for j in range(40)]
    for at in spots:
        y[at:at + M] = repeat
    k = pgs.capi.seed_k(4, M, N)
    reads, where = [], []
    taken = list(spots)

    def free_at():
        """A start whose 150 columns touch no copy of the repeat, no decoy and no decoy's true copy."""
        while True:
            at = int(rng.integers(0, N - M))
            if all(at + M <= s or at >= s + M for s in taken):
                return at

    # reads whose seeds cluster AWAY from their best alignment (B0 < B on a pass that runs): the true copy differs from the read in
    # three letters of three seeds, a decoy elsewhere in every second letter of one seed — more intact seeds, a lower score
    other = lambda c: b"ACGT"[(b"ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]
    decoys = []
    for _ in range(N_DECOY):
        t = free_at(); taken.append(t)
        d = free_at(); taken.append(d)
        x = bytearray(y[t:t + M])
        for p in (5, 5 * k + 5, 10 * k + 5):
            x[p] = other(x[p])
        fake = bytearray(x)
        for p in range(7 * k, 8 * k, 2):                               # (apart: a lone mismatch costs 6 whatever the letters, no gap helps)
            fake[p] = other(fake[p])
        y[d:d + M] = fake
        decoys.append((bytes(x), t, d))
    y = bytes(y)
    for subs, count in COUNTS:
        for _ in range(count):
            at = free_at()
            x = bytearray(y[at:at + M])
            for p in rng.choice(np.arange(10, M - 10), subs, replace=False):
                x[p] = b"ACGT"[(b"ACGT".index(x[p]) + 1 + int(rng.integers(0, 3))) % 4]
            reads.append(bytes(x)); where.append(at)
    for _ in range(N_FOREIGN):
        at = free_at()
        x = bytearray(y[at:at + M])
        for p in range(k // 2, M, k):
            x[p] = ord("N")
        reads.append(bytes(x)); where.append(at)
    for j in range(N_REPEAT):
        reads.append(repeat); where.append(spots[0])
    for _ in range(N_RANDOM):
        reads.append(_dna(rng, M)); where.append(-1)
    for x, t, d in decoys:
        reads.append(x); where.append(t)
    order = rng.permutation(len(reads))
    reads, where = [reads[i] for i in order], [where[i] for i in order]
    hits = hit_counts(reads, y, k)
    return dict(y=y, k=k, reads=reads, where=where, hits=hits, spots=spots, repeat=repeat, decoys={x: (t, d) for x, t, d in decoys})


def run(pgs, y, reads, options=(), calls=1):
    ctx = pgs.Context(0)
    try:
        for key, v in GATES + tuple(options):
            ctx.set_option(key, v)
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        out = []
        for _ in range(calls):
            res = ctx.batch_run(raw=True)
            out.append(dict(res={f: np.array(res[f]) for f in FIELDS}, path=ctx.last_path(), counters=ctx.last_counters(), kernel=ctx.last_kernel()))
        return out
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def runs(pgs, batch):
    seeded = run(pgs, batch["y"], batch["reads"], calls=2)
    chain = run(pgs, batch["y"], batch["reads"], (("no_prefix_seed", 1),))[0]
    sweep = run(pgs, batch["y"], batch["reads"], (("no_prefix", 1),))[0]
    return seeded, chain, sweep


def test_batch_is_what_the_flow_is_for(batch):
    assert 1024 <= len(batch["reads"]) <= 1100 and batch["k"] >= 4 and M // batch["k"] >= 4
    hits = batch["hits"]
    foreign = [h for x, h in zip(batch["reads"], hits) if b"N" in x]
    repeats = [h for x, h in zip(batch["reads"], hits) if x == batch["repeat"]]
    assert len(foreign) == N_FOREIGN and all(h == 0 for h in foreign)                      # no seed at all
    assert len(repeats) == N_REPEAT and all(h >= 40 * (M // batch["k"]) > HIT_CAP for h in repeats)   # over the hit cap
    # every planted read with up to five substitutions keeps an intact seed, and stays within the cap
    planted = [h for x, h, at in zip(batch["reads"], hits, batch["where"]) if at >= 0 and b"N" not in x and x != batch["repeat"]]
    assert len(planted) == sum(c for _, c in COUNTS) + N_DECOY and all(1 <= h <= HIT_CAP for h in planted)
    # the decoy reads: more intact seeds at the decoy than at the true copy, and the oracle scores the decoy lower but above the
    # bound of every height, 3 (m - 16): the cluster rule takes the decoy, B0 < B, and a pass still takes the read
    k, per = batch["k"], M // batch["k"]
    assert len(batch["decoys"]) == N_DECOY
    for x, (t, d) in batch["decoys"].items():
        y = batch["y"]
        at_true = sum(1 for o in range(0, per * k, k) if x[o:o + k] == y[t + o:t + o + k])
        at_decoy = sum(1 for o in range(0, per * k, k) if x[o:o + k] == y[d + o:d + o + k])
        assert at_true == per - 3 and at_decoy == per - 1
        B = ob.align(x, y[t - 100:t + M + 100], ob.F32)["score"]
        B0 = ob.align(x, y[d - 100:d + M + 100], ob.F32)["score"]
        print("decoy read: true copy at %d scores %g, decoy at %d scores %g" % (t, B, d, B0))
        assert 3 * (M - 16) < 3 * M - 6 * ((k + 1) // 2) <= B0 < B == 3 * M - 18, (B0, B)     # (letters that match by chance may add a little)


def test_fields_equal_the_chain_the_sweep_and_the_oracle(batch, runs):
    seeded, chain, sweep = runs
    path = " ".join(seeded[0]["path"])
    print(path)
    print(seeded[0]["counters"])
    assert "prefix_group[" in path and "prefix_seed[k=%d," % batch["k"] in path, path
    assert "prefix_group[" not in " ".join(chain["path"]) and "prefix[" not in " ".join(sweep["path"])
    for other, name in ((chain, "no_prefix_seed"), (sweep, "no_prefix"), (seeded[1], "second call")):
        for f in FIELDS:
            assert np.array_equal(seeded[0]["res"][f], other["res"][f]), (name, f, np.flatnonzero(seeded[0]["res"][f] != other["res"][f])[:8])
    # the oracle on the window of a dozen reads: two of every deficit (their planted copy is their best alignment)
    y, res = batch["y"], seeded[0]["res"]
    picked, per = [], {}
    for q, (x, at) in enumerate(zip(batch["reads"], batch["where"])):
        if at < 0 or b"N" in x or x == batch["repeat"]:
            continue
        d = int(3 * M - res["score"][q])
        if per.setdefault(d, 0) < 2:
            per[d] += 1
            picked.append(q)
    assert len(picked) >= 12, per
    for q in picked:
        lo, hi = max(0, batch["where"][q] - 400), min(N, batch["where"][q] + M + 400)
        exp = ob.align(batch["reads"][q], y[lo:hi], ob.F32)
        assert res["score"][q] == exp["score"] and res["end_x"][q] == exp["end_x"] and res["end_y"][q] == exp["end_y"] + lo, (q, exp)
    # the decoy reads (B0 < B): the result is B at the true copy, not the decoy's
    for q, x in enumerate(batch["reads"]):
        if x in batch["decoys"]:
            t, d = batch["decoys"][x]
            assert res["score"][q] == 3 * M - 18 and res["end_y"][q] == t + M and res["end_x"][q] == M, (q, res["score"][q], res["end_y"][q], t, d)
    # the repeat's reads: the first of forty equal copies
    for q, x in enumerate(batch["reads"]):
        if x == batch["repeat"]:
            assert res["score"][q] == 3 * M and res["end_y"][q] == batch["spots"][0] + M, (q, res["end_y"][q])


def test_counters_and_groups(batch, runs):
    seeded, chain, sweep = runs
    first, second = seeded
    expected = sum(1 for h in batch["hits"] if 1 <= h <= HIT_CAP)
    assert first["counters"]["prefix_seeded"] == expected == second["counters"]["prefix_seeded"], (first["counters"], expected)
    assert first["counters"]["prefix_seed_hits"] == sum(batch["hits"])
    groups = {}
    for t in first["path"]:
        if t.startswith("prefix_group[R="):
            r, n = t[len("prefix_group[R="):-1].split(",n=")
            groups[int(r)] = int(n)
    print(groups)
    assert len(groups) >= 3 and min(groups) in (8, 10), groups         # passes at three heights or more, the lowest on a low tile
    # the reads without a seed ride at the chain's lowest height, R = 13 (or with the next taller group, if theirs is a small one)
    assert sum(n for r, n in groups.items() if r >= 13) >= N_FOREIGN + N_REPEAT, groups
    # the background table is measured in the first call alone
    assert first["counters"]["prefix_calibrated"] == 1 and any(t.startswith("prefix_calibrated[") for t in first["path"])
    assert second["counters"]["prefix_calibrated"] == 0 and not any(t.startswith("prefix_calibrated[") for t in second["path"])
    assert [t for t in second["path"] if not t.startswith("prefix_seed[")] == [t for t in first["path"] if not t.startswith(NOTES)]
    assert first["counters"]["prefix_certified"] >= sum(c for _, c in COUNTS[:4])


def test_a_mostly_seedless_batch_takes_the_chain(pgs, batch):
    rng = np.random.default_rng(8108)
    y, k = batch["y"], batch["k"]
    reads = []
    for j in range(1030):
        at = int(rng.integers(0, N - M))
        x = bytearray(y[at:at + M])
        if j % 5 != 0:                                                # four of five: a foreign letter in every seed
            for p in range(k // 2, M, k):
                x[p] = ord("N")
        reads.append(bytes(x))
    seeded = run(pgs, y, reads)[0]
    chain = run(pgs, y, reads, (("no_prefix_seed", 1),))[0]
    assert "prefix_seed_failed" in seeded["path"] and seeded["counters"]["prefix_seeded"] == 0, seeded["path"]
    assert [t for t in seeded["path"] if not t.startswith(NOTES)] == chain["path"], (seeded["path"], chain["path"])
    for f in FIELDS:
        assert np.array_equal(seeded["res"][f], chain["res"][f]), f
    for name in ("prefix_certified", "prefix_second_pass", "requeried", "whole_batch_again", "candidates"):
        assert seeded["counters"][name] == chain["counters"][name], name
