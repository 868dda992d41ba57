"""Reads an intact seed must find, settled without a sweep (host_pipeline.h prefix_seeded, "settled"), on the device
with all four size gates lowered to a reference of about 1 Mi columns.  One bucket of about 1040 reads of 150 bp: planted copies with
0 .. 5 substitutions and with a single insertion or deletion, decoy reads (the seeds cluster at a lower-scoring copy while the true
copy keeps intact seeds: the answer comes from the OTHER hits' windows), reads with two exact copies (the first wins) and with three
(over the hit cap at k = 12: not settled), copies at column 0 and at the last column, reads with a foreign letter in every seed, reads
of a 40-fold repeat, random reads.  Every field equals the runs under no_seed_certify, no_prefix_seed and no_prefix and the oracle on
a dozen windows; seed_certified is what the rule gives on numpy hit counts and oracle scores; the settled reads are in no group pass;
with the new gate at its default nothing changes; and a batch settled whole launches no score kernel."""
import numpy as np
import pytest

from oracle import binding as ob

pytestmark = pytest.mark.gpu

M = 150
N = (1 << 20) + 333
HIT_CAP = 32
SMAX, GAP = 3, 2
FIELDS = ("score", "pos", "end_x", "end_y")
OLD_GATES = (("prefix_min_cols", 1), ("prefix_seed_min_cols", 1), ("prefix_thin_min_cols", 1))
GATES = OLD_GATES + (("seed_certify_min_cols", 1),)
# (substitutions, reads).  k = 12 leaves 12 seeds in a read; a substitution costs 6, so floor(d / 2) < 12 settles up to three of them
COUNTS = ((0, 220), (1, 170), (2, 150), (3, 130), (4, 90), (5, 70))
N_INS, N_DEL, N_DECOY, N_TWICE, N_THRICE, N_FOREIGN, N_REPEAT, N_RANDOM = 30, 30, 8, 12, 6, 50, 40, 40
NOTES = ("prefix_seed[", "prefix_calibrated[")


def _dna(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def _other(rng, c):
    return b"ACGT"[(b"ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]


def periodic(s):
    return any(s[:-p] == s[p:] for p in range(1, len(s) // 2 + 1))


def usable(x, k):
    return [o for o in range(0, len(x) - k + 1, k) if all(c in b"ACGT" for c in x[o:o + k]) and not periodic(x[o:o + k])]


def hit_counts(reads, y, k):
    """Occurrences in y of every read's usable seeds (k <= 15), summed per read."""
    lut = np.zeros(256, dtype=np.int64)
    for c, v in zip(b"ACGT", range(4)):
        lut[c] = v
    d = lut[np.frombuffer(y, dtype=np.uint8)]
    code = np.zeros(len(y) - k + 1, dtype=np.int64)
    for i in range(k):
        code = code * 4 + d[i:len(y) - k + 1 + i]
    codes = np.sort(code)
    out = []
    for x in reads:
        total = 0
        for o in usable(x, k):
            v = 0
            for c in x[o:o + k]:
                v = v * 4 + int(lut[c])
            total += int(np.searchsorted(codes, v, "right") - np.searchsorted(codes, v, "left"))
        out.append(total)
    return out


@pytest.fixture(scope="module")
def batch(pgs):
    rng = np.random.default_rng(9107)
    y = bytearray(_dna(rng, N))
    k = pgs.capi.seed_k(4, M, N)
    repeat = _dna(rng, M)
    spots = [20_000 + 25_013 * j for j in range(40)]
    for at in spots:
        y[at:at + M] = repeat
    taken = list(spots) + [0, N - M]

    def free_at(length=M + 1):
        while True:
            at = int(rng.integers(M, N - 2 * M))
            if all(at + length <= s or at >= s + M + 1 for s in taken):
                taken.append(at)
                return at

    # decoys: the true copy differs from the read in one letter of each of two seeds (B = 3 m - 12, ten intact seeds of twelve); a decoy
    # elsewhere differs in three letters, four apart, of ONE seed (3 m - 18, eleven intact seeds).  The cluster rule takes the decoy
    decoys = {}
    for _ in range(N_DECOY):
        t, d = free_at(), free_at()
        x = bytearray(y[t:t + M])
        for p in (5, 6 * k + 5):
            x[p] = _other(rng, x[p])
        fake = bytearray(x)
        for p in (3 * k + 1, 3 * k + 5, 3 * k + 9):
            fake[p] = _other(rng, fake[p])
        y[d:d + M] = fake
        decoys[bytes(x)] = (t, d)
    # a stretch planted twice and one planted three times: every seed hits two or three times
    twice, thrice = {}, {}
    for _ in range(N_TWICE):
        a, b = sorted((free_at(), free_at()))
        y[b:b + M] = y[a:a + M]
        twice[bytes(y[a:a + M])] = a
    for _ in range(N_THRICE):
        a, b, c = sorted((free_at(), free_at(), free_at()))
        y[b:b + M] = y[a:a + M]
        y[c:c + M] = y[a:a + M]
        thrice[bytes(y[a:a + M])] = a
    y = bytes(y)
    reads, where = [], []
    for subs, count in COUNTS:
        for _ in range(count):
            at = free_at()
            x = bytearray(y[at:at + M])
            for p in rng.choice(np.arange(10, M - 10), subs, replace=False):
                x[p] = _other(rng, x[p])
            reads.append(bytes(x)); where.append(at)
    for _ in range(N_INS):                                            # a read letter the reference lacks: 149 matches and a gap
        at = free_at()
        p = int(rng.integers(20, M - 20))
        x = y[at:at + p] + bytes([_other(rng, y[at + p])]) + y[at + p:at + M - 1]
        reads.append(x); where.append(at)
    for _ in range(N_DEL):                                            # a reference letter the read lacks
        at = free_at()
        p = int(rng.integers(20, M - 20))
        reads.append(y[at:at + p] + y[at + p + 1:at + M + 1]); where.append(at)
    reads += [y[0:M], y[N - M:N]]; where += [0, N - M]
    for x, (t, d) in decoys.items():
        reads.append(x); where.append(t)
    for x, a in list(twice.items()) + list(thrice.items()):
        reads.append(x); where.append(a)
    for _ in range(N_FOREIGN):
        at = free_at()
        x = bytearray(y[at:at + M])
        for p in range(k // 2, M, k):
            x[p] = ord("N")
        reads.append(bytes(x)); where.append(at)
    for _ in range(N_REPEAT):
        reads.append(repeat); where.append(spots[0])
    for _ in range(N_RANDOM):
        reads.append(_dna(rng, M)); where.append(-1)
    order = rng.permutation(len(reads))
    reads, where = [reads[i] for i in order], [where[i] for i in order]
    return dict(y=y, k=k, reads=reads, where=where, hits=hit_counts(reads, y, k), decoys=decoys, twice=twice, thrice=thrice, repeat=repeat, spots=spots)


def run(pgs, y, reads, gates=GATES, options=()):
    ctx = pgs.Context(0)
    try:
        for key, v in tuple(gates) + tuple(options):
            ctx.set_option(key, v)
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        res = ctx.batch_run(raw=True)
        return dict(res={f: np.array(res[f]) for f in FIELDS}, path=ctx.last_path(), counters=ctx.last_counters(), kernel=ctx.last_kernel(),
                    timings=ctx.last_timings())
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def runs(pgs, batch):
    y, reads = batch["y"], batch["reads"]
    return dict(default=run(pgs, y, reads),
                no_seed_certify=run(pgs, y, reads, options=(("no_seed_certify", 1),)),
                no_prefix_seed=run(pgs, y, reads, options=(("no_prefix_seed", 1),)),
                no_prefix=run(pgs, y, reads, options=(("no_prefix", 1),)),
                gate_left=run(pgs, y, reads, gates=OLD_GATES))


def groups_of(path):
    out = {}
    for t in path:
        if t.startswith("prefix_group[R="):
            r, n = t[len("prefix_group[R="):-1].split(",n=")
            out[int(r)] = int(n)
    return out


def certify_note(path):
    notes = [t for t in path if t.startswith("seed_certify[")]
    if not notes:
        return None
    n, w = notes[0][len("seed_certify[n="):-1].split(",windows=")
    return int(n), int(w)


def test_batch_is_what_the_rule_is_for(batch):
    k, hits, reads = batch["k"], batch["hits"], batch["reads"]
    assert 1024 <= len(reads) <= 1100 and k == 12 and M // k == 12
    by = dict(zip(reads, hits))
    assert all(by[x] == 0 for x in reads if b"N" in x)
    assert all(by[x] > HIT_CAP for x in reads if x == batch["repeat"])
    assert all(2 * len(usable(x, k)) <= by[x] <= HIT_CAP for x in batch["twice"])
    assert all(by[x] >= 3 * len(usable(x, k)) > HIT_CAP for x in batch["thrice"])          # three copies: over the cap
    y = batch["y"]
    for x, (t, d) in batch["decoys"].items():
        at_true = sum(1 for o in range(0, M - k + 1, k) if x[o:o + k] == y[t + o:t + o + k])
        at_decoy = sum(1 for o in range(0, M - k + 1, k) if x[o:o + k] == y[d + o:d + o + k])
        assert at_true == M // k - 2 and at_decoy == M // k - 1
        B = ob.align(x, y[t - 100:t + M + 100], ob.F32)["score"]
        B0 = ob.align(x, y[d - 100:d + M + 100], ob.F32)["score"]
        assert B0 == 3 * M - 18 < B == 3 * M - 12, (B0, B)


def test_fields_equal_every_other_flow_and_the_oracle(batch, runs):
    first = runs["default"]
    print(" ".join(first["path"]))
    print(first["counters"])
    assert certify_note(first["path"]) is not None, first["path"]
    for name in ("no_seed_certify", "no_prefix_seed", "no_prefix"):
        assert certify_note(runs[name]["path"]) is None and runs[name]["counters"]["seed_certified"] == 0
        for f in FIELDS:
            diff = np.flatnonzero(first["res"][f] != runs[name]["res"][f])
            assert len(diff) == 0, (name, f, diff[:8])
    y, res = batch["y"], first["res"]
    picked, per = [], {}
    for q, (x, at) in enumerate(zip(batch["reads"], batch["where"])):
        if at < 0 or b"N" in x or x == batch["repeat"] or x in batch["twice"] or x in batch["thrice"]:
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
    for q, x in enumerate(batch["reads"]):
        if x in batch["decoys"]:                                      # B at the true copy, which only the other hits' windows hold
            t, d = batch["decoys"][x]
            assert res["score"][q] == 3 * M - 12 and res["end_y"][q] == t + M and res["end_x"][q] == M, (q, res["score"][q], res["end_y"][q], t, d)
        if x in batch["twice"] or x in batch["thrice"]:               # the first of the equal copies
            a = batch["twice"].get(x, batch["thrice"].get(x))
            assert res["score"][q] == 3 * M and res["end_y"][q] == a + M, (q, res["end_y"][q], a)
        if x == batch["repeat"]:
            assert res["score"][q] == 3 * M and res["end_y"][q] == batch["spots"][0] + M
    for q in (batch["reads"].index(y[0:M]), batch["reads"].index(y[N - M:N])):
        assert res["score"][q] == 3 * M and res["end_y"][q] in (M, N)


def expected_settled(pgs, batch, scores):
    """The rule on numpy hit counts and oracle scores: B0 is the read's best score (the cluster lands on its planted copy; a chance hit
    of a random read gives a B0 far from the rule either way), for a decoy read the oracle's score around the decoy."""
    y, k = batch["y"], batch["k"]
    out = []
    for q, (x, h) in enumerate(zip(batch["reads"], batch["hits"])):
        if not 1 <= h <= HIT_CAP:
            continue
        B0 = float(scores[q])
        if x in batch["decoys"]:
            d = batch["decoys"][x][1]
            B0 = ob.align(x, y[d - 100:d + M + 100], ob.F32)["score"]
        if pgs.capi.seed_certify_ok(int(SMAX * M - B0), SMAX, GAP, len(usable(x, k))):
            out.append(q)
    return out


def test_counter_and_groups(pgs, batch, runs):
    first, without = runs["default"], runs["no_seed_certify"]
    settled = expected_settled(pgs, batch, runs["no_prefix"]["res"]["score"])
    n_easy = sum(c for s, c in COUNTS if s <= 3) + N_INS + N_DEL + 2 + N_DECOY + N_TWICE
    print(len(settled), n_easy, certify_note(first["path"]), groups_of(first["path"]), groups_of(without["path"]))
    assert len(settled) >= n_easy - 8                                 # (a periodic seed here and there lowers u)
    assert all(x not in batch["thrice"] and x != batch["repeat"] and b"N" not in x for x in (batch["reads"][q] for q in settled))
    assert first["counters"]["seed_certified"] == len(settled) == certify_note(first["path"])[0], (first["counters"], len(settled))
    assert first["counters"]["prefix_seeded"] == without["counters"]["prefix_seeded"]
    # the settled reads are in no group pass: the passes hold the others, a read of a second pass once more
    total = len(batch["reads"])
    assert sum(groups_of(first["path"]).values()) - first["counters"]["prefix_second_pass"] <= total - len(settled)
    assert sum(groups_of(without["path"]).values()) >= total - N_RANDOM - N_FOREIGN - N_REPEAT - N_THRICE
    assert first["counters"]["prefix_certified"] <= total - len(settled)


def test_gate_at_its_default_changes_nothing(runs):
    left, without = runs["gate_left"], runs["no_seed_certify"]
    assert certify_note(left["path"]) is None and left["counters"]["seed_certified"] == 0
    assert [t for t in left["path"] if not t.startswith(NOTES)] == [t for t in without["path"] if not t.startswith(NOTES)]
    for f in FIELDS:
        assert np.array_equal(left["res"][f], without["res"][f]), f
    for name in ("prefix_certified", "prefix_second_pass", "prefix_seeded", "requeried", "whole_batch_again", "candidates"):
        assert left["counters"][name] == without["counters"][name], name


def test_a_batch_settled_whole_launches_no_score_kernel(pgs, batch):
    rng = np.random.default_rng(9108)
    y = batch["y"]
    drawn = []
    for j in range(1100):
        at = int(rng.integers(M, N - 2 * M))
        x = bytearray(y[at:at + M])
        for p in rng.choice(np.arange(10, M - 10), j % 3, replace=False):
            x[p] = _other(rng, x[p])
        drawn.append(bytes(x))
    # (a draw inside the repeat or a stretch planted three times is over the hit cap: left out)
    reads = [x for x, h in zip(drawn, hit_counts(drawn, y, batch["k"])) if 1 <= h <= HIT_CAP and len(usable(x, batch["k"])) == M // batch["k"]][:1030]
    assert len(reads) == 1030
    whole = run(pgs, y, reads)
    sweep = run(pgs, y, reads, options=(("no_prefix", 1),))
    print(" ".join(whole["path"]), whole["counters"], whole["timings"], whole["kernel"])
    for f in FIELDS:
        assert np.array_equal(whole["res"][f], sweep["res"][f]), f
    assert whole["counters"]["seed_certified"] == len(reads) == certify_note(whole["path"])[0]
    assert whole["timings"]["score_launches"] == 0 and not groups_of(whole["path"])
    assert whole["counters"]["prefix_certified"] == 0 and whole["counters"]["requeried"] == 0
    # last_kernel: what a call that took no score kernel reports — the cleared record
    assert whole["kernel"]["cells"] == 0 and whole["kernel"]["name"] == "" and whole["kernel"]["rows_per_lane"] == 0
