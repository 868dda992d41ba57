"""Inputs whose GREEDY traceback outgrows its first decision window, and the model that says by how much (no GPU here).

Every traceback of the linear engines runs over a window that ends at the argmax and reaches budget + need(end row) columns to
the left: budget = |x| / 8 + 64, need(i) = i + ceil(i * smax / g) + 2.  An optimal path never needs the
budget; the reference's walk is greedy by neighbour value (smithwaterman.cpp:40-78) and can.  The cheap input that makes it: a
read that ends in a homopolymer run, against a reference whose run is longer,

    x = "A" * (m - 1) + "C",    y = flank + "A" * K + "C" + flank    (flanks random over G / T).

Below row m the cells over the run form a plateau H(i, j) = smax * min(i, j); the only full-score cell is (m, column of C).  From
there the walk takes one diagonal step, W = K - m + 1 steps WEST along row m - 1 (the west neighbour equals the plateau value and
beats the diagonal one), then the diagonal to row 1: the consensus is K + 1 long and pos is the first column of the run.

Model of a window with column budget b, read off the oracle's own strings: before each step of the walk

    slack = b + s * NW + (1 + s) * N - W,      s = smax / g,

with NW / N / W the diagonal / north / west steps taken so far (a diagonal or north step lowers the row, which lowers need(row) by
1 + s; a diagonal or west step uses up one column).  A negative minimum: the window cannot hold the walk.  The library's window is
at most this wide (it takes min(warm, need)), so a negative value makes a retry certain; the model leaves the + 2 / ceil terms
out, so cases are only CLASSIFIED by it when they are at least 8 columns away from zero (tests/test_walk_window_ref.py)."""
import numpy as np

KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")

# (match, mismatch, gap) of the engines' cases
DEFAULT = (3.0, -3.0, 2.0)
GAP_ABOVE_MATCH = (1.0, -1.0, 4.0)
CHEAP_GAP = (10.0, -2.0, 1.0)
MISMATCH_ZERO = (2.0, 0.0, 1.0)


def budget(m):
    """Column budget of the first window of an m-row query (host_wave.h, host_pipeline.h, host_solo.h, host_saved.h)."""
    return m // 8 + 64


def need(i, smax, g):
    """Columns into a window from which row i is exact (L2)."""
    return i + int(np.ceil(i * smax / g)) + 2


def flank(pgs, seed, n):
    """n letters, uniform over G / T (no A, no C: nothing in a flank matches the read)."""
    if n == 0:
        return b""
    bits = (pgs.synth.splitmix64(seed, n) >> np.uint64(63)).astype(np.intp)
    return np.frombuffer(b"GT", dtype=np.uint8)[bits].tobytes()


def homopolymer_read(m, tail=b"C"):
    return b"A" * (m - len(tail)) + tail


def homopolymer_case(pgs, seed, m, K, flank_left, flank_right, tail=b"C"):
    """(x, y): the read of m rows that ends its run of A with `tail`, the reference with a run of K and the same tail between
    G / T flanks.  The run starts at 0-based column flank_left."""
    x = homopolymer_read(m, tail)
    y = flank(pgs, seed, flank_left) + b"A" * K + tail + flank(pgs, seed + 1, flank_right)
    return x, y


def walk_steps(res):
    """The walk of an alignment as a string over 'D' (diagonal, NW), 'N' (north: a letter of x against '-') and 'W' (west: a letter
    of y against '-'), in walk order — the consensus strings are stored end cell first."""
    cx, cy = res["cons_x"], res["cons_y"]
    assert len(cx) == len(cy)
    return "".join("W" if a == "-" else ("N" if b == "-" else "D") for a, b in zip(cx, cy))


def step_counts(res):
    s = walk_steps(res)
    return s.count("D"), s.count("N"), s.count("W")


def window_slack(res, b, smax, g):
    """Minimum over the cells the walk visits of b + s * NW + (1 + s) * N - W."""
    s = smax / g
    nw = n = w = 0
    low = float(b)
    for c in walk_steps(res):
        if c == "D":
            nw += 1
        elif c == "N":
            n += 1
        else:
            w += 1
        low = min(low, b + s * nw + (1.0 + s) * n - w)
    return low


def first_window_slack(res, m, smax, g):
    return window_slack(res, budget(m), smax, g)


def rounds_needed(res, m, smax, g):
    """Smallest r for which the budget after r widenings, budget * 4^r, holds the walk."""
    r = 0
    while window_slack(res, budget(m) * 4 ** r, smax, g) < 0:
        r += 1
        assert r < 16
    return r


def ordinary_read(pgs, ref, seed, length):
    """A copy of `length` letters of `ref` (uint8 array) with 1 % substitutions and no indels: (read bytes, 0-based offset)."""
    q, off = pgs.synth.read_from_ref(ref, seed, length, sub_rate=0.01, indel_rate=0.0)
    return q.tobytes(), off


def identity_lut(match, mismatch, letters=b"ACGT"):
    """256 x 256 table that IS match / mismatch on `letters` (and mismatch everywhere else)."""
    lut = np.full((256, 256), mismatch, dtype=np.float32)
    for a in letters:
        lut[a, a] = match
    return lut


# ---- the cases of tests/test_gpu_walk_window.py, classified by tests/test_walk_window_ref.py ---------------------------------
class Lone:
    """One lone read.  rounds: None = control (the oracle's walk has no west step), 0 = west steps that stay at least 8 columns
    inside the first window, r >= 1 = forcing (first-window slack <= -8, budget * 4^r the first that holds the walk),
    "edge" = within 8 columns of the first window's border (results only)."""

    def __init__(self, name, sem, scoring, m, K, rounds, fl=700, fr=900):
        self.name, self.sem, self.scoring, self.m, self.K, self.rounds, self.fl, self.fr = name, sem, scoring, m, K, rounds, fl, fr
        self.seed = 4000 + 7 * m + K

    def build(self, pgs):
        return homopolymer_case(pgs, self.seed, self.m, self.K, self.fl, self.fr)

    @property
    def forcing(self):
        return isinstance(self.rounds, int) and self.rounds >= 1

    def __repr__(self):
        return self.name


def _lone(sem, sc, m, K, rounds, **kw):
    name = "%s-%g_%g_%g-m%d-K%d" % ("u8" if sem else "f32", sc[0], sc[1], sc[2], m, K)
    return Lone(name, sem, sc, m, K, rounds, **kw)


F32, U8 = 0, 1
# budget(60) = 71 -> 284 -> 1136 -> 4544; budget(150) = 82 -> 328 -> 1312 -> 5248; budget(300) = 101 -> 404 -> 1616 -> 6464;
# W = K - m + 1 for K >= m, no west step for K < m.  At 10 / -2 / 1 need(150) is 1652 columns: a left flank of 7000 keeps the
# windows of every round off the start of the reference (a window that reaches it is not checked: CLAMPED below)
LONE = [
    _lone(F32, DEFAULT, 150, 100, None), _lone(F32, DEFAULT, 150, 400, 1), _lone(F32, DEFAULT, 150, 1000, 2), _lone(F32, DEFAULT, 150, 1500, 3),
    _lone(F32, DEFAULT, 60, 40, None), _lone(F32, DEFAULT, 60, 100, 0), _lone(F32, DEFAULT, 60, 250, 1), _lone(F32, DEFAULT, 60, 400, 2),
    _lone(F32, DEFAULT, 60, 1000, 2), _lone(F32, DEFAULT, 60, 1500, 3),
    _lone(F32, DEFAULT, 300, 100, None), _lone(F32, DEFAULT, 300, 400, "edge"), _lone(F32, DEFAULT, 300, 600, 1), _lone(F32, DEFAULT, 300, 1000, 2),
    _lone(F32, DEFAULT, 300, 1500, 2), _lone(F32, DEFAULT, 300, 2100, 3),
    _lone(F32, GAP_ABOVE_MATCH, 150, 100, None), _lone(F32, GAP_ABOVE_MATCH, 150, 400, 1), _lone(F32, GAP_ABOVE_MATCH, 150, 1500, 3),
    _lone(F32, CHEAP_GAP, 150, 100, None, fl=7000), _lone(F32, CHEAP_GAP, 150, 400, 1, fl=7000), _lone(F32, CHEAP_GAP, 150, 1000, 2, fl=7000), _lone(F32, CHEAP_GAP, 150, 1500, 3, fl=7000),
    _lone(F32, CHEAP_GAP, 150, 2000, 3, fl=7000),          # (the only run here longer than this scoring's first window, 82 + 1652 columns)
    _lone(U8, DEFAULT, 60, 40, None), _lone(U8, DEFAULT, 60, 400, 2), _lone(U8, DEFAULT, 60, 1500, 3),
    _lone(U8, GAP_ABOVE_MATCH, 150, 100, None), _lone(U8, GAP_ABOVE_MATCH, 150, 400, 1), _lone(U8, GAP_ABOVE_MATCH, 150, 1000, 2),
]

# the boundary sweep: one read, every K (the model crosses zero between K = 232 and K = 233 at 3 / -3 / 2)
SWEEP_M = 150
SWEEP_K = tuple(range(222, 246))
SWEEP_ENGINES = ((F32, DEFAULT), (U8, GAP_ABOVE_MATCH))


def sweep_case(pgs, K):
    return homopolymer_case(pgs, 5200 + K, SWEEP_M, K, 700, 900)


# Runs of one reference are told apart by their letters: run k is RUNS[k][0] * K + RUNS[k][1] between flanks over the two letters it
# does not use, and its read is RUNS[k][0] * (m - 1) + RUNS[k][1], which reaches its full score at that run alone (and, for a
# control run shorter than the read, its greatest score there: the uniform stretches hold no run of that length).
RUNS = ((b"A", b"C", b"GT"), (b"C", b"A", b"GT"), (b"T", b"G", b"AC"), (b"G", b"T", b"AC"))


def run_flank(pgs, seed, n, letters):
    bits = (pgs.synth.splitmix64(seed, n) >> np.uint64(63)).astype(np.intp)
    return np.frombuffer(letters, dtype=np.uint8)[bits].tobytes()


def run_read(m, k):
    return RUNS[k][0] * (m - 1) + RUNS[k][1]


def batch_case(pgs, seed, m, Ks, n, forcing_at, gap_cols=6000, lead=1500, trail=1500):
    """n reads against one uniform ACGT reference with one run per entry of Ks (run k in the letters of RUNS[k], framed by 200
    flank columns), the runs gap_cols apart.  forcing_at: {read index: run index, or (run index, rows)}: the read that claims
    that run (m rows unless given); every other slot holds an ordinary read of m rows (a copy of a run-free stretch with 1 %
    substitutions).  Returns (reads, reference bytes, [0-based first column of each run])."""
    assert len(Ks) <= len(RUNS)
    total = lead + sum(K + 1 + 400 for K in Ks) + gap_cols * (len(Ks) - 1) + trail
    ref = bytearray(pgs.synth.dna(seed, total).tobytes())
    at, starts, free = lead, [], [(0, lead)]
    for k, K in enumerate(Ks):
        a, c, fl = RUNS[k]
        piece = run_flank(pgs, seed + 10 + k, 200, fl) + a * K + c + run_flank(pgs, seed + 20 + k, 200, fl)
        ref[at:at + len(piece)] = piece
        starts.append(at + 200)
        at += len(piece)
        free.append((at, at + (gap_cols if k + 1 < len(Ks) else trail)))
        at += gap_cols if k + 1 < len(Ks) else trail
    assert at == total
    ref = bytes(ref)
    arr = np.frombuffer(ref, dtype=np.uint8)
    reads = []
    for i in range(n):
        if i in forcing_at:
            k, rows = forcing_at[i] if isinstance(forcing_at[i], tuple) else (forcing_at[i], m)
            reads.append(run_read(rows, k))
        else:
            lo, hi = free[i % len(free)]
            reads.append(ordinary_read(pgs, arr[lo:hi], seed + 100 + i, m)[0])
    return reads, ref, starts


# the batches of tests/test_gpu_walk_window.py: name -> (rows of an ordinary read, run lengths, reads, {index: run or (run, rows)},
# kwargs of batch_case).  Runs 0 .. 2 of the 150-row batches take 1, 2 and 3 rounds, run 3 (shorter than the read) is the control.
BATCHES = {
    "batch200": (150, (400, 1000, 1500, 100), 200, {0: 0, 1: 1, 57: 3, 100: 2, 198: 1, 199: 0}, {}),
    "batch9": (150, (400, 1000, 1500, 100), 9, {0: 0, 1: 1, 2: 3, 4: 2, 7: 1, 8: 0}, {}),
    "batch4100": (40, (400,), 4100, {0: 0, 2048: 0, 4099: 0}, dict(lead=1200, trail=1000)),
    "batch_long": (150, (1300, 2100), 7, {1: (0, 700), 5: (1, 1500)}, {}),
}
_built = {}


def batch(pgs, name):
    """(reads, reference bytes, run starts, forcing_at) of BATCHES[name], built once."""
    if name not in _built:
        m, Ks, n, forcing_at, kw = BATCHES[name]
        _built[name] = batch_case(pgs, 6100 + 37 * sorted(BATCHES).index(name), m, Ks, n, forcing_at, **kw) + (forcing_at,)
    return _built[name]


_expected = {}


def expected(oracle, key, reads, ref, sem, scoring, lut=None):
    """The oracle's answers for a batch, computed once per `key` on a few threads (equal reads once) and left unchanged."""
    if key not in _expected:
        from concurrent.futures import ThreadPoolExecutor
        uniq = sorted(set(reads))
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(lambda q: oracle.align(q, ref, sem, scoring[0], scoring[1], scoring[2], lut), uniq))
        by = dict(zip(uniq, res))
        _expected[key] = [by[q] for q in reads]
    return _expected[key]


def rounds_clamped(res, m, smax, g):
    """rounds_needed for a window that may reach the start of the range: the widening stops as soon as budget * 4^r +
    need(end row) covers every column in front of the end cell (the window is then the whole prefix: nothing to check)."""
    r = 0
    while window_slack(res, budget(m) * 4 ** r, smax, g) < 0 and budget(m) * 4 ** r + need(res["end_x"], smax, g) < res["end_y"]:
        r += 1
    return r


# ---- windows clamped by the start of the range ------------------------------------------------------------------------------------
# One read of 150 rows; the range it is aligned against BEGINS with `lead_run` letters of the run, so the walk's west steps end at
# the range's first column region and the window's left end is the range start as soon as budget + need(150) = 82 * 4^r + 377
# covers the lead_run + 1 columns in front of the end cell: at once for 400, after one widening for 600.
SPLIT_N, SPLIT_PIECES, SPLIT_RATIO = 8000, 4, 2.0
CLAMPED = {
    "lone_k400": dict(lead_run=400, widenings=0, kind="lone"),
    "lone_k600": dict(lead_run=600, widenings=1, kind="lone"),
    "split": dict(lead_run=600, widenings=1, kind="split"),       # the run straddles the cut in front of the winning piece
    "range": dict(lead_run=600, widenings=1, kind="range"),       # best_range + align_scored_range: a range that starts inside the run
}


def clamped_case(pgs, name, make_string_range=None):
    c = dict(CLAMPED[name])
    m = 150
    x = homopolymer_read(m)
    if c["kind"] == "lone":
        _, y = homopolymer_case(pgs, 7300 + c["lead_run"], m, c["lead_run"], 0, 900)
        c["range"] = (0, len(y))
    else:
        # pieces of _make_string_range(4, 150, 8000, 2.0): overlap 300, piece length 2225: [0, 2225) [1925, 4150) [3850, 6075) [5775, 8000)
        left, before = 3850, 200                                   # piece 2 starts 200 letters into the run
        K = before + c["lead_run"]
        y = flank(pgs, 7400, left - before) + b"A" * K + b"C"
        y += flank(pgs, 7401, SPLIT_N - len(y))
        c["range"] = (left, 6075) if c["kind"] == "split" else (left, SPLIT_N)
        c["ranges"] = [(0, 3000), (left, SPLIT_N)]
        c["winner"] = 2 if c["kind"] == "split" else 1
    c["x"], c["y"] = x, y
    c["range_bytes"] = y[c["range"][0]:c["range"][1]]
    c["west"] = c["lead_run"] - m + 1
    return c


# ---- long queries: (rows, run, left flank, right flank), need(m) = 2.5 m + 2 columns in front of the end cell left free of the
# reference's start.  The last one is the lone query beyond 2048 rows against the shortest range the strip-mined sweep takes
# (bucket_fast_ok, host_score.h: strips need 4096 columns): there need(2500) = 6252 exceeds the reference, the zero-border window is
# clamped at once and only the saved-state traceback's own window, end_x + budget columns, is outgrown.
LONG_LONE = [(700, 1300, 700, 900), (1500, 2100, 2500, 900), (2500, 3400, 3400, 1391), (2500, 3400, 300, 395)]


def long_lone_case(pgs, k):
    m, K, fl, fr = LONG_LONE[k]
    return homopolymer_case(pgs, 7000 + m, m, K, fl, fr)


def clear_of_start(res, m, smax, g, rounds):
    """Every window before round `rounds` ends at least 8 columns short of the start of the reference (no clamp decides)."""
    return all(budget(m) * 4 ** r + need(res["end_x"], smax, g) <= res["end_y"] - 8 for r in range(rounds))
