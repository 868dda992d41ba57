"""Inputs and bookkeeping of tests/test_gpu_big_batch.py: BIG batches of small alignments — enough items that the per-item host
loops behind the kernels (csrc/host_batch.h, host_wave.h, host_pipeline.h, all through parallel_for of csrc/host_common.h) leave
the calling thread for the worker pool — with every field of every item against the oracle.

Small per item, large in count.  y is a protein string of 40 letters over 12 letters of the alphabet; D = 2048 dictionary entries x
of 0 to 64 letters in four classes BY INDEX (d mod 4), all from fixed seeds:

  d mod 4 == 0   empty            not in the launch at all: the defaults of the result arrays must stand
  d mod 4 == 1   foreign          1..64 letters drawn from the 8 letters y does not use: every cell is 0, score 0, no traceback
  d mod 4 == 2   planted          a piece of y (16..26 letters; every 8th the whole of y) with substitutions, one inserted and one deleted
                                  letter, between foreign flanks: a traced hit whose strings hold gaps
  d mod 4 == 3   random           1..64 letters over all 20, at least one of them a letter of y: a traced hit, usually short

(25 % each; the non-empty entries are pairwise distinct.)  A batch of N items is the dictionary indexed by the fixed sequence
seq(k) = (A k + B) mod 2048 with A odd, so the oracle runs 2048 times and not N times, and — A being a unit mod 4 — ANY four
consecutive items of a batch hold all four classes: whichever contiguous part of a batch a host loop loses, it loses items of every
class.

Every checked call is preceded, on the same context, by a call on the batch prev(k) = seq(k + STRIDE).  A * STRIDE = 2 mod 4, so the
class of prev(k) is the class of seq(k) plus two: empty <-> planted, foreign <-> random.  The result arrays live on the context
across calls, so an item that a loop skips keeps what the preceding call left at its index — by construction a traced hit where the
checked batch expects nothing, and nothing where it expects a hit: a skipped item cannot look right by being stale.
tests/test_big_batch_ref.py asserts all of this with the oracle alone."""
import numpy as np

AA = b"ACDEFGHIKLMNPQRSTVWY"
Y_LETTERS = np.frombuffer(AA[:12], dtype=np.uint8)
FOREIGN_LETTERS = np.frombuffer(AA[12:], dtype=np.uint8)
ALL_LETTERS = np.frombuffer(AA, dtype=np.uint8)

D = 2048
YLEN = 40
MAXLEN = 64
CLASSES = ("empty", "foreign", "planted", "random")                  # class of entry d: CLASSES[d % 4]
A, B, STRIDE = 1237, 11, 1026
assert A % 2 == 1 and (A * STRIDE) % 4 == 2

KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
ROUTES = ("objects", "view", "score_view")                           # align_batch; batch_run(raw=True) + consensus(k); ... flags=SCORE_ONLY

DEFAULT_SC = (3.0, -3.0, 2.0)
NON_DYADIC_SC = (0.7, -0.3, 0.1)                                     # (tests/stress_small_batches.py SC) no common power of two: sw_wave_kernel
BEYOND_SC = (5.0, -4.0, 3.0)                                         # (same list) quantum 1: the packed float16 pass decides maxima below 128 only
BEYOND_FROM = 128.0

# configuration -> (options, scoring, patterns every one of which must match the call's path, patterns none of which may)
CONFIGS = {
    "default": ((), DEFAULT_SC, (r"devlist\[", r"devlist_results\[by_id=1\]"), ()),
    "scatter": (("no_devlist_by_id",), DEFAULT_SC, (r"devlist\[", r"devlist_results\[by_id=0\]"), ()),
    "hostlist": (("no_devlist",), DEFAULT_SC, (r"wave\[",), (r"devlist",)),
    "nowindow": (("no_wave_window",), DEFAULT_SC, (r"devlist\[[^\]]*windows=0", r"devlist_results\[by_id=1\]"), (r"devlist\[[^\]]*windows=1",)),
    "f32": (("no_wave_f16",), DEFAULT_SC, (r"devlist\[[^\]]*f16=0", r"devlist_results\[by_id=1\]"), (r"devlist\[[^\]]*f16=1",)),
    # (without the profile kernel x of up to |y| letters take the lanes and longer ones stream: two launches, neither holds the whole batch)
    "nondyadic": ((), NON_DYADIC_SC, (r"devlist\[orient=0[^\]]*prof=0", r"devlist\[orient=1[^\]]*prof=0", r"devlist_results\[by_id=0\]"), (r"devlist\[[^\]]*prof=1",)),
    "beyond": ((), BEYOND_SC, (r"devlist\[[^\]]*f16=1", r"devlist_results\[by_id=1\]"), ()),
}

# (MI355_SW_POOL_THREADS or None, N, configurations): the variable is read once per process, so each row is run in fresh processes
ALL = tuple(CONFIGS)
PLAN = (
    (None, 49151, ("default",)),                                     # one below the threshold: every loop on the calling thread
    (None, 49153, ALL),                                              # one above (and no multiple of host_batch.h's 256-item tile)
    ("1", 3001, ("default",)),                                       # serial by request
    ("3", 1025, ("default",)), ("3", 3001, ("default",)),
    ("8", 1025, ("default",)), ("8", 3001, ("default",)),
    ("16", 1025, ("default",)), ("16", 3001, ALL),
    ("64", 1025, ("default",)), ("64", 3001, ("default",)),
)
SIZES = tuple(sorted({n for _, n, _ in PLAN}))


def expect_pooled(value, n):
    """Whether the host loops of a call on n items take the pool (csrc/host_common.h parallel_for)."""
    return n >= 49152 if value is None else (int(value) > 1 and n >= 1024)


def _draw(rng, letters, n):
    return letters[rng.integers(0, len(letters), size=n)].tobytes()


def make_y():
    rng = np.random.default_rng(20261)
    y = bytearray(_draw(rng, Y_LETTERS, YLEN))
    y[:len(Y_LETTERS)] = Y_LETTERS.tobytes()                         # (every one of its 12 letters does occur)
    return bytes(y)


def _planted(rng, y, whole):
    """flank + mutated piece of y + flank, at most MAXLEN letters: substitutions by foreign letters, one letter inserted, one deleted
    — each at least 4 letters inside the piece and apart from each other, so that matches on both sides bridge the gap."""
    ln = YLEN if whole else int(rng.integers(16, 27))
    at = int(rng.integers(0, YLEN - ln + 1))
    piece = bytearray(y[at:at + ln])
    ins = int(rng.integers(4, ln // 2 - 2))                          # in front of piece[ins]
    dele = int(rng.integers(ln // 2 + 2, ln - 4))                    # piece[dele] goes
    for _ in range(int(rng.integers(0, 3))):
        s = int(rng.integers(0, ln))
        if min(abs(s - ins), abs(s - ins + 1), abs(s - dele)) >= 3:
            piece[s] = int(FOREIGN_LETTERS[rng.integers(0, len(FOREIGN_LETTERS))])
    out = piece[:ins] + _draw(rng, FOREIGN_LETTERS, 1) + piece[ins:dele] + piece[dele + 1:]
    room = MAXLEN - len(out)
    left = int(rng.integers(0, room // 2 + 1))
    right = int(rng.integers(0, room - left + 1))
    return _draw(rng, FOREIGN_LETTERS, left) + bytes(out) + _draw(rng, FOREIGN_LETTERS, right)


def make_dictionary(y=None):
    """The D entries (bytes), class by index."""
    y = make_y() if y is None else y
    rng = np.random.default_rng(20262)
    yset = set(y)
    edge = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64]                    # lengths every class with a free length takes first
    seen, out, taken = set(), [], {c: 0 for c in CLASSES}
    for d in range(D):
        c = CLASSES[d % 4]
        j = taken[c]
        taken[c] += 1
        if c == "empty":
            out.append(b"")
            continue
        while True:
            if c == "foreign":
                m = edge[j] if j < len(edge) else int(rng.integers(2, MAXLEN + 1))   # (only 8 one-letter strings exist: one is enough)
                x = _draw(rng, FOREIGN_LETTERS, m)
            elif c == "planted":
                x = _planted(rng, y, whole=j % 8 == 0)
            else:
                m = edge[j] if j < len(edge) else int(rng.integers(1, MAXLEN + 1))
                x = _draw(rng, ALL_LETTERS, m)
                if not yset & set(x):
                    continue
            if x not in seen:
                break
        seen.add(x)
        out.append(x)
    return out


def seq(n, shift=0):
    """Dictionary index of every item of a batch of n: the checked batch (shift 0), the one that precedes it (shift STRIDE)."""
    k = np.arange(n, dtype=np.int64) + shift
    return (A * k + B) % D


def batch(dictionary, n, shift=0):
    return [dictionary[d] for d in seq(n, shift)]


def oracle_records(ob, dictionary, y, sc):
    """The oracle's record of every dictionary entry under scoring sc = (match, mismatch, gap): a list of dicts over KEYS."""
    return [{k: r[k] for k in KEYS} for r in (ob.align(x, y, 0, *sc) for x in dictionary)]


def parts(n, nparts):
    """The contiguous parts [k0, k1) a loop over n items is cut into as nparts parts of ceil(n / nparts) items (the empty ones left out)."""
    step = (n + nparts - 1) // nparts
    return [(t * step, min(n, (t + 1) * step)) for t in range(nparts) if t * step < n]
