"""The scaffold the 16-lane slot kernels share (csrc/sw_wave_common.h: stream window, step count, profile fill and row fetch, key
fold, winner reduction) at its seams, on sw_wave_kernel, sw_wave_prof_kernel, sw_wave_prof16_kernel and sw_affine_prof_kernel.
Every case: score, end cell and — where traced — pos and both alignment strings equal to the CPU oracle (tests/affine_ref.py for
the affine kernel), and the path tag of the kernel that ran, so that no case passes on another kernel.

Stream lengths sit around the window's edges: a stream of nb positions takes nb + 16 steps, so the segment boundary is at nb = 48 |
49 and 112 | 113, the prefetch boundary at 64 and 128.  The instances are reached as tests/test_gpu_round3.py and
tests/test_gpu_affine_db.py reach them: the small-alignment batch (devlist[...]), its fallbacks under no_wave_f16, no_wave_window
and no_wave_prof, and an affine call whose batch is filled to 2^18 cells per range."""
import numpy as np
import pytest

from tests import affine_ref

pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 47, 48, 49, 63, 64, 65, 112, 113, 129]
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
FIELDS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")
AFFINE = (3, -3, 5, 1)
MIN_CELLS = 1 << 18                                                  # the affine path's threshold for sw_affine_prof_kernel

# how the small-alignment batch reaches each kernel of the family: (options, tag of the launch with lanes = columns of y)
PROF16 = ((), "devlist[orient=1,R=%d,prof=1,f16=1,windows=%d,trace=%d,pieces=0]")       # sw_wave_prof16_kernel (+ windows on the f32 one)
PROF32 = (("no_wave_f16",), "devlist[orient=1,R=%d,prof=1,f16=0,windows=%d,trace=%d,pieces=0]")   # sw_wave_prof_kernel<TRACK>, <DIRS>
PROF_WHOLE = (("no_wave_window",), "devlist[orient=1,R=%d,prof=1,f16=0,windows=0,trace=%d,pieces=0]")   # sw_wave_prof_kernel<TRACK, DIRS>
WAVE = (("no_wave_prof",), "devlist[orient=%d,R=%d,prof=0,f16=0,windows=0,trace=%d,pieces=0]")   # sw_wave_kernel<ORIENT, float>


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def rand(rng, n, alpha=AA):
    return alpha[rng.integers(0, len(alpha), n)].tobytes()


def prof_R(n):
    return 9 if n <= 144 else 10 if n <= 160 else 20 if n <= 320 else 32


def wave_R(n):
    return 10 if n <= 160 else 20 if n <= 320 else 32


_expected = {}


def expected(oracle, key, xs, y):
    """The oracle's alignments of xs against y, computed once per case."""
    if key not in _expected:
        _expected[key] = [oracle.align(x, y, 0) for x in xs]
    return _expected[key]


def run(ctx, pgs, xs, y, options=(), trace=True):
    for o in options:
        ctx.set_option(o, 1)
    try:
        got = ctx.align_batch(xs, y, semantics=0, flags=0 if trace else pgs.capi.SCORE_ONLY)
        return got, ctx.last_path()
    finally:
        for o in options:
            ctx.set_option(o, None)


def check(got, exp, trace, what):
    keys = FIELDS if trace else ("score", "end_x", "end_y")
    bad = [(k, f, g[f], e[f]) for k, (g, e) in enumerate(zip(got, exp)) for f in keys if g[f] != e[f]]
    assert not bad, (what, bad[:4])


def check_prof(ctx, pgs, oracle, key, xs, y, how, trace=True):
    """xs against y (|y| <= 512, every x streams) on one of the profile kernels."""
    options, tag = how
    R = prof_R(len(y))
    windows = int(trace and how is not PROF_WHOLE)
    want = tag % ((R, int(trace)) if how is PROF_WHOLE else (R, windows, int(trace)))
    got, path = run(ctx, pgs, xs, y, options, trace)
    assert want in path, (want, path)
    check(got, expected(oracle, key, xs, y), trace, (key, options, trace))


def check_wave(ctx, pgs, oracle, key, xs, y, trace=True):
    """xs against y on sw_wave_kernel: lanes = rows of x for |x| <= |y| (ORIENT 0), columns of y for the longer ones (ORIENT 1)."""
    options, tag = WAVE
    got, path = run(ctx, pgs, xs, y, options, trace)
    n = len(y)
    if any(0 < len(x) <= min(n, 512) for x in xs):
        want = tag % (0, wave_R(max(len(x) for x in xs if len(x) <= min(n, 512))), int(trace))
        assert want in path, (want, path)
    if any(len(x) > n for x in xs):
        want = tag % (1, wave_R(n), int(trace))
        assert want in path, (want, path)
    check(got, expected(oracle, key, xs, y), trace, (key, options, trace))


def related(rng, y, m):
    """m letters that align with y: a piece of y with a few substitutions."""
    at = int(rng.integers(0, max(1, len(y))))
    s = bytearray((y * (m // max(1, len(y)) + 2))[at:at + m])
    for i in range(0, m, 11):
        s[i] = int(AA[rng.integers(0, 20)])
    return bytes(s)


# ---- stream lengths around the window's edges, slots of one wavefront differing in length -------------------------------------
def _length_batch(n, order):
    rng = np.random.default_rng(7100 + n)
    y = rand(rng, n)
    xs = [related(rng, y, m) if k % 2 else rand(rng, m) for k, m in enumerate(LENS * 3)]
    if order == "sorted":
        xs.sort(key=len)
    return xs, y


@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("how,trace", [(PROF16, True), (PROF16, False), (PROF32, True), (PROF32, False), (PROF_WHOLE, True)],
                         ids=["prof16_windows", "prof16_score", "prof_windows", "prof_score", "prof_whole"])
def test_stream_lengths_profile_kernels(ctx, pgs, oracle, how, order, trace):
    xs, y = _length_batch(144, order)
    check_prof(ctx, pgs, oracle, ("len", 144, order), xs, y, how, trace)


@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("trace", [True, False], ids=["track_dirs", "track"])
@pytest.mark.parametrize("n", [10, 150], ids=["orient1", "orient0"])
def test_stream_lengths_wave_kernel(ctx, pgs, oracle, n, order, trace):
    """sw_wave_kernel<R = 10, float>: |y| = 10 makes every x longer than 10 a stream (ORIENT 1, nb = |x|); |y| = 150 makes every x
    lanes (ORIENT 0) against a stream of 150 positions.  ORIENT 0 with the stream lengths of LENS: test_wave_kernel_orient0_streams."""
    xs, y = _length_batch(n, order)
    check_wave(ctx, pgs, oracle, ("len", n, order), xs, y, trace)


@pytest.mark.parametrize("trace", [True, False], ids=["track_dirs", "track"])
def test_wave_kernel_orient0_streams(ctx, pgs, oracle, trace):
    """ORIENT 0: the stream is y, so every length of LENS is a reference of its own; lanes hold x of up to that length."""
    for n in LENS:
        rng = np.random.default_rng(7200 + n)
        y = rand(rng, n)
        xs = [related(rng, y, m) for m in sorted({1, max(1, n // 2), n})] + [rand(rng, max(1, n - 1))]
        check_wave(ctx, pgs, oracle, ("o0", n), xs, y, trace)


# ---- slot occupancy: idle slots, a second workgroup, an odd count (prof16's high half idle), a pair across a segment boundary -----
@pytest.mark.parametrize("count", [1, 16, 17, 33])
@pytest.mark.parametrize("how", [PROF16, PROF32, PROF_WHOLE, WAVE], ids=["prof16", "prof", "prof_whole", "wave"])
def test_slot_occupancy(ctx, pgs, oracle, how, count):
    rng = np.random.default_rng(7300 + count)
    y = rand(rng, 144)
    xs = [related(rng, y, int(m)) for m in rng.integers(150, 260, count)]   # (longer than y: streams on every kernel)
    if how is WAVE:
        check_wave(ctx, pgs, oracle, ("occ", count), xs, y)
    else:
        check_prof(ctx, pgs, oracle, ("occ", count), xs, y, how)


@pytest.mark.parametrize("lens", [(48, 49), (49, 48), (112, 113), (40, 129), (64, 65)])
def test_pair_across_a_segment_boundary(ctx, pgs, oracle, lens):
    """Two problems in one slot of sw_wave_prof16_kernel whose steps end in different segments."""
    rng = np.random.default_rng(7400 + lens[0])
    y = rand(rng, 144)
    xs = [related(rng, y, m)[:m // 2] + rand(rng, m - m // 2) for m in lens]
    for how in (PROF16, PROF32):
        check_prof(ctx, pgs, oracle, ("pair", lens), xs, y, how, trace=False)
        check_prof(ctx, pgs, oracle, ("pair", lens), xs, y, how, trace=True)


# ---- lane side: 1, 16 R - 1, 16 R, 16 R + 1 (the next R) --------------------------------------------------------------------------
LANE_SIDES = [1, 143, 144, 145, 159, 160, 161, 319, 320, 321, 511, 512]


def _lane_batch(n):
    rng = np.random.default_rng(7500 + n)
    y = rand(rng, n)
    xs = [y, rand(rng, 20) + y[n // 2:] + rand(rng, 30), related(rng, y, n + 40), rand(rng, n + 7), rand(rng, 600)]
    return xs, y


@pytest.mark.parametrize("n", LANE_SIDES)
def test_lane_side_profile_kernels(ctx, pgs, oracle, n):
    xs, y = _lane_batch(n)
    for how in ((PROF16, PROF32) if n <= 160 else (PROF32,)):         # (the float16 kernel has R = 9 and 10 only)
        check_prof(ctx, pgs, oracle, ("lane", n), xs, y, how, trace=False)
    check_prof(ctx, pgs, oracle, ("lane", n), xs, y, PROF32, trace=True)


@pytest.mark.parametrize("n", LANE_SIDES)
def test_lane_side_wave_kernel(ctx, pgs, oracle, n):
    xs, y = _lane_batch(n)
    check_wave(ctx, pgs, oracle, ("lane", n), xs, y)


def _affine_run(ctx, xs, y):
    ctx.set_reference(y)
    ctx.batch_upload(xs)
    got = ctx.affine_batch_run(match=float(AFFINE[0]), mismatch=float(AFFINE[1]), gap_open=float(AFFINE[2]), gap_extend=float(AFFINE[3]))
    return got, ctx.last_path()


def _fill(rng, xs, n):
    xs = list(xs)
    rows = sum(len(x) for x in xs)
    while rows * n < MIN_CELLS:
        m = int(rng.integers(600, 1001))
        xs.append(rand(rng, m))
        rows += m
    return xs


def check_affine(ctx, key, xs, y):
    got, path = _affine_run(ctx, xs, y)
    assert "affine_prof[R=%d]" % prof_R(len(y)) in path and "affine_exact" not in path, path
    if key not in _expected:
        _expected[key] = affine_ref.locate_batch(xs, y, *AFFINE)
    es, ei, ej = _expected[key]
    bad = [(k, float(got["score"][k]), int(got["end_x"][k]), int(got["end_y"][k]), float(es[k]), int(ei[k]), int(ej[k]))
           for k in range(len(xs)) if (got["score"][k], got["end_x"][k], got["end_y"][k]) != (es[k], ei[k], ej[k])]
    assert not bad, (key, bad[:4])
    return got


@pytest.mark.parametrize("n", LANE_SIDES)
def test_lane_side_affine_kernel(ctx, n):
    xs, y = _lane_batch(n)
    rng = np.random.default_rng(7600 + n)
    check_affine(ctx, ("alane", n), _fill(rng, xs, n), y)


@pytest.mark.parametrize("order", ["sorted", "unsorted"])
def test_stream_lengths_affine_kernel(ctx, order):
    rng = np.random.default_rng(7700)
    y = rand(rng, 144)
    xs = _fill(rng, [related(rng, y, m) if k % 2 else rand(rng, m) for k, m in enumerate(LENS * 2)], 144)
    if order == "sorted":
        xs.sort(key=len)
    check_affine(ctx, ("alens", order), xs, y)


@pytest.mark.parametrize("count", [1, 16, 17, 33])
def test_slot_occupancy_affine_kernel(ctx, count):
    """Exactly `count` problems: rows enough for 2^18 cells against 144 columns without any filling."""
    rng = np.random.default_rng(7750 + count)
    y = rand(rng, 144)
    if count == 1:
        xs = [rand(rng, 1000) + y[20:120] + rand(rng, 900)]
    else:
        xs = [related(rng, y, int(m)) for m in rng.integers(130, 260, count)]
    assert len(xs) == count and sum(len(x) for x in xs) * 144 >= MIN_CELLS
    check_affine(ctx, ("aocc", count), xs, y)


# ---- the tie rule: the first maximum in column-major order ------------------------------------------------------------------------
JUNK = b"X" * 40                                                     # a letter no y here has: two copies stay two alignments


def _tie_case():
    rng = np.random.default_rng(7800)
    y = rand(rng, 150)
    motif, other = y[20:60], y[100:140]                              # 40 letters each: score 120, below the float16 key range's end
    y2 = y[:100] + motif + y[140:]                                   # the motif twice in y: columns 21 .. 60 and 101 .. 140 (other lanes)
    xs = [JUNK + motif + JUNK + motif + JUNK,                        # same columns, two rows: the earlier row
          JUNK + other + JUNK + motif + JUNK,                        # two columns, the later column at the earlier row: the earlier column
          JUNK * 5]                                                  # nothing matches: 0 at (0, 0)
    xs2 = [JUNK * 2 + motif + JUNK * 2]                              # one row, two columns: the earlier column
    return xs, y, xs2, y2


def test_tie_rule(ctx, pgs, oracle):
    xs, y, xs2, y2 = _tie_case()
    exp = expected(oracle, "tie", xs, y)
    assert (exp[0]["score"], exp[0]["end_x"], exp[0]["end_y"]) == (120.0, 80, 60)
    assert (exp[1]["score"], exp[1]["end_x"], exp[1]["end_y"]) == (120.0, 160, 60)
    assert (exp[2]["score"], exp[2]["end_x"], exp[2]["end_y"]) == (0.0, 0, 0)
    exp2 = expected(oracle, "tie2", xs2, y2)
    assert (exp2[0]["score"], exp2[0]["end_x"], exp2[0]["end_y"]) == (120.0, 120, 60)
    for trace in (False, True):
        for how in (PROF16, PROF32):
            check_prof(ctx, pgs, oracle, "tie", xs, y, how, trace)
            check_prof(ctx, pgs, oracle, "tie2", xs2, y2, how, trace)
        check_wave(ctx, pgs, oracle, "tie", xs, y, trace)            # (every x is longer than y: ORIENT 1)
        check_wave(ctx, pgs, oracle, "tie2", xs2, y2, trace)


def test_tie_rule_affine_kernel(ctx):
    xs, y, xs2, y2 = _tie_case()
    rng = np.random.default_rng(7801)
    got = check_affine(ctx, "atie", _fill(rng, xs, len(y)), y)
    assert [(float(got["score"][k]), int(got["end_x"][k]), int(got["end_y"][k])) for k in range(3)] == [(120.0, 80, 60), (120.0, 160, 60), (0.0, 0, 0)]
    got = check_affine(ctx, "atie2", _fill(rng, xs2, len(y2)), y2)
    assert (float(got["score"][0]), int(got["end_x"][0]), int(got["end_y"][0])) == (120.0, 120, 60)


# ---- resumed start: the decision pass begins at step k0 > 0, its history word comes from the stream --------------------------------
@pytest.mark.parametrize("how", [PROF16, PROF32], ids=["f16_states", "f32_states"])
def test_resumed_start(ctx, pgs, oracle, how):
    rng = np.random.default_rng(7900)
    y = rand(rng, 144)
    xs = []
    for at in (65, 96, 127, 128, 129, 200, 333):                     # argmax rows beyond 64, around the saved states' steps
        x = bytearray(rand(rng, at + 60))
        x[at:at + 24] = y[50:74]                                     # score 72: the float16 pass decides it, the walk fits its window
        xs.append(bytes(x))
    exp = expected(oracle, "resumed", xs, y)
    assert all(e["end_x"] > 64 and e["score"] >= 72 for e in exp)
    check_prof(ctx, pgs, oracle, "resumed", xs, y, how, trace=True)
    cnt = ctx.last_counters()
    assert cnt["left_window"] == 0 and cnt["beyond_f16"] == 0, cnt   # every walk stayed inside its resumed window


# ---- sw_wave_kernel's other instances: uint8 cells, decisions only, keyed tracking (windows of the score-kernel path) ------------
@pytest.mark.parametrize("sem", [0, 1], ids=["float", "u8"])
def test_wave_kernel_behind_the_score_kernel(ctx, pgs, oracle, sem):
    """Reads of 150 letters against a long reference under no_strip: the score kernel's candidates are located by sw_wave_kernel
    <ORIENT 0, TRACK> (keyed in the uint8 engine) and traced by <ORIENT 0, DIRS>, at R = 10."""
    ref = pgs.synth.dna(7950, 60_000)
    reads = [pgs.synth.read_from_ref(ref, 7951 + k, 150, sub_rate=0.03, indel_rate=0.005)[0].tobytes() for k in range(20)]
    refb = ref.tobytes()
    ctx.set_option("no_strip", 1)
    try:
        got = ctx.align_batch(reads, refb, semantics=sem)
        path = ctx.last_path()
    finally:
        ctx.set_option("no_strip", None)
    assert "wave[orient=0,R=10,track=1,dirs=0,keyed=%d,prof=0,u8=%d]" % (sem, sem) in path, path
    assert "wave[orient=0,R=10,track=0,dirs=1,keyed=0,prof=0,u8=%d]" % sem in path, path
    for k, (q, g) in enumerate(zip(reads, got)):
        e = oracle.align(q, refb, sem)
        assert all(g[f] == e[f] for f in FIELDS), (sem, k, g, e)
