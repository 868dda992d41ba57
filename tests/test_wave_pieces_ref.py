"""The conditions on the inputs of tests/test_gpu_wave_pieces.py, from the oracle alone (no GPU): the restated piece table of
tests/wave_pieces.py against hand-written pins, every case's declared condition (argmax cell, tie partners, path span, which walks
leave which window, which piece-local maxima reach 128 q), and — for the merge rule, the `own` piece rule, the `before` of whole
sequences, the window's k0 and the warm-up length — a deliberately wrong restatement that gives other expected values for at least
one case.  A GPU test built on a wrong picture of the cut fails here."""
import os
import re
import shutil

import pytest

import wave_pieces as wp
from wave_pieces import B, CKPT, GUARD

CASES = wp.all_cases()
_oracle_cache = {}


def aligned(oracle, c):
    key = repr(c)
    if key not in _oracle_cache:
        m, x, g = c.scoring
        _oracle_cache[key] = [oracle.align(s, c.y, 0, m, x, g) for s in c.xs]
    return _oracle_cache[key]


def by_name(name, ny=144, sc=wp.SCORINGS[0]):
    return next(c for c in CASES if c.name == name and c.ny == ny and c.scoring == sc)


# ---- the table against hand-written pins -------------------------------------------------------------------------------------------
def test_constants_and_margins():
    assert (B, GUARD, CKPT, wp.K["kWindowRows"]) == (1024, 32, 32, 80)
    assert wp.K["warm_gate"] == 4 and wp.K["f16_max_stream"] == 65000 and wp.K["f16_R"] == (9, 10) and wp.K["key_limit_q"] == 128
    assert [wp.prof_R(n) for n in (128, 144, 145, 160, 161, 300, 320, 321)] == [9, 9, 10, 10, 20, 20, 20, 32]
    assert (wp.cols(144, 3, 2), wp.warm_rows(144, 3, 2), wp.rounding_slack(144, 3, 2)) == (360, 448, 24)
    assert (wp.cols(128, 3, 2), wp.warm_rows(128, 3, 2), wp.rounding_slack(128, 3, 2)) == (320, 384, 0)
    assert wp.warm_rows(144, 2, 0.5) == 832 and wp.warm_rows(144, 5, 3) == 448 and wp.warm_rows(300, 5, 0.25) == 6400
    assert wp.quantum(3, -3, 2) == 1 and wp.quantum(2, -1, 0.5) == 0.5 and wp.quantum(5, -4, 0.25) == 0.25 and wp.quantum(1, -1, 1 / 3) == 0


def test_table_pins_two_cut_sequences_and_wholes():
    # ids:      0     1     2    3     4        launch order: 1 (2049), 3 (2048), 2 (1472: not above 1472), 4, 0
    t = wp.piece_table([100, 2049, 1472, 2048, 1000], 144, 3, 2)
    assert (t["warm"], t["split_above"], t["order"], t["nlong"]) == (448, 1472, [1, 3, 2, 4, 0], 2)
    assert t["pieces"] == [(0, 0, 1024), (0, 576, 1472), (0, 1600, 449), (1, 0, 1024), (1, 576, 1472)]
    assert t["pc_before"] == [0, 1024, 2496, 2945, 3969] and t["pc_first"] == [0, 3, 5]
    assert (t["piece_stream"], t["long_stream"], t["stream_all"]) == (5441, 4097, 5441 + 1472 + 1000 + 100)
    assert [(p["kk"], p["seq"], p["before"]) for p in t["problems"][5:]] == [(5, 2, 5441), (6, 4, 6913), (7, 0, 7913)]
    assert t["kk_of_seq"] == {1: [0, 1, 2], 3: [3, 4], 2: [5], 4: [6], 0: [7]}
    assert t["pairs"] == [(0, 1), (2, 3), (4, 5), (6, 7)]            # A's last piece with B's first, B's last with the longest whole
    assert [p["ckpt_row"] for p in t["problems"]] == [0, 33, 81, 96, 130, 177, 225, 257]
    assert t["tag"] == "devlist[orient=1,R=9,prof=1,f16=1,windows=1,trace=1,pieces=1]"
    assert wp.piece_table(t["lengths"], 144, 3, 2, trace=False)["tag"] == "devlist[orient=1,R=9,prof=1,f16=1,windows=0,trace=0,pieces=1]"
    assert wp.piece_table(t["lengths"], 144, 3, 2, options=("no_wave_f16",))["tag"] == "devlist[orient=1,R=9,prof=1,f16=0,windows=1,trace=1,pieces=1]"
    off = wp.piece_table(t["lengths"], 144, 3, 2, options=("no_wave_pieces",))
    assert off["tag"] == "devlist[orient=1,R=9,prof=1,f16=1,windows=1,trace=1,pieces=0]" and off["nprob"] == 5 and off["order"] == t["order"]
    assert wp.piece_table(t["lengths"], 144, 3, 2, options=("no_wave_window",))["tag"] == "devlist[orient=1,R=9,prof=1,f16=0,windows=0,trace=1,pieces=0]"


def test_table_pins_equal_lengths_and_an_odd_piece_count():
    # equal lengths: the stable sort keeps id order, the launch runs it backwards
    t = wp.piece_table([1473, 50, 1473], 144, 3, 2)
    assert t["order"] == [2, 0, 1] and t["nlong"] == 2
    assert t["pieces"] == [(0, 0, 1024), (0, 576, 897), (1, 0, 1024), (1, 576, 897)] and t["pc_before"] == [0, 1024, 1921, 2945]
    assert t["problems"][4]["before"] == 3842 and t["pairs"] == [(0, 1), (2, 3), (4, None)]
    t = wp.piece_table([4300], 160, 3, 2)                            # cols 400, warm 512, R = 10
    assert (t["warm"], t["R"]) == (512, 10)
    assert t["pieces"] == [(0, 0, 1024), (0, 512, 1536), (0, 1536, 1536), (0, 2560, 1536), (0, 3584, 716)]
    assert t["pairs"] == [(0, 1), (2, 3), (4, None)] and t["pc_before"] == [0, 1024, 2560, 4096, 5632]


def test_table_pins_other_scorings_and_gates():
    t = wp.piece_table([1857, 1856], 144, 2, 0.5, -1)
    assert (t["warm"], t["split_above"], t["nlong"], t["pieces"]) == (832, 1856, 1, [(0, 0, 1024), (0, 192, 1665)])
    assert t["problems"][2]["before"] == 2689 and t["q"] == 0.5
    t = wp.piece_table([4300, 2049], 300, 3, 2)                      # R = 20: no float16 instance, pieces on float32 cells
    assert t["tag"] == "devlist[orient=1,R=20,prof=1,f16=0,windows=1,trace=1,pieces=1]" and t["warm"] == 832
    t = wp.piece_table([4300, 2049], 300, 5, 0.25, -4)               # warm 6400 > 4 kPieceRows
    assert t["tag"] == "devlist[orient=1,R=20,prof=1,f16=0,windows=1,trace=1,pieces=0]" and t["nprob"] == 2
    assert wp.piece_table([70000, 2000], 144, 3, 2, options=("no_wave_pieces",))["f16"] == 0      # (a stream beyond 65 000 rows)
    assert wp.piece_table([70000, 2000], 144, 3, 2)["f16"] == 1                                   # ... in pieces: float16 again


# ---- every case: its declared condition, in the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_conditions(oracle, case):
    res = aligned(oracle, case)
    t = case.table()
    m, x, g = case.scoring
    assert len(case.xs) <= 41 and max(len(s) for s in case.xs) <= 4300 + 65
    for k, (r, cl) in enumerate(zip(res, case.claims)):
        what = (repr(case), k, cl)
        if "end" in cl:
            assert (r["end_x"], r["end_y"]) == cl["end"], (what, r)
        if "score" in cl:
            assert r["score"] == cl["score"], (what, r)
        if "cut" in cl:
            assert (len(t["kk_of_seq"][k]) > 1) == cl["cut"], what
        if "leaves" in cl:
            assert wp.walk_leaves_window(t, k, r) == cl["leaves"], what
        if "k0" in cl:
            assert wp.window(t, k, r["end_x"])[2] == cl["k0"], (what, wp.window(t, k, r["end_x"]))
        if "ties" in cl:                                             # both partners hold the maximum, each as the end cell of its own rows
            for i, j in cl["ties"]:
                assert oracle.score_only(case.xs[k][:i], case.y[:j], 0, m, x, g) == r["score"], (what, i, j)
        if "overlap" in cl:                                          # an own row of one piece, a warm-up row of the next
            e0, e1 = (t["problems"][t["kk_of_seq"][k][e]] for e in cl["overlap"])
            assert e0["start"] < r["end_x"] <= (cl["overlap"][0] + 1) * B and e1["start"] < r["end_x"] <= cl["overlap"][1] * B, what
        if "begins_before" in cl:
            assert r["end_x"] == cl["end_row"] and wp.path_first_cell(r)[0] <= cl["begins_before"] < r["end_x"], (what, r["end_x"])


def test_cases_stand_on_the_edges_they_name():
    for ny, sc in wp.CONFIGS:
        w = wp.warm_rows(ny, sc[0], sc[2])
        t = by_name("boundary", ny, sc).table()
        assert [len(t["kk_of_seq"][k]) for k in range(9)] == [3] * 9 and t["problems"][t["kk_of_seq"][0][2]]["rows"] == w + 1
        t = by_name("gate", ny, sc).table()
        assert [len(t["kk_of_seq"][k]) for k in range(4)] == [1, 1, 2, 2] and t["problems"][t["kk_of_seq"][2][1]]["start"] == B - w
        t = by_name("ties", ny, sc).table()
        assert t["nlong"] == 3 and all(p["kk"] >= t["nprob"] - 3 for p in t["problems"] if not p["piece"])
        c = by_name("windows", ny, sc)
        assert c.claims[0]["k0"] == w - GUARD == min(wp.window(c.table(), 0, i)[2] for i in range(B + 1, 2 * B + 1))
        assert [cl["k0"] for cl in c.claims[1:4]] == [w + 128, w + 160, w + 160]
        c = by_name("walk_lengths", ny, sc)
        assert [cl["leaves"] for cl in c.claims[:CKPT + 2]] == [n > 48 for n in range(GUARD, GUARD + CKPT + 2)]
        assert [cl.get("leaves") for cl in c.claims[CKPT + 2:]] == ([False, False, True, True] if sc[2] >= 1 else [None] * 4)
    t = wp.boundary_case(*wp.GATE_OFF).table()
    assert t["nlong"] == 0 and "pieces=0" in t["tag"]


# ---- the float16 pair ------------------------------------------------------------------------------------------------------------------
def test_f16_pairs_and_limits(oracle):
    c = by_name("f16_pair")
    t = c.table()
    P = t["problems"]
    assert [(P[a]["seq"], P[a]["rows"], P[b2]["seq"], P[b2]["rows"]) for a, b2 in t["pairs"][1:3]] == [(0, t["warm"] + 1, 1, B), (1, t["warm"] + B, 2, len(c.xs[2]))]
    res = aligned(oracle, c)
    kk, rows, k0 = wp.window(t, 1, res[1]["end_x"])
    assert kk == 3 and k0 > P[2]["rows"] + 16                        # B's window resumes from a state saved after A's stream has ended
    assert wp.window(t, 0, res[0]["end_x"])[0] == 2                  # ... and A's own argmax is in its short last piece
    c = by_name("f16_limit")
    t = c.table()
    m, x, g = c.scoring
    pmax = lambda kk: oracle.score_only(wp.piece_rows_of(t, c.xs[t["problems"][kk]["seq"]], kk), c.y, 0, m, x, g)
    for k, cl in enumerate(c.claims):
        kks = t["kk_of_seq"][k]
        assert any(pmax(kk) >= 128 for kk in kks) == cl["beyond"], (k, [pmax(kk) for kk in kks])
        if "hot_piece" in cl:
            hot = kks[cl["hot_piece"]]
            assert [pmax(kk) for kk in kks if kk != hot] == [60.0, 60.0] and pmax(hot) == cl["score"], k
            assert t["problems"][hot ^ 1]["seq"] == cl["partner_seq"], k
    assert wp.predict_counters(t, c.xs, c.y, aligned(oracle, c), pmax) == (0, 2)
    # on float32 cells every walk gets a window: 43 rows in a window of 33 + 19, 44 in one of 33 + 19, but 46 in one of 33 + 7 (+ 2 lanes)
    assert wp.predict_counters(c.table(options=("no_wave_f16",)), c.xs, c.y, aligned(oracle, c), pmax) == (1, 0)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_saved_states_have_room(case):
    """The saved states of every problem (float32 pass) and of every pair at its first problem's place, for the longer of the two
    (float16 pass), lie inside the scratch and do not overlap — whichever of the pair is the longer one."""
    for options in ((), ("no_wave_f16",), ("no_wave_pieces",)):
        t = case.table(options=options)
        rng = sorted(wp.state_ranges(t))
        for (r0, n0, who), (r1, _, _) in zip(rng, rng[1:] + [(t["ckpt_rows_total"], 0, None)]):
            assert r0 + n0 <= r1, (repr(case), options, who, r0, n0, r1)


# ---- what a wrong restatement would give ---------------------------------------------------------------------------------------------
def _piece_results(oracle, c, t, k):
    """(score, end_x, end_y) of every piece of sequence k, scored as a problem of its own, rows in the sequence's numbering."""
    m, x, g = c.scoring
    out = []
    for kk in t["kk_of_seq"][k]:
        r = oracle.align(wp.piece_rows_of(t, c.xs[k], kk), c.y, 0, m, x, g)
        out.append((r["score"], r["end_x"] + t["problems"][kk]["start"] if r["score"] > 0 else 0, r["end_y"]))
    return out


def test_merge_rule_is_pinned(oracle):
    c = by_name("ties")
    t = c.table()
    res = aligned(oracle, c)
    wrong_row_first = wrong_last = 0
    for k in range(3):
        cands = _piece_results(oracle, c, t, k)
        want = (res[k]["score"], res[k]["end_x"], res[k]["end_y"])
        assert wp.merge(cands) == want, (k, cands)
        wrong_row_first += wp.merge_row_first(cands) != want
        wrong_last += wp.merge_last_maximum(cands) != want
    assert wrong_row_first >= 1 and wrong_last >= 1
    # the copy in the overlap: two pieces report the same cell
    cands = _piece_results(oracle, c, t, 2)
    assert cands[1] == cands[2] == (res[2]["score"], res[2]["end_x"], res[2]["end_y"])


def test_own_piece_rule_is_pinned(oracle):
    c = by_name("boundary")
    t = c.table()
    res = aligned(oracle, c)
    m, x, g = c.scoring
    no_minus_one = unclamped = 0
    for k, r in enumerate(res):
        kk = wp.owner(t, k, r["end_x"])
        p = t["problems"][kk]
        # the owner's own rows hold the argmax: it lies behind the warm-up (or in piece 0) and inside the piece
        own_lo = B * (kk - t["kk_of_seq"][k][0])
        assert own_lo < r["end_x"] <= p["start"] + p["rows"] and (own_lo == 0 or r["end_x"] - p["start"] > t["warm"]), (k, kk)
        no_minus_one += wp.owner_without_minus_one(t, k, r["end_x"]) != kk
        unclamped += wp.owner_unclamped(t, k, r["end_x"]) not in t["kk_of_seq"][k]
    assert no_minus_one >= 2                                         # (the hits that end on rows b and 2 b)
    assert wp.owner_unclamped(t, 0, 2 * B + 1) == wp.owner(t, 0, 2 * B + 1)       # the clamp only matters without the - 1 ...
    assert wp.owner_without_minus_one(t, 8, 3 * B) == t["kk_of_seq"][8][2] and unclamped == 0


def test_before_of_whole_sequences_is_pinned():
    c = by_name("ties")
    t = c.table()
    wrong = wp.before_without_long_stream(t)
    assert all(wrong[p["kk"]] == p["before"] + t["long_stream"] for p in t["problems"] if not p["piece"])
    # with it, the last whole sequence's saved states would lie beyond the scratch
    last = t["problems"][-1]
    assert wp.ckpt_row(wrong[last["kk"]], last["kk"]) + wp.states_needed(last["rows"]) > t["ckpt_rows_total"]
    assert last["ckpt_row"] + wp.states_needed(last["rows"]) <= t["ckpt_rows_total"]


def test_window_k0_is_pinned(oracle):
    c = by_name("walk_lengths")
    t = c.table()
    res = aligned(oracle, c)
    flips = 0
    for k, r in enumerate(res):
        kk, rows, k0 = wp.window(t, k, r["end_x"])
        i0, j0 = wp.path_first_cell(r)
        leaves_wrong = i0 - 1 - t["problems"][kk]["start"] + (j0 - 1) // t["R"] < wp.k0_without_guard(rows)
        flips += leaves_wrong != c.claims[k]["leaves"]
    assert flips == 48 - GUARD + 1 + 2                               # (without the guard every walk of 32 .. 48 letters would leave too, and 52, 53 from lane 5)


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("long_path")], ids=repr)
def test_long_path_needs_its_rows(oracle, case):
    """Case 5: every chain spans 314 of the 319 rows L1 allows at |y| = 128 (the chain of an argmax must end above its first match: 5
    rows are the price).  The span is read from scores alone — the reference's walk is greedy by neighbour value and stops at the first
    zero neighbour, after four cells here, so the strings do not show it: the stream from the chain's first row on still has the
    maximum, one row later it has not.  The chain lies inside the piece that owns its end with at least 64 rows to spare (the code's
    kWindowGuard + kCkptEvery: see the module on why no later start of the code's piece can be shown to fail), and a piece that started
    16, 32 or 64 rows behind the chain's first row gives another score."""
    m, x, g = case.scoring
    t = case.table()
    assert wp.rounding_slack(case.ny, m, g) == 0 and case.claims[0]["span"] == 314 == wp.cols(case.ny, m, g) - 1 - 5
    res = aligned(oracle, case)
    for k, cl in enumerate(case.claims):
        xk = case.xs[k][:cl["path_end"]]                             # (the stream up to the chain's end: the chain's end is its argmax)
        full = oracle.align(xk, case.y, 0, m, x, g)
        assert (full["score"], full["end_x"], full["end_y"]) == (12.0, cl["path_end"], case.ny), (k, full)
        first = cl["path_end"] - cl["span"] + 1
        p = t["problems"][wp.owner(t, k, cl["path_end"])]
        assert p["start"] == B - t["warm"] and first - 1 - p["start"] >= GUARD + CKPT, (k, first, p)
        same = oracle.align(xk[first - 1:], case.y, 0, m, x, g)
        assert (same["score"], same["cons_x"], same["cons_y"]) == (full["score"], full["cons_x"], full["cons_y"])
        for late in (1, 16, 32, 64):
            assert oracle.score_only(xk[first - 1 + late:], case.y, 0, m, x, g) < full["score"], (k, late)
        if cl["strong"]:
            kk, rows, k0 = wp.window(t, k, res[k]["end_x"])
            # the state the window resumes from (rows k0 - 16 .. k0 - 1 of the piece) lies inside the long path's rows
            assert first - 1 - p["start"] <= k0 - 16 and k0 - 1 < cl["path_end"] - p["start"], (k, k0)


def test_warm_up_length_is_pinned(oracle):
    """A warm-up without the slope term (|y| + reach, rounded: 192 rows at |y| = 128) starts piece 1 inside every chain of case 5: the
    piece's own maximum is then lower than the sequence's for every d, while the code's piece has it."""
    for case in (c for c in CASES if c.name.startswith("long_path_d")):
        m, x, g = case.scoring
        t = case.table()
        short = wp.warm_rows_without_slope(case.ny, m, g)
        assert short == 192 and t["warm"] == 384
        for k, cl in enumerate(case.claims):
            xk = case.xs[k][:cl["path_end"]]
            assert oracle.score_only(xk[B - t["warm"]:], case.y, 0, m, x, g) == 12.0
            assert oracle.score_only(xk[B - short:], case.y, 0, m, x, g) < 12.0, (k, cl)


def test_changed_constants_re_aim_or_fail(tmp_path):
    """A copy of the headers with kPieceRows, kWindowGuard or kCkptEvery edited: the restatement follows it; with the warm-up's formula
    edited it fails."""
    names = ("sw_batch_kernels.h", "sw_wave_common.h", "sw_wave_kernel.h", "host_batch.h", "host_wave.h")

    def copy_with(name, pattern, repl):
        d = tmp_path / re.sub(r"\W", "_", pattern)[:40]
        d.mkdir()
        for n in names:
            shutil.copy(os.path.join(wp.CSRC, n), d / n)
        text = (d / name).read_text()
        new, count = re.subn(pattern, repl, text)
        assert count == 1, (name, pattern)
        (d / name).write_text(new)
        return str(d)

    k = wp.read_constants(copy_with("sw_batch_kernels.h", r"kPieceRows = 1024;", "kPieceRows = 512;"))
    assert k["kPieceRows"] == 512
    t = wp.piece_table([1200], 144, 3, 2, k=k)
    assert t["pieces"] == [(0, 0, 512), (0, 64, 960), (0, 576, 624)] and wp.owner(t, 0, 513, k) == 1
    k = wp.read_constants(copy_with("sw_batch_kernels.h", r"kWindowGuard = 32;", "kWindowGuard = 48;"))
    assert (k["kWindowGuard"], k["kWindowRows"], wp.warm_rows(128, 3, 2, k)) == (48, 96, 448)
    k = wp.read_constants(copy_with("sw_wave_common.h", r"kCkptEvery = 32;", "kCkptEvery = 16;"))
    assert (k["kCkptEvery"], wp.warm_rows(128, 3, 2, k), wp.ckpt_row(1024, 1, k)) == (16, 384, 66)
    with pytest.raises(AssertionError):
        wp.read_constants(copy_with("host_batch.h", r"kWindowGuard \+ kCkptEvery \+ 63\) / 64 \* 64", "kWindowGuard + 63) / 64 * 64"))
    with pytest.raises(AssertionError):
        wp.read_constants(copy_with("host_batch.h", r"warm <= 4 \* kPieceRows", "warm <= 4096"))
