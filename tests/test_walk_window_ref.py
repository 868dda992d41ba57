"""The conditions on the inputs of tests/test_gpu_walk_window.py, from the oracle alone (no GPU): every case gets its class —
forcing (the first traceback window cannot hold the greedy walk, and how many widenings it takes) or control — from the oracle's own
consensus strings and the window model of tests/walk_window_cases.py.  A GPU test built on a wrong picture of the walk fails here."""
import numpy as np
import pytest

import walk_window_cases as wc


def _align(oracle, x, y, sem, sc, lut=None):
    return oracle.align(x, y, sem, sc[0], sc[1], sc[2], lut)


def _classify(res, m, sc, rounds, what):
    """rounds as walk_window_cases.Lone: None control, 0 inside, r >= 1 forcing, "edge" unclassified, "some" forcing without a pinned count."""
    smax, g = sc[0], sc[2]
    slack = wc.first_window_slack(res, m, smax, g)
    nw, n, w = wc.step_counts(res)
    if rounds is None:
        assert w == 0 and slack == wc.budget(m), (what, (nw, n, w), slack)
    elif rounds == "edge":
        assert w > 0 and abs(slack) < 8, (what, w, slack)
    elif rounds == 0:
        assert w > 0 and slack >= 8, (what, w, slack)
    elif rounds == "some":                                   # forcing; the round that ends it may lie within 8 columns of a border
        assert slack <= -8 and wc.rounds_needed(res, m, smax, g) >= 1, (what, slack)
    else:
        assert slack <= -8, (what, slack)
        assert wc.rounds_needed(res, m, smax, g) == rounds, (what, wc.rounds_needed(res, m, smax, g), rounds)
        # ... and neither the last budget that fails nor the first that holds is within 8 columns of the walk's need
        assert wc.window_slack(res, wc.budget(m) * 4 ** (rounds - 1), smax, g) <= -8, what
        assert wc.window_slack(res, wc.budget(m) * 4 ** rounds, smax, g) >= 8, what
        assert wc.clear_of_start(res, m, smax, g, rounds), what           # the count is the model's, not a clamp's


def test_model_on_hand_made_strings():
    """walk_steps reads the strings end cell first; one west step costs a column, a diagonal one earns s, a north one 1 + s."""
    res = dict(cons_x="CA--AA", cons_y="CAAAA-", end_x=4, end_y=5)
    assert wc.walk_steps(res) == "DDWWDN"
    assert wc.step_counts(res) == (3, 1, 2)
    # budget 1, s = 1.5: 1 -> 2.5 -> 4 -> 3 -> 2 -> 3.5 -> 6
    assert wc.window_slack(res, 1, 3.0, 2.0) == 1.0
    assert wc.window_slack(dict(cons_x="C---", cons_y="CAAA"), 1, 3.0, 2.0) == 1 + 1.5 - 3
    assert wc.budget(150) == 82 and wc.budget(60) == 71 and wc.budget(2500) == 376
    assert wc.need(150, 3.0, 2.0) == 150 + 225 + 2 and wc.need(3, 1.0, 4.0) == 3 + 1 + 2


@pytest.mark.parametrize("case", wc.LONE, ids=repr)
def test_lone_cases_have_their_class_and_shape(pgs, oracle, case):
    x, y = case.build(pgs)
    assert len(x) == case.m and len(y) >= 1024
    res = _align(oracle, x, y, case.sem, case.scoring)
    _classify(res, case.m, case.scoring, case.rounds, case.name)
    if case.K >= case.m:                                     # the predicted shape: one diagonal step, K - m + 1 west, the diagonal
        assert len(res["cons_x"]) == case.K + 1 and res["pos"] == case.fl + 1 and res["end_x"] == case.m, res
        assert res["end_y"] == case.fl + case.K + 1
        assert wc.walk_steps(res) == "D" + "W" * (case.K - case.m + 1) + "D" * (case.m - 1)
        assert res["score"] == case.scoring[0] * case.m
    if case.sem == wc.U8:
        assert res["score"] < 255                            # below the cap: the saturated engine still sees the plateau's edge


def test_lone_cases_cover_every_round_count_per_solo_instance():
    for m in (60, 150, 300):                                 # sw_solo_kernel: R = 3 up to 192 rows, R = 5 beyond
        got = {c.rounds for c in wc.LONE if c.m == m and c.sem == wc.F32 and c.scoring == wc.DEFAULT}
        assert {None, 1, 2, 3} <= got, (m, got)
    assert {(c.sem, c.scoring) for c in wc.LONE} == {(wc.F32, wc.DEFAULT), (wc.F32, wc.GAP_ABOVE_MATCH), (wc.F32, wc.CHEAP_GAP),
                                                    (wc.U8, wc.DEFAULT), (wc.U8, wc.GAP_ABOVE_MATCH)}
    for K, r in ((100, None), (400, 1), (1000, 2), (1500, 3)):
        assert any(c.m == 150 and c.K == K and c.rounds == r and c.scoring == wc.DEFAULT and c.sem == wc.F32 for c in wc.LONE)


@pytest.mark.parametrize("sem,sc", wc.SWEEP_ENGINES, ids=("f32", "u8"))
def test_sweep_crosses_zero_exactly_once(pgs, oracle, sem, sc):
    slack = []
    for K in wc.SWEEP_K:
        x, y = wc.sweep_case(pgs, K)
        res = _align(oracle, x, y, sem, sc)
        assert len(res["cons_x"]) == K + 1 and res["pos"] == 701 and res["end_x"] == wc.SWEEP_M
        slack.append(wc.first_window_slack(res, wc.SWEEP_M, sc[0], sc[2]))
    assert wc.SWEEP_K == tuple(range(222, 246))
    assert all(a > b for a, b in zip(slack, slack[1:])), slack           # one column less per K
    assert sum(1 for a, b in zip(slack, slack[1:]) if (a >= 0) != (b >= 0)) == 1, slack
    assert slack[0] >= 8 and slack[-1] <= -8, slack                      # what the GPU test asserts at the two ends


def test_truncated_walk_cannot_pass(pgs, oracle):
    """The greedy walk over the first-round window alone — the columns [end_y - (budget + need(m)), end_y) behind a zero border —
    gives another answer than the walk over the whole matrix wherever the run is longer than that window: a library that accepted
    its first window would be caught by pos and the consensus length.  (Where the window holds the whole run the cells in it are
    exact after all — the flank in front holds zeros — and only the counter tells; every engine and scoring has a longer run.)"""
    told = set()
    for case in wc.LONE:
        if not case.forcing:
            continue
        x, y = case.build(pgs)
        sc = case.scoring
        full = _align(oracle, x, y, case.sem, sc)
        w = wc.budget(case.m) + wc.need(case.m, sc[0], sc[2])
        lo = full["end_y"] - w
        assert lo > 0, case
        part = oracle.trace_from(x, y[lo:full["end_y"]], case.sem, case.m, w, sc[0], sc[1], sc[2])
        assert part["score"] == full["score"], case                     # the end cell itself is exact in the window (L2)
        same = (part["pos"] + lo, len(part["cons_x"])) == (full["pos"], len(full["cons_x"]))
        assert same == (case.K + 1 <= w), (case, w, part["pos"] + lo, full["pos"], len(part["cons_x"]))
        if not same:
            assert part["pos"] + lo > full["pos"] and len(part["cons_x"]) < len(full["cons_x"])
            told.add((case.sem, case.scoring, case.m))
    assert {(c.sem, c.scoring, c.m) for c in wc.LONE} == told


@pytest.mark.parametrize("name", sorted(wc.BATCHES))
def test_batches_have_their_classes(pgs, oracle, name):
    reads, ref, starts, forcing_at = wc.batch(pgs, name)
    m, Ks, n, _, _ = wc.BATCHES[name]
    assert len(reads) == n and len(ref) >= 1024
    assert all(b - a - Ks[k] - 1 - 400 >= 6000 for k, (a, b) in enumerate(zip(starts, starts[1:])))    # runs at least 6000 columns apart
    scorings = [("default", wc.DEFAULT)] + ([("mismatch0", wc.MISMATCH_ZERO)] if name in ("batch9", "batch_long") else [])
    for tag, sc in scorings:
        exp = wc.expected(oracle, (name, tag), reads, ref, wc.F32, sc)
        rounds = []
        for i, q in enumerate(reads):
            res = exp[i]
            if i not in forcing_at:
                assert wc.first_window_slack(res, len(q), sc[0], sc[2]) >= 8, (name, tag, i)     # ordinary reads stay inside
                continue
            k, rows = forcing_at[i] if isinstance(forcing_at[i], tuple) else (forcing_at[i], m)
            assert len(q) == rows and res["end_x"] == rows and res["pos"] == starts[k] + 1, (name, tag, i, res["pos"], starts[k])
            if Ks[k] < rows:
                _classify(res, rows, sc, None, (name, tag, i))
            else:
                assert len(res["cons_x"]) == Ks[k] + 1
                r = wc.rounds_needed(res, rows, sc[0], sc[2])
                _classify(res, rows, sc, "some" if name == "batch_long" else r, (name, tag, i))
                assert r >= 1
                rounds.append(r)
        if name in ("batch200", "batch9"):
            assert sorted(set(rounds)) == [1, 2, 3], rounds
            assert any(Ks[forcing_at[i]] < m for i in forcing_at)                                  # the control run
        assert rounds
    if name in ("batch200", "batch9", "batch4100"):
        last = n - 1
        mid = {"batch200": 100, "batch9": 4, "batch4100": 2048}[name]
        assert {0, mid, last} <= set(forcing_at)
        if name != "batch4100":
            assert {1, last - 1} <= set(forcing_at)


def test_table_that_is_the_default_scoring_changes_nothing(pgs, oracle):
    reads, ref, _, _ = wc.batch(pgs, "batch9")
    lut = wc.identity_lut(3.0, -3.0)
    plain = wc.expected(oracle, ("batch9", "default"), reads, ref, wc.F32, wc.DEFAULT)
    table = wc.expected(oracle, ("batch9", "lut"), reads, ref, wc.F32, wc.DEFAULT, lut)
    assert table == plain


@pytest.mark.parametrize("name", sorted(wc.CLAMPED))
def test_clamped_cases(pgs, oracle, name):
    """Windows that reach the start of the range: the model says the budget fails, the clamp ends the widening."""
    c = wc.clamped_case(pgs, name)
    sc = wc.DEFAULT
    res = _align(oracle, c["x"], c["range_bytes"], wc.F32, sc)
    assert res["pos"] == 1 and res["end_x"] == len(c["x"]), res         # the walk ends at the range's first column
    assert wc.step_counts(res)[2] == c["west"]
    r = wc.rounds_clamped(res, len(c["x"]), sc[0], sc[2])
    assert r == c["widenings"], (name, r)
    assert wc.window_slack(res, wc.budget(len(c["x"])) * 4 ** r, sc[0], sc[2]) <= -8    # only the clamp lets this window pass
    # the clamp is not within 8 columns of engaging a round earlier or later
    reach = lambda k: wc.budget(len(c["x"])) * 4 ** k + wc.need(res["end_x"], sc[0], sc[2])
    assert reach(r) >= res["end_y"] + 8 and (r == 0 or reach(r - 1) <= res["end_y"] - 8)


def test_long_lone_cases(pgs, oracle):
    for k, (m, K, fl, fr) in enumerate(wc.LONG_LONE):
        x, y = wc.long_lone_case(pgs, k)
        res = _align(oracle, x, y, wc.F32, wc.DEFAULT)
        _classify(res, m, wc.DEFAULT, "some", ("long lone", m))         # (700 rows: 151 * 4 + 1.5 - 601 = 4.5, one widening or two)
        assert len(res["cons_x"]) == K + 1 and res["pos"] == fl + 1
        # the saved-state traceback's own window, [end_y - (end_x + budget), end_y) (host_saved.h), is narrower still
        assert wc.step_counts(res)[2] > wc.budget(m) + 8 and res["end_y"] - (res["end_x"] + wc.budget(m)) > 8
        # the first zero-border window stays off the start of the reference: a widening is certain ... except in the last case
        assert wc.clear_of_start(res, m, 3.0, 2.0, 1) == (k < 3)
    m, K, fl, fr = wc.LONG_LONE[-1]
    assert m > 2048 and fl + K + 1 + fr == 4096                          # the shortest range the strip-mined sweep takes
    assert wc.need(m, 3.0, 2.0) > 4096                                   # ... whose every zero-border window starts at column 0
    assert wc.LONG_LONE[2][0] == m and wc.LONG_LONE[2][1] == K
