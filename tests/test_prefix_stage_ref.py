"""The cases of tests/test_gpu_prefix_stage.py on the oracle's full matrices (no GPU): the emulated key of every planted read on the
sub-reference y[lo:hi] lies within the sampling slack of the exact maximum of its first P rows there, and the planted columns do what
tests/prefix_stage_cases.py says of them — so that the device test's exact comparison is a comparison with the right thing."""
import numpy as np
import pytest

from oracle import binding as ob
from prefix_filter import prefix_values
from prefix_stage_cases import INSIDE, N, NAMES, P, PAIRS, PARTLY, R, SCORING, batch
from row_sampled_fold import SUB, slack


def _exact(x, y):
    return ob.fill(x[:P], y, ob.F32, *SCORING)


def test_pairs_cover_the_load_paths():
    assert {lo & 3 for lo, _ in PAIRS} == {0, 1, 2, 3}
    assert {lo for lo, _ in PAIRS} == {0, 1, 2, 3, 5, 13, 31, 33}
    assert {N - hi for _, hi in PAIRS if hi > PARTLY + 40} == {0, 1, 5, 17}
    # the cut at hi in every byte of a dword, and in a 16-byte vector's second, third and fourth dword
    assert {(hi - lo) & 3 for lo, hi in PAIRS} == {0, 1, 2, 3}
    assert {((hi - lo) & 15) >> 2 for lo, hi in PAIRS} >= {1, 2, 3}
    for lo, hi in PAIRS:
        assert hi - lo > 128 * SUB, "a second workgroup must run"
    assert 0 < PARTLY % SUB < SUB - P


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
def test_planted_columns(pair):
    lo, hi = pair
    match, mismatch, gap = SCORING
    reads, y = batch(lo, hi)
    assert len(reads) % 2 == 1 and len(y) == N
    sub = y[lo:hi]
    exact, key = {}, {}
    for name, x in zip(NAMES, reads):
        H = _exact(x, sub)
        exact[name] = float(H.max())
        val = prefix_values(x, sub, R, match, mismatch, gap)
        print("[%d, %d) %s: emulated key %g, exact prefix maximum %g" % (lo, hi, name, val.max(), exact[name]))
        key[name] = float(val.max())
        assert exact[name] - slack(R, gap) <= key[name] <= exact[name], (name, key[name], exact[name])
        if name == "ends_at_hi":
            assert H[P, hi - lo] == match * P == exact[name]
        if name == "starts_at_lo":
            assert H[P, P] == match * P == exact[name]
    # the straddling copy: the range holds INSIDE of its columns, the columns behind hi would score more — and a sweep that took them
    # in would publish another key
    beyond = min(P - INSIDE, N - hi)
    x = reads[NAMES.index("straddles_hi")]
    assert _exact(x, sub)[INSIDE, hi - lo] == match * INSIDE
    if beyond >= 17:
        assert float(_exact(x, y[lo:hi + beyond]).max()) == match * (INSIDE + beyond) > exact["straddles_hi"]
        assert prefix_values(x, y[lo:hi + beyond], R, match, mismatch, gap).max() > key["straddles_hi"]
    # the copy in front of lo: found from column 0, not from lo
    if lo >= 31:
        x = reads[NAMES.index("in_front_of_lo")]
        assert float(_exact(x, y[:hi]).max()) >= match * lo > exact["in_front_of_lo"]
        assert prefix_values(x, y[:hi], R, match, mismatch, gap).max() > key["in_front_of_lo"]
    assert exact["no_hit"] < match * P - slack(R, gap)               # (cheap gaps: a random read scores about half a copy)
