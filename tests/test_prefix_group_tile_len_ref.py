"""The fill rule of the seeded flow's group passes (host_score.h prefix_group_tile_len behind the C-ABI) against a plain
restatement of its model, over a grid, with its invariants and its pinned cases.  No GPU: the resident workgroups per CU are an argument.

The model: a launch of `pairs` reads over n columns on tiles of c columns has pairs x ceil(ceil(n / c) / (256 / SL)) workgroups, the
chip holds CUs x resident of them at once, a tile costs ceil((warm + c + SL) / 64) segments of 64 steps, and a launch costs the rounds
it holds plus a tail of f0 rounds.  The cheapest multiple of E between the redundancy floor and the old length wins — only with
>= 4 % gain."""
import itertools

import pytest

CUS, SL = 256, 2
OLD = 16384


MAX_ROUNDS = 2.0                                                     # kPrefixFillMaxRounds of host_score.h


def wgs_of(pairs, n, c):
    return pairs * -(-(-(-n // c)) // (256 // SL))


def cost(pairs, n, c, warm, resident, f0):
    wgs = wgs_of(pairs, n, c)
    slots = CUS * resident
    rounds = float(wgs) / float(slots) + f0
    return float(-(-(warm + c + SL) // 64) * 64) * rounds


def model(pairs, n, E, warm, resident, old, f0, cap, gain):
    if resident < 1:
        return old
    lo = E
    while lo <= old and float(warm + SL) >= cap * float(lo):
        lo += E
    if wgs_of(pairs, n, old) > MAX_ROUNDS * CUS * resident:                 # deeper than anything measured: nothing moves
        return old
    base = cost(pairs, n, old, warm, resident, f0)
    best, best_cost = old, base
    c = old // E * E
    while c >= lo:
        if c != old:
            k = cost(pairs, n, c, warm, resident, f0)
            if k < best_cost:
                best, best_cost = c, k
        c -= E
    return best if best_cost <= (1.0 - gain) * base else old


PAIRS = (1, 2, 3, 7, 20, 39, 61, 100, 121, 200, 256, 400, 700, 992, 1500, 2000)
COLS = (4 << 20, 5_000_001, 16_777_216, 50_000_000, 123_456_789, 250_000_000)


@pytest.mark.parametrize("E", (256, 512))
def test_rule_equals_the_model_and_keeps_its_invariants(pgs, E):
    f0, cap, gain = pgs.capi.prefix_fill_constants()
    assert 0.0 < f0 < 1.0 and 0.0 < cap < 0.25 and gain == 0.04
    moved = 0
    for pairs, n, resident, warm, old in itertools.product(PAIRS, COLS, (3, 4, 5), (64, 128, 192), (OLD, 8192, 65536)):
        got = pgs.capi.prefix_group_tile_len(pairs, n, E, warm, SL, CUS, resident, old)
        what = (pairs, n, E, warm, resident, old)
        assert got == model(pairs, n, E, warm, resident, old, f0, cap, gain), what
        assert got % E == 0 and E <= got <= old, what
        if got != old:
            moved += 1
            assert (warm + SL) / got < cap, what                                        # redundancy under the cap
            assert wgs_of(pairs, n, old) <= MAX_ROUNDS * CUS * resident, what           # only launches as shallow as those measured
            assert cost(pairs, n, got, warm, resident, f0) <= (1.0 - gain) * cost(pairs, n, old, warm, resident, f0), what
    assert moved > 0


def test_pinned_cases(pgs):
    tile = pgs.capi.prefix_group_tile_len
    # the bench batch's largest residual group: 121 reads = 61 pairs at R = 13, 5 workgroups resident per CU
    assert tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD) < OLD
    # its main pass before the settled reads, measured at 16384 columns (18.6 rounds): a fixed point
    assert tile(992, 50_000_000, 256, 128, SL, CUS, 5, OLD) == OLD
    # groups of some hundred reads, 2 - 8 rounds deep at the old length: never swept at any tile length, they stay
    for pairs in (120, 200, 260, 400):
        assert tile(pairs, 50_000_000, 256, 128, SL, CUS, 5, OLD) == OLD, pairs
    assert tile(88, 50_000_000, 256, 128, SL, CUS, 5, OLD) < OLD                        # (1.65 rounds: measured)
    # resident workgroups unknown: the rule before
    for resident in (0, -1):
        assert tile(61, 50_000_000, 256, 128, SL, CUS, resident, OLD) == OLD
    # explicit constants reach the rule: the longer a launch's tail, the shorter the tile; next to no tail, nothing to gain
    assert tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD, 1.0, 0.05) <= tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD, 0.3, 0.05) < OLD
    assert tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD, 1e-9, 0.05) == OLD
    # the redundancy cap is the floor: (128 + 2) / c < cap
    assert 3072 <= tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD, 0.5, 0.045) < 4096 <= tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD, 0.5, 1.0 / 30)
    assert tile(20, 50_000_000, 256, 128, SL, CUS, 4, 7680, 0.5, 0.045) == 3072      # (the model's optimum lies below the floor)
    # a cap nothing meets: the rule before
    assert tile(61, 50_000_000, 256, 128, SL, CUS, 5, OLD, 0.62, 1e-6) == OLD


def test_options_are_on_the_abi_list(pgs):
    names = pgs.capi.option_names()
    assert "no_prefix_fill" in names and "prefix_fill_min_cols" in names and "prefix_group_chunk" in names
    assert len(names) == len(set(names))
