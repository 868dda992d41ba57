"""The inputs of tests/test_gpu_big_batch.py are what tests/big_batch_cases.py says they are — on the CPU, with the oracle alone:
the shares of the four classes, what the oracle makes of each class under every scoring the GPU test uses, that the batch which
precedes a checked one differs from it at EVERY index (a traced hit wherever the checked batch expects nothing), and that every
contiguous part a host loop could lose — one of 8, one of 64 — holds items of all four classes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_batch_cases as bb  # noqa: E402

SCORINGS = sorted({c[1] for c in bb.CONFIGS.values()})


@pytest.fixture(scope="module")
def y():
    return bb.make_y()


@pytest.fixture(scope="module")
def dictionary(y):
    return bb.make_dictionary(y)


@pytest.fixture(scope="module")
def records(oracle, dictionary, y):
    return {sc: bb.oracle_records(oracle, dictionary, y, sc) for sc in SCORINGS}


def _cls(d):
    return bb.CLASSES[d % 4]


def test_dictionary_shares_and_shapes(dictionary, y):
    assert len(y) == bb.YLEN == 40 and set(y) == set(bb.Y_LETTERS.tobytes()) and len(dictionary) == bb.D == 2048
    assert all(len(x) <= bb.MAXLEN and set(x) <= set(bb.AA) for x in dictionary)
    by = {c: [x for d, x in enumerate(dictionary) if _cls(d) == c] for c in bb.CLASSES}
    assert all(x == b"" for x in by["empty"]) and len(by["empty"]) >= 0.05 * bb.D
    assert all(x and not set(x) & set(y) for x in by["foreign"]) and len(by["foreign"]) >= 0.10 * bb.D
    assert len(by["planted"]) >= 0.25 * bb.D
    assert all(x and set(x) & set(y) for x in by["random"])
    full = [x for x in dictionary if x]
    assert len(set(full)) == len(full)                               # the non-empty entries are pairwise distinct
    for c in ("foreign", "random"):
        assert {1, 2, 63, 64} <= {len(x) for x in by[c]}
    assert max(len(x) for x in by["planted"]) == bb.MAXLEN


def test_classes_under_the_oracle(records):
    for sc, rec in records.items():
        for d, r in enumerate(rec):
            c = _cls(d)
            if c in ("empty", "foreign"):                            # nothing to find: the defined no-match record
                assert r == dict(score=0.0, pos=0, end_x=0, end_y=0, cons_x="", cons_y=""), (sc, d, r)
            else:                                                    # a traced hit
                assert r["score"] > 0 and r["end_x"] > 0 and r["end_y"] > 0 and len(r["cons_x"]) == len(r["cons_y"]) > 0, (sc, d, r)
    # planted entries: traced strings that hold gaps, on both sides (one inserted and one deleted letter)
    planted = [r for d, r in enumerate(records[bb.DEFAULT_SC]) if _cls(d) == "planted"]
    both = sum("-" in r["cons_x"] and "-" in r["cons_y"] for r in planted)
    assert both >= 0.9 * len(planted), both
    # ... and under the scoring of the "beyond" configuration a few of them lie beyond the packed float16 pass, most items do not
    beyond = sum(r["score"] >= bb.BEYOND_FROM for r in records[bb.BEYOND_SC])
    assert 16 <= beyond <= 0.1 * bb.D, beyond
    assert max(r["score"] for r in records[bb.DEFAULT_SC]) < bb.BEYOND_FROM


@pytest.mark.parametrize("n", bb.SIZES)
def test_preceding_batch_differs_everywhere(records, n):
    cur, prev = bb.seq(n), bb.seq(n, bb.STRIDE)
    assert (cur % 4 != prev % 4).all() and ((cur + 2) % 4 == prev % 4).all()
    for sc, rec in records.items():
        for k in range(n):
            a, b = rec[cur[k]], rec[prev[k]]
            assert a != b and all(a[key] != b[key] for key in ("score", "end_x", "end_y")), (sc, k)
            if a["score"] == 0:                                      # empty or score 0 in the checked batch: a traced hit before it
                assert b["score"] > 0 and b["cons_x"], (sc, k)
            else:                                                    # ... and the other way round
                assert b["score"] == 0 and not b["cons_x"], (sc, k)


@pytest.mark.parametrize("n", bb.SIZES)
def test_every_part_holds_every_class(n):
    for shift in (0, bb.STRIDE):
        s = bb.seq(n, shift)
        for nparts in (8, 64):
            ps = bb.parts(n, nparts)
            assert ps[0][0] == 0 and ps[-1][1] == n and all(a[1] == b[0] for a, b in zip(ps, ps[1:]))
            for k0, k1 in ps:
                assert {_cls(d) for d in s[k0:k1]} == set(bb.CLASSES), (n, nparts, k0, k1)
        assert len(np.unique(s[:min(n, bb.D)])) == min(n, bb.D)      # a permutation of the dictionary per 2048 items


def test_plan_covers_what_it_should():
    values = {v for v, _, _ in bb.PLAN}
    assert values == {None, "1", "3", "8", "16", "64"}
    assert {n for v, n, _ in bb.PLAN if v is None} == {49151, 49153} and 49153 % 256 != 0
    assert not bb.expect_pooled(None, 49151) and bb.expect_pooled(None, 49153) and not bb.expect_pooled("1", 3001)
    for v in ("3", "8", "16", "64"):
        assert {n for w, n, _ in bb.PLAN if w == v} == {1025, 3001} and bb.expect_pooled(v, 1025)
    full = [(v, n) for v, n, cfgs in bb.PLAN if set(cfgs) == set(bb.CONFIGS)]
    assert full == [(None, 49153), ("16", 3001)]
    assert all("default" in cfgs for _, _, cfgs in bb.PLAN)
