"""world_size-2 gloo tests of the multi-GPU sharding logic on CPU.  The compute
callables are oracle-backed here (tests may use the oracle); on the GPU box the same functions are
driven by capi.Context methods."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, size, port, fn_name, ret):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_package
    pgs = load_package()
    from oracle import binding as ob
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        ret[rank] = globals()[fn_name](rank, size, pgs, ob)
    finally:
        dist.destroy_process_group()


def _run(fn_name, size=2):
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(size, port, fn_name, ret), nprocs=size, join=True)
    return dict(ret)


def _case_query_sharding(rank, size, pgs, ob):
    from parallel_genomeseq_amd import dist as pd
    ref = pgs.synth.dna(5, 20000)
    reads = [pgs.synth.read_from_ref(ref, 50 + k, [40, 80, 125, 150][k % 4])[0].tobytes() for k in range(11)]
    refb = ref.tobytes()
    calls = []

    def align_fn(qs):
        calls.append(len(qs))
        return [ob.align(q, refb, ob.F32) for q in qs]

    idx, res, g = pd.align_queries_sharded(align_fn, reads, weights=[len(r) * len(refb) for r in reads])
    best = pd.allreduce_best(max(r["score"] for r in res), int(idx[int(np.argmax([r["score"] for r in res]))]))
    return dict(idx=idx.tolist(), score=g["score"].tolist(), pos=g["pos"].tolist(), end_y=g["end_y"].tolist(), best=best,
                expect=[ob.align(q, refb, ob.F32) for q in reads])


def test_query_sharding_gloo():
    out = _run("_case_query_sharding")
    a, b = out[0], out[1]
    assert sorted(a["idx"] + b["idx"]) == list(range(11)) and not set(a["idx"]) & set(b["idx"])
    for o in (a, b):       # every rank holds the full gathered arrays
        assert o["score"] == [e["score"] for e in o["expect"]]
        assert o["pos"] == [e["pos"] for e in o["expect"]]
        assert o["end_y"] == [e["end_y"] for e in o["expect"]]
    scores = [e["score"] for e in a["expect"]]
    assert a["best"] == b["best"] == (float(max(scores)), int(np.argmax(scores)))   # ties -> lowest index


def _case_ref_sharding(rank, size, pgs, ob):
    from parallel_genomeseq_amd import dist as pd
    ref = pgs.synth.dna(6, 30000)
    q = ref[7000:7100].tobytes()
    ref = ref.tobytes()
    ref = ref[:21000] + q + ref[21000 + len(q):]          # second identical hit in a later piece
    out = {}
    for sm, la, npiece in ((ob.F32, ob.F32, 5), (ob.U8SAT, ob.U8SAT, 7)):
        ranges = ob.make_string_range(npiece, len(q), len(ref), 2.0)

        def maxima_fn(pieces):
            return [ob.score_only(q, ref[ranges[p][0]:ranges[p][1]], sm) for p in pieces]

        def final_fn(piece):
            l, r = ranges[piece]
            return ob.align(q, ref[l:r], la)

        res, piece = pd.align_split_sharded(ranges, maxima_fn, final_fn)
        exp = ob.align_split(q, ref, npiece, 2.0, sm, la)
        out[npiece] = (res, piece, exp)
    return out


def test_ref_sharding_gloo():
    out = _run("_case_ref_sharding")
    for rank in (0, 1):
        for npiece, (res, piece, exp) in out[rank].items():
            assert piece == exp["piece"]
            for k in ("score", "pos", "cons_x", "cons_y"):
                assert res[k] == exp[k], (rank, npiece, k)


def _fractional_case(pgs, ob, seed):
    """A query with a degraded second copy, fractional scoring 2.5 / -1.5 / 0.5: for seeds 81 and 138 two pieces'
    maxima differ by 0.5 only (92.0 | 92.5, 89.0 | 89.5), the larger one in the LATER piece — keys that truncate the
    score would elect the earlier piece."""
    ref = pgs.synth.dna(100 + seed, 6000).tobytes()
    q = pgs.synth.read_from_ref(np.frombuffer(ref, dtype=np.uint8), 7 + seed, 40, sub_rate=0.08, indel_rate=0.03)[0].tobytes()
    rng = np.random.default_rng(seed)
    q2 = bytearray(q)
    for k in rng.choice(40, size=3, replace=False):
        q2[k] = ord("ACGT"[("ACGT".index(chr(q2[k])) + 1) % 4])
    pos = int(rng.integers(100, 5000))
    return q, ref[:pos] + bytes(q2) + ref[pos + 40:]


def _case_ref_sharding_fractional(rank, size, pgs, ob):
    from parallel_genomeseq_amd import dist as pd
    out = {}
    sc = dict(match=2.5, mismatch=-1.5, gap=0.5)
    for seed in (81, 138):
        q, ref = _fractional_case(pgs, ob, seed)
        ranges = ob.make_string_range(6, len(q), len(ref), 2.0)
        full = [ob.score_only(q, ref[l:r], ob.F32, **sc) for l, r in ranges]

        def maxima_fn(pieces):
            return [full[p] for p in pieces]

        def final_fn(piece):
            l, r = ranges[piece]
            return ob.align(q, ref[l:r], ob.F32)                  # default scoring (plocalaligner.cpp:135)

        res, piece = pd.align_split_sharded(ranges, maxima_fn, final_fn)
        exp = ob.align_split(q, ref, 6, 2.0, ob.F32, ob.F32, **sc)
        out[seed] = (res, piece, exp, full)
    # fractional scores through the gather and the best-key all-reduce
    scores = [12.0, 12.5, 12.25, 12.5]
    lo, hi = pd.shard_block(len(scores), rank, size)
    idx, res, g = pd.align_queries_sharded(lambda qs: [dict(score=s, pos=1, end_x=1, end_y=1) for s in qs], scores)
    mine = scores[lo:hi]
    best = pd.allreduce_best(max(mine), lo + int(np.argmax(mine)))
    out["gather"] = (g["score"].tolist(), best)
    return out


def test_ref_sharding_fractional_scores_gloo():
    """scores travel as float32 bit patterns, so 92.5 beats 92.0 across ranks (serial rule
    plocalaligner.cpp:122-129 compares floats)."""
    out = _run("_case_ref_sharding_fractional")
    for rank in (0, 1):
        for seed in (81, 138):
            res, piece, exp, full = out[rank][seed]
            truncated = [int(v) for v in full]
            assert truncated.index(max(truncated)) != full.index(max(full))       # the case is what it claims to be
            assert piece == exp["piece"] == full.index(max(full))
            for k in ("score", "pos", "cons_x", "cons_y"):
                assert res[k] == exp[k], (rank, seed, k)
        g, best = out[rank]["gather"]
        assert g == [12.0, 12.5, 12.25, 12.5] and best == (12.5, 1)


def test_partitions():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_package
    load_package()
    from parallel_genomeseq_amd import dist as pd
    assert [pd.shard_block(10, r, 4) for r in range(4)] == [(0, 3), (3, 6), (6, 8), (8, 10)]
    bins = pd.shard_lpt([9, 1, 1, 1, 8, 2, 2, 3], 2)
    assert sorted(np.concatenate(bins).tolist()) == list(range(8))
    loads = [sum([9, 1, 1, 1, 8, 2, 2, 3][i] for i in b) for b in bins]
    assert abs(loads[0] - loads[1]) <= 1
    assert pd.unpack_key(max(pd.pack_key(30, 5), pd.pack_key(30, 2), pd.pack_key(29, 0))) == (30.0, 2)
    assert pd.unpack_key(max(pd.pack_key(12.0, 1), pd.pack_key(12.5, 3))) == (12.5, 3)
    assert pd.pack_key(0.0, 0) > 0                                  # a piece whose maximum is 0 still beats "no piece"


def _case_ref_sharding_certified(rank, size, pgs, ob):
    """align_split_sharded_certified with best_fn callables that behave like mi355_sw_best_range under an optimistic margin:
    a first sweep that UNDER-reports every maximum below a certification threshold (here: halves it), exact above it and in
    the second sweep (known_best given).  Cases: the true best above the threshold (one round), below it (two rounds), and a
    tie between pieces of different ranks."""
    from parallel_genomeseq_amd import dist as pd
    ref = pgs.synth.dna(6, 30000)
    q = ref[7000:7100].tobytes()
    refb = ref.tobytes()
    refb = refb[:21000] + q + refb[21000 + len(q):]        # the same hit in a later piece (other rank): lowest piece wins
    out = {}
    for name, threshold in (("above", 250.0), ("below", 400.0)):
        ranges = ob.make_string_range(6, len(q), len(refb), 2.0)
        calls = []

        def best_fn(pieces, known_best):
            calls.append(known_best)
            true = [ob.score_only(q, refb[ranges[p][0]:ranges[p][1]], ob.F32) for p in pieces]
            if known_best > 0:                              # second sweep: exact for everything >= known_best
                seen, above = true, -1.0
            else:
                seen = [t if t > threshold else float(int(t) // 2) for t in true]
                above = threshold
            at = int(np.argmax(seen))
            return seen[at], at, above

        def final_fn(piece):
            l, r = ranges[piece]
            return ob.align(q, refb[l:r], ob.F32)

        res, piece, rounds = pd.align_split_sharded_certified(ranges, best_fn, final_fn)
        out[name] = (res, piece, rounds, list(calls), ob.align_split(q, refb, 6, 2.0, ob.F32, ob.F32))
    return out


def test_ref_sharding_certified_gloo():
    out = _run("_case_ref_sharding_certified")
    for rank in (0, 1):
        for name, (res, piece, rounds, calls, exp) in out[rank].items():
            assert piece == exp["piece"], (rank, name)
            for k in ("score", "pos", "cons_x", "cons_y"):
                assert res[k] == exp[k], (rank, name, k)
            assert rounds == (1 if name == "above" else 2), (rank, name, rounds, calls)
            assert calls[0] == 0.0 and (name == "above" or calls[1] > 0)


# ---- the gather of align_queries_sharded carries what the C-ABI returns: end_y is an int64 column (references of 2^31 letters and more)
WIDE_END_Y = [0, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, 3_100_000_000, 2 ** 40 + 7]
WIDE = [dict(score=s, pos=p, end_x=x, end_y=y)
        for s, p, x, y in zip([0.0, 12.5, 12.25, 0.7, 1234.75, 3.0000002], [0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 2, 77],
                              [0, 1, 2 ** 31 - 1, 64, 40000, 7], WIDE_END_Y)]
WIDE_WEIGHTS = [5, 1, 9, 2, 8, 3]                                    # LPT at world 2: interleaved shards {0, 2, 5} / {1, 3, 4}


def _gather_wide(rank, size, pgs, ob, weights, rows=WIDE):
    from parallel_genomeseq_amd import dist as pd
    idx, res, g = pd.align_queries_sharded(lambda qs: [dict(rows[q]) for q in qs], list(range(len(rows))), weights=weights)
    assert all(g[k].dtype == (np.float32 if k == "score" else np.int64) for k in g)
    return dict(idx=idx.tolist(), **{k: g[k].tolist() for k in ("score", "pos", "end_x", "end_y")})


def _case_gather_wide_block(rank, size, pgs, ob):
    return _gather_wide(rank, size, pgs, ob, None)


def _case_gather_wide_lpt(rank, size, pgs, ob):
    return _gather_wide(rank, size, pgs, ob, WIDE_WEIGHTS)


def _case_gather_end_x_too_wide(rank, size, pgs, ob):
    rows = [dict(r) for r in WIDE]
    rows[4]["end_x"] = 2 ** 31                                       # (block shards at world 2: rank 1 alone holds it)
    try:
        _gather_wide(rank, size, pgs, ob, None, rows)
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize("size", (1, 2))
@pytest.mark.parametrize("shards", ("block", "lpt"))
def test_gather_carries_wide_end_y_gloo(size, shards):
    """end_y of 2^31 and beyond (int64 in the C-ABI), pos up to 2^32 - 1 and fractional scores arrive exactly on every rank; packed
    into one int32 word, end_y = 2^31 + 5 came back as -2147483643 and 3 100 000 000 as -1194967296."""
    out = _run("_case_gather_wide_" + shards, size)
    assert sorted(out) == list(range(size))
    every = sorted(i for o in out.values() for i in o["idx"])
    assert every == list(range(len(WIDE)))
    if size == 2 and shards == "lpt":
        assert out[0]["idx"] != list(range(len(out[0]["idx"])))      # shards that are no contiguous blocks
    for rank in range(size):
        o = out[rank]
        assert o["score"] == [float(np.float32(r["score"])) for r in WIDE], rank
        for k in ("pos", "end_x", "end_y"):
            assert o[k] == [r[k] for r in WIDE], (rank, k, o[k])


@pytest.mark.parametrize("size", (1, 2))
def test_gather_refuses_end_x_beyond_int32_gloo(size):
    """end_x = 2^31 is refused, not wrapped — on EVERY rank, so none is left waiting in the collective."""
    out = _run("_case_gather_end_x_too_wide", size)
    for rank in range(size):
        assert out[rank] is not None and "end_x" in out[rank], (rank, out[rank])
