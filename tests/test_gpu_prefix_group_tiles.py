"""The tile lengths the fill rule of the seeded flow's group passes can choose (host_score.h prefix_group_tile_len), on the
device.

Raw values: the step tiles at 768 and 1280 columns — 3 and 5 sub-chunks per tile, no power of two, which tests/test_gpu_prefix_step_tiles.py
and tests/test_gpu_prefix_low_tiles.py (1024 columns) do not reach — for every height of the seeded flow, against the numpy emulation
(tests/prefix_cascade.py tile_values with mk = 1), exactly: keys and the value of every sub-chunk.

The flow: the batch of tests/test_gpu_prefix_seed_flow.py on its reference of about 1 Mi columns with the gates lowered, the new one
included.  On 256 CUs so short a reference leaves every launch far under one round on 2048-column tiles, so the chip is declared 32
CUs wide (option assume_cus: it sizes launches, nothing else): the largest group's launch is then between one and two rounds deep on
16384-column tiles, the bench's situation, and the rule shortens them.  Every field equals the same call under no_prefix_fill, under no_prefix and the oracle; the
largest group's tile is what the C-ABI function returns for its pairs and columns; with the gate at its default nothing moves."""
import numpy as np
import pytest

from oracle import binding as ob
from prefix_cascade import LANES, tile_values
from row_sampled_fold import SUB
from test_gpu_prefix_seed_flow import FIELDS, GATES, M, N, batch, run      # noqa: F401  (batch: the module's fixture, built again here)

pytestmark = pytest.mark.gpu

SCORING = (3.0, -3.0, 2.0)
LO = 5                                                               # no multiple of 4: the staging's byte shift
NAMES = ["starts_at_lo", "across_the_tiles", "ends_at_hi", "no_hit"]
CUS = 32
FILL_GATES = GATES + (("prefix_fill_min_cols", 1), ("assume_cus", CUS))
FREE = ("seed_certified", "prefix_certified", "prefix_second_pass", "requeried")    # counters that do not depend on where tiles are cut


def _batch(R, chunk, n):
    P = LANES * R
    rng = np.random.default_rng(9900 + 64 * R + chunk)
    y = bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
    hi = n
    reads = [y[LO:LO + M],
             y[LO + 2 * chunk - 60:LO + 2 * chunk - 60 + M],         # rows 1 .. P end in the second tile, the copy in the third
             y[hi - P:hi] + b"N" * (M - P),                           # row P ends in the range's last column
             bytes(rng.choice(list(b"ACGT"), M).astype(np.uint8))]
    return reads, y


@pytest.mark.parametrize("chunk", [768, 1280])
@pytest.mark.parametrize("R", [8, 10, 13, 16, 19])
def test_step_tile_values_on_3_and_5_sub_chunks(pgs, R, chunk):
    P = LANES * R
    match, mismatch, gap = SCORING
    n = LO + 2 * chunk + 77 + 17                                    # a little over two tiles, the last sub-chunk partial
    lo, hi = LO, n
    reads, y = _batch(R, chunk, n)
    ctx = pgs.Context(0)
    try:
        ctx.set_option("prefix_rowp_step", R)
        ctx.set_option("chunk", chunk)
        ctx.set_reference(y)
        ctx.batch_upload(reads)
        got = ctx.score_ranges([(lo, hi)], semantics=pgs.F32, match=match, mismatch=mismatch, gap=gap)[0]
        values = ctx.prefix_values()
        path, kernel = " ".join(ctx.last_path()), ctx.last_kernel()
    finally:
        ctx.close()
    assert "prefix[SL=2,R=%d,P=%d,fold=rowP,step=1]" % (R, P) in path, path
    assert kernel["lanes"] == LANES and kernel["rows_per_lane"] == R and kernel["chunk_len"] == chunk and kernel["sub_len"] == SUB, kernel
    assert chunk // SUB in (3, 5) and chunk % SUB == 0 and lo % 4 != 0
    assert 2 * chunk < hi - lo < 2 * chunk + SUB and (hi - lo) % SUB != 0
    assert values is not None and values.shape == (len(reads), 3 * chunk // SUB), None if values is None else values.shape
    for k, (name, x) in enumerate(zip(NAMES, reads)):
        emu = tile_values(x, y[lo:hi], R, chunk, kernel["warm"], match, mismatch, gap, mk=1)
        print("R=%d chunk=%d %-18s key %g, emulated %s" % (R, chunk, name, got[k], emu.astype(int).tolist()))
        assert values[k].tolist() == emu.tolist(), (name, values[k].tolist(), emu.tolist())
        assert got[k] == emu.max(), (name, got[k], float(emu.max()))
    assert all(got[k] == match * P for k in (0, 1, 2)), got


@pytest.fixture(scope="module")
def runs(pgs, batch):
    y, reads = batch["y"], batch["reads"]
    fill = run(pgs, y, reads, FILL_GATES[len(GATES):])[0]
    old = run(pgs, y, reads, FILL_GATES[len(GATES):] + (("no_prefix_fill", 1),))[0]
    sweep = run(pgs, y, reads, (("no_prefix", 1),))[0]
    return fill, old, sweep


def _groups(path):
    out = {}
    for t in path:
        if t.startswith("prefix_group[R="):
            r, n = t[len("prefix_group[R="):-1].split(",n=")
            out.setdefault(int(r), int(n))                            # (a height's first pass; second passes join later groups)
    return out


def test_flow_fields_equal_the_rule_before_the_sweep_and_the_oracle(batch, runs):
    fill, old, sweep = runs
    print(" ".join(fill["path"]))
    print(fill["counters"])
    groups = _groups(fill["path"])
    assert len(groups) >= 3 and min(groups.values()) < 256 <= max(groups.values()), groups      # three heights, one group small
    assert "prefix_group[" in " ".join(old["path"]) and "prefix[" not in " ".join(sweep["path"])
    for other, name in ((old, "no_prefix_fill"), (sweep, "no_prefix")):
        for f in FIELDS:
            assert np.array_equal(fill["res"][f], other["res"][f]), (name, f, np.flatnonzero(fill["res"][f] != other["res"][f])[:8])
    y, res = batch["y"], fill["res"]
    picked, per = [], {}
    for q, (x, at) in enumerate(zip(batch["reads"], batch["where"])):
        if at < 0 or b"N" in x or x == batch["repeat"]:
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


def test_largest_group_takes_the_rule_s_tile(pgs, runs):
    fill, old, sweep = runs
    groups = _groups(fill["path"])
    assert groups == _groups(old["path"])
    for name in FREE:
        assert fill["counters"][name] == old["counters"][name], (name, fill["counters"][name], old["counters"][name])
    R, n = max(groups.items(), key=lambda g: g[1])
    kf, ko = fill["kernel"], old["kernel"]
    assert kf["rows_per_lane"] == R == ko["rows_per_lane"] and kf["sub_len"] == ko["sub_len"] == 256, (kf, ko)
    resident = fill["counters"]["prefix_fill_resident"]
    print("largest group R=%d n=%d: tile %d, before %d, warm %d, resident %d, moved %d passes"
          % (R, n, kf["chunk_len"], ko["chunk_len"], kf["warm"], resident, fill["counters"]["prefix_fill_moved"]))
    assert 1 <= resident <= 8 and old["counters"]["prefix_fill_resident"] == 0 and old["counters"]["prefix_fill_moved"] == 0
    want = pgs.capi.prefix_group_tile_len((n + 1) // 2, N, kf["sub_len"], kf["warm"], LANES, CUS, resident, ko["chunk_len"])
    assert kf["chunk_len"] == want, (kf["chunk_len"], want)
    assert kf["chunk_len"] < ko["chunk_len"] and fill["counters"]["prefix_fill_moved"] >= 1, (kf["chunk_len"], ko["chunk_len"])


def test_default_gate_keeps_the_rule_before(pgs, batch, runs):
    fill, old, sweep = runs
    y, reads = batch["y"], batch["reads"]
    gated = run(pgs, y, reads, (("assume_cus", CUS),))[0]             # 1 Mi columns are below the gate's 4 Mi
    # (the seed and calibration tags carry measured times: compared without them, as tests/test_gpu_prefix_seed_flow.py does)
    plain = lambda path: [t.split(",scan_us")[0].split(",ms=")[0] for t in path]
    assert plain(gated["path"]) == plain(old["path"]), (gated["path"], old["path"])
    assert gated["counters"] == old["counters"], (gated["counters"], old["counters"])
    assert gated["kernel"]["chunk_len"] == old["kernel"]["chunk_len"] and gated["counters"]["prefix_fill_moved"] == 0
    for f in FIELDS:
        assert np.array_equal(gated["res"][f], old["res"][f]), f


def test_prefix_group_chunk_forces_the_groups_alone(pgs, batch, runs):
    fill, old, sweep = runs
    y, reads = batch["y"], batch["reads"]
    forced = run(pgs, y, reads, (("assume_cus", CUS), ("prefix_group_chunk", 1280)))[0]
    assert forced["kernel"]["chunk_len"] == 1280 and forced["kernel"]["sub_len"] == 256, forced["kernel"]
    for f in FIELDS:
        assert np.array_equal(forced["res"][f], old["res"][f]), f
    for name in FREE:
        assert forced["counters"][name] == old["counters"][name], name
    # a call that runs no seeded group: the full sweep's tile is what it is without the option
    plain = run(pgs, y, reads, (("no_prefix", 1), ("prefix_group_chunk", 1280)))[0]
    assert plain["kernel"]["chunk_len"] == sweep["kernel"]["chunk_len"] != 1280, (plain["kernel"], sweep["kernel"])
    assert [t.split(",ms=")[0] for t in plain["path"]] == [t.split(",ms=")[0] for t in sweep["path"]], (plain["path"], sweep["path"])
