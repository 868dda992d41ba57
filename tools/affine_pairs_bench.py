"""The extension stage of a seed-and-extend mapper on the device: a list of (read, window) pairs under affine gaps.

  * 100 000 reads of 150 bp made by synth.read_from_ref (substitutions and indels) from a 5 Mbp reference, each aligned against the
    window of 150 + 2 x 64 columns around its true locus (clipped at the reference's ends), scoring 3 / -3 / 5 / 1, reference and
    reads resident: Context.affine_pairs_run;
  * the default dispatch (sw_affine_pair_kernel) and option no_affine_pairs (every pair a whole problem of sw_affine_exact_kernel)
    alternate in one process, --steps runs each after --warmup, medians; both results must be equal.

  * --mode end_to_end: the same pairs, the local instance (sw_affine_pair_kernel) and the end-to-end one (sw_affine_pair_e2e_kernel:
    the whole read against its window) alternate in one process, medians; the yardstick is the local instance of the same run, the
    op-count model of both comes from mi355_sw_last_kernel, and the end-to-end result is checked once against the same call on the
    exact kernel (option no_affine_pairs).  Default --out: profiles/affine_pairs_e2e_n1.json.

Prints ONE JSON line and writes it to --out; kernel times are those of mi355_sw_last_timings (device events), call times are wall
clock around the call.

    python tools/affine_pairs_bench.py [--pairs 100000 --ref-len 5000000 --steps 5 --warmup 1 --out profiles/affine_pairs_n1.json]
    python tools/affine_pairs_bench.py --mode end_to_end
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ_LEN, FLANK = 150, 64
SCORING = dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--ref-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("local", "end_to_end"), default="local")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "affine_pairs_e2e_n1.json" if args.mode == "end_to_end" else "affine_pairs_n1.json")
    import __graft_entry__ as entry
    pgs = entry._load_package()
    ref = pgs.synth.dna(31, args.ref_len)
    reads, lefts, rights = [], np.zeros(args.pairs, dtype=np.int64), np.zeros(args.pairs, dtype=np.int64)
    for k in range(args.pairs):
        read, at = pgs.synth.read_from_ref(ref, 1000 + k, READ_LEN, sub_rate=0.03, indel_rate=0.02)[:2]
        reads.append(read.tobytes())
        lefts[k] = max(0, int(at) - FLANK)
        rights[k] = min(args.ref_len, int(at) + READ_LEN + FLANK)
    query = np.arange(args.pairs, dtype=np.int32)
    ctx = pgs.Context(0)
    ctx.set_reference(ref.tobytes())
    ctx.batch_upload(reads)
    if args.mode == "end_to_end":
        return e2e_against_local(args, ctx, reads, query, lefts, rights)
    sides = {"pair_kernel": 0, "exact_kernel": 1}
    t = {s: dict(kernel_us=[], call_ms=[]) for s in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side, off in sides.items():                             # alternating: both sides see the same clocks
            ctx.set_option("no_affine_pairs", off)
            try:
                t0 = time.perf_counter()
                got = ctx.affine_pairs_run(query, lefts, rights, **SCORING)
                wall = time.perf_counter() - t0
            finally:
                ctx.set_option("no_affine_pairs", 0)
            lt = ctx.last_timings()
            info[side] = dict(path=ctx.last_path(), kernel=ctx.last_kernel()["name"], launches=lt["score_launches"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"] + lt["locate_us"])   # [0] pair kernel, [1] exact kernel
                t[side]["call_ms"].append(wall * 1e3)
    equal = all(np.array_equal(results["pair_kernel"][f], results["exact_kernel"][f]) for f in ("score", "end_x", "end_y"))
    cells = float(np.dot([len(r) for r in reads], rights - lefts))
    line = dict(bench="affine_pairs_bench", pairs=args.pairs, read_len=READ_LEN, window=READ_LEN + 2 * FLANK, ref_len=args.ref_len,
                scoring="3/-3/5/1", steps=args.steps, cells=cells, results_equal=bool(equal),
                mean_score=float(results["pair_kernel"]["score"].mean()))
    for side in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, gcups_kernel=cells / max(k_us, 1e-9) / 1e3)
    line["speedup_kernel"] = line["exact_kernel"]["kernel_ms"] / max(line["pair_kernel"]["kernel_ms"], 1e-9)
    line["speedup_call"] = line["exact_kernel"]["call_ms"] / max(line["pair_kernel"]["call_ms"], 1e-9)
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if equal else 1


def e2e_against_local(args, ctx, reads, query, lefts, rights):
    """The local and the end-to-end instance of the pair kernel on the same pairs, alternating; one JSON line."""
    sides = ("local", "end_to_end")
    t = {s: dict(kernel_us=[], call_ms=[]) for s in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side in sides:                                          # alternating: both sides see the same clocks
            t0 = time.perf_counter()
            got = ctx.affine_pairs_run(query, lefts, rights, mode=side, **SCORING)
            wall = time.perf_counter() - t0
            lt, ki = ctx.last_timings(), ctx.last_kernel()
            info[side] = dict(path=ctx.last_path(), kernel=ki["name"], launches=lt["score_launches"], valu_ops_per_cell=ki["valu_ops_per_cell"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"])
                t[side]["call_ms"].append(wall * 1e3)
    ctx.set_option("no_affine_pairs", 1)
    try:
        exact = ctx.affine_pairs_run(query, lefts, rights, mode="end_to_end", **SCORING)
    finally:
        ctx.set_option("no_affine_pairs", 0)
    equal = all(np.array_equal(results["end_to_end"][f], exact[f]) for f in ("score", "end_x", "end_y"))
    cells = float(np.dot([len(r) for r in reads], rights - lefts))
    line = dict(bench="affine_pairs_bench", mode="end_to_end", pairs=args.pairs, read_len=READ_LEN, window=READ_LEN + 2 * FLANK,
                ref_len=args.ref_len, scoring="3/-3/5/1", steps=args.steps, cells=cells, results_equal_exact_kernel=bool(equal),
                mean_score=float(results["end_to_end"]["score"].mean()), mean_score_local=float(results["local"]["score"].mean()),
                not_above_local=bool((results["end_to_end"]["score"] <= results["local"]["score"]).all()))
    for side in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, gcups_kernel=cells / max(k_us, 1e-9) / 1e3)
    line["kernel_ratio_e2e_over_local"] = line["end_to_end"]["kernel_ms"] / max(line["local"]["kernel_ms"], 1e-9)
    line["call_ratio_e2e_over_local"] = line["end_to_end"]["call_ms"] / max(line["local"]["call_ms"], 1e-9)
    line["model_ratio_e2e_over_local"] = line["end_to_end"]["valu_ops_per_cell"] / line["local"]["valu_ops_per_cell"]
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if equal and line["not_above_local"] else 1


if __name__ == "__main__":
    sys.exit(main())
