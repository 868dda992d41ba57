"""What settling reads by the windows of their seed hits (host_pipeline.h prefix_seeded, "settled") costs and saves,
on the bench shape: 2048 x 150 bp reads against the 50 Mbp synthetic reference (seeds of bench.py), inputs resident.  The batches of
tools/prefix_seed_ab.py — the bench batch, the same offsets at 10 % substitutions, the bench batch with every 20th read replaced by a
random 150-mer, the first 512 reads — and the repeat-rich batch of bench.py's extra_repeat_rich on its own reference, each under option
no_seed_certify (the parent's flow) and under the default dispatch, the two alternating call by call.  Per batch and option: median ms
per batch_run call (host clock; the call ends in a device synchronise), the spread of the calls (max - min), the counters, the prefix
and seed notes of the path, and whether score / pos / end cell equal those of the other option.  `within_bound`: the default costs
no more than the parent's flow plus three times that flow's own spread.  Prints ONE JSON line.

    python tools/seed_certify_ab.py [--steps 6 --warmup 1 --reads 2048 --read-len 150 --ref-len 50000000]
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

OPTION = "no_seed_certify"
OPTIONS = (OPTION, None)
FIELDS = ("score", "pos", "end_x", "end_y")


def measure(ctx, batch, args):
    ctx.batch_upload(batch)
    ms = {o: [] for o in OPTIONS}
    out, rec = {}, {}
    for step in range(args.warmup + args.steps):
        for option in OPTIONS:
            ctx.set_option(OPTION, True if option else None)
            t0 = time.perf_counter()
            out[option] = ctx.batch_run(raw=True)
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                ms[option].append(dt * 1e3)
            cnt, kernel, tim = ctx.last_counters(), ctx.last_kernel(), ctx.last_timings()
            rec[option] = dict(
                sweep_ms=tim["score_us"] * 1e-3, locate_ms=tim["locate_us"] * 1e-3, score_launches=tim["score_launches"],
                seed_certified=cnt["seed_certified"], prefix_certified=cnt["prefix_certified"], prefix_second_pass=cnt["prefix_second_pass"],
                requeried=cnt["requeried"], whole_batch_again=cnt["whole_batch_again"], candidates=cnt["candidates"],
                prefix_thinned=cnt["prefix_thinned"], prefix_seeded=cnt["prefix_seeded"], prefix_seed_hits=cnt["prefix_seed_hits"],
                rows_per_lane=kernel["rows_per_lane"], cells=kernel["cells"],
                path=[t for t in ctx.last_path() if t.startswith(("prefix", "seed_certify")) or t in ("requery", "whole_again")])
    line = {}
    for option in OPTIONS:
        rec[option].update(ms_per_call=statistics.median(ms[option]), spread_ms=max(ms[option]) - min(ms[option]),
                           ms_per_call_all=[round(v, 3) for v in ms[option]])
        line[option or "default"] = rec[option]
    line["equal"] = all(bool(np.array_equal(out[None][f], out[OPTION][f])) for f in FIELDS)
    parent, default = line[OPTION], line["default"]
    line["within_bound"] = default["ms_per_call"] <= parent["ms_per_call"] + 3.0 * parent["spread_ms"]
    ctx.set_option(OPTION, None)
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    args = ap.parse_args(argv)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    line = dict(tool="seed_certify_ab", reads=args.reads, read_len=args.read_len, ref_len=args.ref_len, steps=args.steps)
    ctx = pgs.Context(0)
    try:
        ref = pgs.synth.dna(3, args.ref_len)
        ctx.set_reference(ref)
        bench = [r.tobytes() for r in pgs.synth.reads_from_ref(ref, 4, args.reads, args.read_len)[0]]
        subs10 = [r.tobytes() for r in pgs.synth.reads_from_ref(ref, 4, args.reads, args.read_len, sub_rate=0.10)[0]]
        nohit = list(bench)
        for k in range(19, args.reads, 20):
            nohit[k] = pgs.synth.dna(1000 + k, args.read_len).tobytes()
        for name, batch in (("bench_batch", bench), ("subs_10_percent", subs10), ("with_no_hit_reads", nohit), ("first_512_reads", bench[:512])):
            line[name] = measure(ctx, batch, args)
        # the repeat-rich batch on its own reference (bench.py extra_repeat_rich)
        ref, planted = pgs.synth.dna_repeats(33, args.ref_len, families=4, family_len=300, copies=4000, divergence=0.03,
                                             tandem_runs=500, tandem_len=400, polya_runs=500, polya_len=300)
        reads = pgs.synth.reads_with_repeats(ref, planted, 34, args.reads, args.read_len, repeat_fraction=0.01)[0]
        ctx.set_reference(ref)
        line["repeat_rich"] = measure(ctx, [r.tobytes() for r in reads], args)
    finally:
        ctx.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
