"""What the sampled running maximum of sw_score_kernel costs in candidates, on the bench shape: 2048 x 150 bp reads against the 50 Mbp
synthetic reference (seeds of bench.py), inputs resident.  Two batches: the bench batch (every read has a hit), and the same batch
with 5 % of the reads replaced by uniform random 150-mers — reads WITHOUT a hit, whose key is the background maximum and whose
candidates are every sub-chunk within the sweep's slack of it.  Per batch: ms per call (host clock around
batch_run, which ends in a device synchronise; median over --steps), the sweep's device time, and the counters of the candidate
filters.  Prints ONE JSON line; run it on two builds of the library to compare them.

    python tools/row_sample_ab.py [--steps 5 --warmup 1 --reads 2048 --read-len 150 --ref-len 50000000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--no-hit-fraction", type=float, default=0.05)
    args = ap.parse_args(argv)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    ctx = pgs.Context(0)
    ref = pgs.synth.dna(3, args.ref_len)
    reads, _ = pgs.synth.reads_from_ref(ref, 4, args.reads, args.read_len)
    reads = [r.tobytes() for r in reads]
    ctx.set_reference(ref)
    nohit = list(reads)
    every = max(1, int(round(1.0 / args.no_hit_fraction)))
    replaced = 0
    for k in range(every - 1, args.reads, every):                   # spread over the batch: the reads of a tile pair stay mixed
        nohit[k] = pgs.synth.dna(1000 + k, args.read_len).tobytes()
        replaced += 1
    line = dict(tool="row_sample_ab", reads=args.reads, read_len=args.read_len, ref_len=args.ref_len, steps=args.steps,
                no_hit_reads=replaced)
    for name, batch in (("bench_batch", reads), ("with_no_hit_reads", nohit)):
        ctx.batch_upload(batch)
        ms, sweep_ms = [], []
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.batch_run(raw=True)
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                ms.append(dt * 1e3)
                sweep_ms.append(ctx.last_timings()["score_us"] * 1e-3)
        cnt = ctx.last_counters()
        line[name] = dict(ms_per_call=statistics.median(ms), ms_per_call_all=[round(v, 3) for v in ms],
                          sweep_ms=statistics.median(sweep_ms), requeried=cnt["requeried"],
                          whole_batch_again=cnt["whole_batch_again"], candidates=cnt["candidates"],
                          kernel=ctx.last_kernel()["name"], valu_ops_per_cell=ctx.last_kernel()["valu_ops_per_cell"],
                          path=[t for t in ctx.last_path() if t.startswith("score[")][:2])
    ctx.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
