"""What the tile length of the seeded flow's group passes costs (host_score.h prefix_group_tile_len), on the bench shape:
2048 x 150 bp reads against the 50 Mbp synthetic reference (seeds of bench.py), inputs resident.  Two batches whose groups differ in
size — the bench batch, and the bench batch with every 20th read replaced by a random 150-mer (tools/seed_certify_ab.py) — each under
the default rule, under option no_prefix_fill (the rule before), and with prefix_group_chunk forcing the groups' tiles to each of
--chunks.  The settings alternate call by call in one process.  Per batch and setting: median ms per batch_run call (host clock; the
call ends in a device synchronise) and its spread, the device time of the call's score launches, whether all five result arrays equal
the default's, and per group pass (--steps further calls under option trace, stderr read back, settings alternating again): rows
per lane, pairs, tile, workgroups, slots, the rounds the model counts, the length of the rule before, and the median and spread of
the launch's device time over those calls.  Prints ONE JSON line.

    python tools/prefix_group_tiles.py [--steps 7 --warmup 2 --chunks 1024,2048,... --reads 2048 --read-len 150 --ref-len 50000000]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("score", "pos", "end_x", "end_y", "cons_len")
CHUNKS = (1024, 2048, 3072, 4096, 6144, 8192, 12288, 16384)
FILL = re.compile(r"prefix fill: R=(\d+) pairs=(\d+) tile=(\d+) workgroups=(\d+) slots=(\d+) rounds=([0-9.]+) old=(\d+)")
LAUNCH = re.compile(r"score launch: ([0-9.]+) ms")


def apply(ctx, setting):
    ctx.set_option("no_prefix_fill", True if setting == "no_prefix_fill" else None)
    ctx.set_option("prefix_group_chunk", setting if isinstance(setting, int) else None)


def traced_call(ctx):
    """One call under option trace with the process's stderr in a file: the group passes in launch order."""
    sys.stderr.flush()
    keep = os.dup(2)
    groups = []
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            ctx.set_option("trace", True)
            ctx.batch_run(raw=True)
        finally:
            ctx.set_option("trace", None)
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode("latin-1")
    pending = None
    for line in text.splitlines():
        m = FILL.search(line)
        if m:
            pending = dict(zip(("R", "pairs", "tile", "workgroups", "slots"), map(int, m.groups()[:5])), rounds=float(m.group(6)), old=int(m.group(7)))
            continue
        m = LAUNCH.search(line)
        if m and pending is not None:
            pending["device_ms"] = float(m.group(1))
            groups.append(pending)
            pending = None
    return groups


def traced_groups(ctx, settings, calls):
    """Per setting the group passes with the MEDIAN device time of `calls` traced calls (and their spread), the settings alternating
    call by call as in the timed loop; the traced calls are apart from the timed ones, whose host clock the trace would disturb."""
    seen = {s: [] for s in settings}
    for _ in range(calls):
        for s in settings:
            apply(ctx, s)
            seen[s].append(traced_call(ctx))
    out = {}
    for s in settings:
        groups = [dict(g) for g in seen[s][0]]
        for k, g in enumerate(groups):
            ms = [call[k]["device_ms"] for call in seen[s] if len(call) == len(groups)]
            g.update(device_ms=statistics.median(ms), device_spread_ms=max(ms) - min(ms), device_calls=len(ms))
        out[s] = groups
    return out


def measure(ctx, batch, settings, args):
    ctx.batch_upload(batch)
    ms = {s: [] for s in settings}
    sweep = {s: [] for s in settings}
    out, rec = {}, {}
    for step in range(args.warmup + args.steps):
        for s in settings:
            apply(ctx, s)
            t0 = time.perf_counter()
            out[s] = ctx.batch_run(raw=True)
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                ms[s].append(dt * 1e3)
                sweep[s].append(ctx.last_timings()["score_us"] * 1e-3)
            cnt = ctx.last_counters()
            rec[s] = dict(seed_certified=cnt["seed_certified"], prefix_certified=cnt["prefix_certified"], prefix_second_pass=cnt["prefix_second_pass"],
                          requeried=cnt["requeried"], candidates=cnt["candidates"], prefix_thinned=cnt["prefix_thinned"],
                          path=[t for t in ctx.last_path() if t.startswith("prefix_group")])
    line = {}
    groups = traced_groups(ctx, settings, args.steps)
    for s in settings:
        rec[s].update(ms_per_call=statistics.median(ms[s]), spread_ms=max(ms[s]) - min(ms[s]), sweep_ms=statistics.median(sweep[s]),
                      equal=all(bool(np.array_equal(out[s][f], out[None][f])) for f in FIELDS), groups=groups[s])
        line["default" if s is None else str(s)] = rec[s]
    apply(ctx, None)
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunks", default=",".join(str(c) for c in CHUNKS))
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    args = ap.parse_args(argv)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    settings = [None, "no_prefix_fill"] + [int(c) for c in args.chunks.split(",") if c]
    line = dict(tool="prefix_group_tiles", reads=args.reads, read_len=args.read_len, ref_len=args.ref_len, steps=args.steps,
                constants=dict(zip(("f0", "cap", "gain"), pgs.capi.prefix_fill_constants())))
    ctx = pgs.Context(0)
    try:
        ref = pgs.synth.dna(3, args.ref_len)
        ctx.set_reference(ref)
        bench = [r.tobytes() for r in pgs.synth.reads_from_ref(ref, 4, args.reads, args.read_len)[0]]
        nohit = list(bench)
        for k in range(19, args.reads, 20):
            nohit[k] = pgs.synth.dna(1000 + k, args.read_len).tobytes()
        for name, batch in (("bench_batch", bench), ("with_no_hit_reads", nohit)):
            line[name] = measure(ctx, batch, settings, args)
    finally:
        ctx.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
