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

  * --band W_HALF[,W_HALF..]: the same pairs with the band [flank - w, flank + w] around the diagonal of the read's true locus (flank:
    the columns the window starts in front of it), Context.affine_pairs_run(band_lo=, band_hi=) on sw_affine_band_kernel, against the
    unbanded local instance on the same pairs, alternating in one process, medians.  A band is a different answer, so the check is
    the banded exact kernel (option no_affine_band), once per width; kernel time, ratio and the op-count model (ops per cell x cells
    of both kernels, from mi355_sw_last_kernel) come side by side.  Default --out: profiles/affine_pairs_band_n1.json.

  * --extend: the same reads, each window cut to START at the read's true start (the anchored model needs that) and to end 64
    columns behind it: Context.affine_extend_run on sw_affine_pair_ext_kernel against the local instance (sw_affine_pair_kernel) on the
    same pairs, alternating in one process, medians; the op-count model of both comes from mi355_sw_last_kernel, and the extension
    result is checked once against the same call on the exact kernel (option no_affine_pairs).  Default --out:
    profiles/affine_pairs_extend_n1.json.

  * --extend --band W_HALF[,W_HALF..]: the pairs of --extend with the band [-w, w] around the anchor's diagonal,
    Context.affine_extend_run(band_lo=, band_hi=) on sw_affine_band_ext_kernel, against the unbanded extension call
    (sw_affine_pair_ext_kernel) on the same pairs, alternating in one process, medians.  A band is a different answer, so the check
    is the exact kernel under the band (option no_affine_band), once per width; kernel time, ratio and the ratio the row loop's op
    count predicts come side by side.  Default --out: profiles/affine_extend_band_n1.json.

  * --extend --band W_HALF[,W_HALF..] --zdrop Z[,Z..] [--chimeric F] [--scoring M,X,O,E]: the pairs of --extend --band under the z-drop stop
    rule, Context.affine_extend_zdrop_run on sw_affine_band_extz_kernel, against the banded extension call (sw_affine_band_ext_kernel)
    on the same pairs and bands, alternating in one process, medians and the spread of the steps.  --chimeric F replaces the tail of
    that share of the reads, from a random point between 20 % and 80 % of the read, by random letters: the reads a stop rule is for.
    Beside the times: the share of pairs that stopped, the rows the wavefronts ran (counter zdrop_rows_run) against the rows of the
    list and against rows_done, and the ratio the row loops' op counts predict for a zdrop that never fires.  The z-drop result is
    checked once per width against the exact path (option no_affine_band).  Default --out: profiles/affine_extend_zdrop_n1.json
    (with --chimeric: affine_extend_zdrop_chimeric_n1.json).

  * --global [--band W_HALF[,W_HALF..]]: the reads of --extend, each against the window [at, at + 150) behind its true start, anchored at
    both ends: Context.affine_global_run on sw_affine_pair_glob_kernel (with --band: under [-w, w] on sw_affine_band_glob_kernel)
    alternating with Context.affine_extend_run (with --band: the banded extension call) on the same pairs in one process, medians
    and the spread of the steps.  The yardstick is the extension instance of the same run: the global loop is a strict subset of its
    loop, so a kernel ratio above 1.0 is a finding.  The global result is checked once against the exact kernel (options
    no_affine_pairs / no_affine_band); the op-count prediction from mi355_sw_last_kernel of both sides comes beside the measured
    ratio.  Default --out: profiles/affine_global_n1.json / affine_global_band_n1.json.

Prints ONE JSON line and writes it to --out; kernel times are those of mi355_sw_last_timings (device events), call times are wall
clock around the call.

    python tools/affine_pairs_bench.py [--pairs 100000 --ref-len 5000000 --steps 5 --warmup 1 --out profiles/affine_pairs_n1.json]
    python tools/affine_pairs_bench.py --mode end_to_end
    python tools/affine_pairs_bench.py --band 8,16,32,64
    python tools/affine_pairs_bench.py --extend
    python tools/affine_pairs_bench.py --extend --band 8,16,32,64
    python tools/affine_pairs_bench.py --extend --band 8,16,32,64 --zdrop 1048576
    python tools/affine_pairs_bench.py --extend --band 8,16,32,64 --zdrop 20,100 --chimeric 0.5 --scoring 1,-4,7,1
    python tools/affine_pairs_bench.py --global
    python tools/affine_pairs_bench.py --global --band 8,16,32,64

--read-len N (default 150, the instance R = 10 of the pair kernels) times another instance of kPairR: 30 / 80 / 150 / 250 / 380 / 500
rows reach R = 2 / 5 / 10 / 16 / 24 / 32; the windows grow with the read.
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
    global READ_LEN
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--ref-len", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("local", "end_to_end"), default="local")
    ap.add_argument("--band", default=None, help="half widths of the band around the read's diagonal, comma separated")
    ap.add_argument("--extend", action="store_true", help="the anchored extension call against the local instance")
    ap.add_argument("--global", dest="glob", action="store_true", help="the call anchored at both ends against the extension call")
    ap.add_argument("--read-len", type=int, default=READ_LEN, help="rows of a read: picks the instance of the pair kernels")
    ap.add_argument("--zdrop", default=None, help="with --extend --band: z-drop values, comma separated; the stop rule against the banded call")
    ap.add_argument("--chimeric", type=float, default=0.0, help="with --zdrop: share of the reads whose tail is replaced by random letters")
    ap.add_argument("--scoring", default=None, help="with --zdrop: match,mismatch,gap_open,gap_extend instead of 3,-3,5,1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    READ_LEN = args.read_len
    if args.zdrop is not None and not (args.extend and args.band is not None):
        ap.error("--zdrop needs --extend --band")
    if (args.chimeric or args.scoring is not None) and args.zdrop is None:
        ap.error("--chimeric and --scoring belong to --zdrop")
    if args.glob and (args.extend or args.mode != "local"):
        ap.error("--global stands alone (with --band or without)")
    if args.extend and args.mode != "local":
        ap.error("--extend needs the local mode")
    if args.band is not None and args.mode != "local":
        ap.error("--band needs the local mode")
    if args.out is None and args.zdrop is not None:
        args.out = os.path.join(ROOT, "profiles", "affine_extend_zdrop_chimeric_n1.json" if args.chimeric else "affine_extend_zdrop_n1.json")
    if args.out is None:
        name = "affine_global_band_n1.json" if args.glob and args.band is not None else "affine_global_n1.json" if args.glob else "affine_extend_band_n1.json" if args.extend and args.band is not None else "affine_pairs_extend_n1.json" if args.extend else "affine_pairs_band_n1.json" if args.band is not None else "affine_pairs_e2e_n1.json" if args.mode == "end_to_end" else "affine_pairs_n1.json"
        args.out = os.path.join(ROOT, "profiles", name)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    ref = pgs.synth.dna(31, args.ref_len)
    reads, lefts, rights = [], np.zeros(args.pairs, dtype=np.int64), np.zeros(args.pairs, dtype=np.int64)
    diag = np.zeros(args.pairs, dtype=np.int64)                       # the diagonal j - i of the read's true locus in its window
    for k in range(args.pairs):
        read, at = pgs.synth.read_from_ref(ref, 1000 + k, READ_LEN, sub_rate=0.03, indel_rate=0.02)[:2]
        if args.chimeric and k < args.chimeric * args.pairs:          # a chimeric read: the tail from a random point is junk
            rng = np.random.default_rng(7000 + k)
            cut = int(rng.integers(READ_LEN // 5, 4 * READ_LEN // 5))
            read = read.copy()
            read[cut:] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(read) - cut)]
        reads.append(read.tobytes())
        lefts[k] = int(at) if args.extend or args.glob else max(0, int(at) - FLANK)
        rights[k] = min(args.ref_len, int(at) + READ_LEN + (0 if args.glob else FLANK))
        diag[k] = int(at) - lefts[k]
    query = np.arange(args.pairs, dtype=np.int32)
    ctx = pgs.Context(0)
    ctx.set_reference(ref.tobytes())
    ctx.batch_upload(reads)
    if args.glob:
        return global_against_extend(args, ctx, reads, query, lefts, rights)
    if args.zdrop is not None:
        return zdrop_against_banded_extend(args, ctx, reads, query, lefts, rights)
    if args.extend and args.band is not None:
        return banded_extend_against_extend(args, ctx, reads, query, lefts, rights)
    if args.extend:
        return extend_against_local(args, ctx, reads, query, lefts, rights)
    if args.mode == "end_to_end":
        return e2e_against_local(args, ctx, reads, query, lefts, rights)
    if args.band is not None:
        return banded_against_local(args, ctx, reads, query, lefts, rights, diag)
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


def extend_against_local(args, ctx, reads, query, lefts, rights):
    """The local instance of the pair kernel and the extension instance on the same pairs (windows that start at the read's true
    start), alternating; one JSON line."""
    sides = ("local", "extend")
    t = {s: dict(kernel_us=[], call_ms=[]) for s in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side in sides:                                          # alternating: both sides see the same clocks
            t0 = time.perf_counter()
            got = ctx.affine_pairs_run(query, lefts, rights, **SCORING) if side == "local" else ctx.affine_extend_run(query, lefts, rights, **SCORING)
            wall = time.perf_counter() - t0
            lt, ki = ctx.last_timings(), ctx.last_kernel()
            info[side] = dict(path=ctx.last_path(), kernel=ki["name"], launches=lt["score_launches"], valu_ops_per_cell=ki["valu_ops_per_cell"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"])
                t[side]["call_ms"].append(wall * 1e3)
    ctx.set_option("no_affine_pairs", 1)
    try:
        exact = ctx.affine_extend_run(query, lefts, rights, **SCORING)
    finally:
        ctx.set_option("no_affine_pairs", 0)
    fields = ("score", "end_x", "end_y", "to_end_score", "to_end_y")
    equal = all(np.array_equal(results["extend"][f], exact[f]) for f in fields)
    ext = results["extend"]
    cells = float(np.dot([len(r) for r in reads], rights - lefts))
    line = dict(bench="affine_pairs_bench", mode="extend", pairs=args.pairs, read_len=READ_LEN, window=READ_LEN + FLANK,
                ref_len=args.ref_len, scoring="3/-3/5/1", steps=args.steps, cells=cells, results_equal_exact_kernel=bool(equal),
                mean_score=float(ext["score"].mean()), mean_to_end_score=float(ext["to_end_score"].mean()),
                mean_score_local=float(results["local"]["score"].mean()), clipped=float((ext["end_x"] < READ_LEN).mean()),
                not_above_local=bool((ext["score"] <= results["local"]["score"]).all()),
                to_end_not_above_best=bool((ext["to_end_score"] <= ext["score"]).all()))
    for side in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, gcups_kernel=cells / max(k_us, 1e-9) / 1e3)
    line["kernel_ratio_ext_over_local"] = line["extend"]["kernel_ms"] / max(line["local"]["kernel_ms"], 1e-9)
    line["call_ratio_ext_over_local"] = line["extend"]["call_ms"] / max(line["local"]["call_ms"], 1e-9)
    line["model_ratio_ext_over_local"] = line["extend"]["valu_ops_per_cell"] / line["local"]["valu_ops_per_cell"]
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if equal and line["not_above_local"] and line["to_end_not_above_best"] else 1


def global_against_extend(args, ctx, reads, query, lefts, rights):
    """The extension instance and the global instance on the same pairs (windows of the read's length behind its true start), unbanded
    or at every half width of --band, alternating; one JSON line."""
    widths = [int(w) for w in str(args.band).split(",")] if args.band is not None else [None]
    tag = lambda w: "" if w is None else "_w%d" % w
    sides = [(kind + tag(w), kind, w) for w in widths for kind in ("extend", "global")]
    t = {s: dict(kernel_us=[], call_ms=[]) for s, _, _ in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side, kind, w in sides:                                 # alternating: all sides see the same clocks
            kw = dict(band_lo=-w, band_hi=w) if w is not None else {}
            call = ctx.affine_global_run if kind == "global" else ctx.affine_extend_run
            t0 = time.perf_counter()
            got = call(query, lefts, rights, **kw, **SCORING)
            wall = time.perf_counter() - t0
            lt, ki = ctx.last_timings(), ctx.last_kernel()
            info[side] = dict(path=ctx.last_path(), kernel=ki["name"], launches=lt["score_launches"], valu_ops_per_cell=ki["valu_ops_per_cell"],
                              rows_per_lane=ki["rows_per_lane"], cells=lt["cells"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"])
                t[side]["call_ms"].append(wall * 1e3)
    equal = {}
    option = "no_affine_pairs" if args.band is None else "no_affine_band"
    ctx.set_option(option, 1)
    try:
        for side, kind, w in sides:
            if kind == "global":
                kw = dict(band_lo=-w, band_hi=w) if w is not None else {}
                exact = ctx.affine_global_run(query, lefts, rights, **kw, **SCORING)
                equal[side] = bool(np.array_equal(results[side]["score"], exact["score"]) and not any(p.startswith("affine_pair_glob") or
                                   p.startswith("affine_band_glob") for p in ctx.last_path()))
    finally:
        ctx.set_option(option, 0)
    line = dict(bench="affine_pairs_bench", mode="global", band_half_widths=None if args.band is None else widths, pairs=args.pairs,
                read_len=READ_LEN, window=READ_LEN, ref_len=args.ref_len, scoring="3/-3/5/1", steps=args.steps,
                results_equal_exact_kernel=equal)
    for side, kind, w in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, gcups_kernel=info[side]["cells"] / max(k_us, 1e-9) / 1e3,
                          kernel_ms_min=min(t[side]["kernel_us"]) / 1e3, kernel_ms_max=max(t[side]["kernel_us"]) / 1e3,
                          call_ms_min=min(t[side]["call_ms"]), call_ms_max=max(t[side]["call_ms"]))
    ok = all(equal.values())
    for w in widths:
        e, g = line["extend" + tag(w)], line["global" + tag(w)]
        ge, gg = results["extend" + tag(w)], results["global" + tag(w)]
        g["mean_score"] = float(gg["score"][np.isfinite(gg["score"])].mean())
        g["unreachable"] = float((~np.isfinite(gg["score"])).mean())
        g["negative"] = float((gg["score"] < 0).mean())
        g["equals_to_end_score"] = float((gg["score"] == ge["to_end_score"]).mean())
        g["not_above_to_end"] = bool((gg["score"] <= ge["to_end_score"]).all())   # the corner is one cell of row m
        ok = ok and g["not_above_to_end"]
        # same instance, same steps, same cells on both sides: the prediction is the ratio of the ops per cell
        g["kernel_ratio_global_over_extend"] = g["kernel_ms"] / max(e["kernel_ms"], 1e-9)
        g["call_ratio_global_over_extend"] = g["call_ms"] / max(e["call_ms"], 1e-9)
        g["model_ratio_global_over_extend"] = (g["rows_per_lane"] * g["valu_ops_per_cell"]) / (e["rows_per_lane"] * e["valu_ops_per_cell"])
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if ok else 1


def banded_extend_against_extend(args, ctx, reads, query, lefts, rights):
    """The unbanded extension instance and the banded one at every half width of --band on the same pairs, alternating; one JSON line."""
    widths = [int(w) for w in str(args.band).split(",")]
    sides = ["extend"] + ["band_w%d" % w for w in widths]
    bands = {"band_w%d" % w: (-w, w) for w in widths}
    fields = ("score", "end_x", "end_y", "to_end_score", "to_end_y")
    t = {s: dict(kernel_us=[], call_ms=[]) for s in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side in sides:                                          # alternating: all sides see the same clocks
            kw = dict(band_lo=bands[side][0], band_hi=bands[side][1]) if side in bands else {}
            t0 = time.perf_counter()
            got = ctx.affine_extend_run(query, lefts, rights, **kw, **SCORING)
            wall = time.perf_counter() - t0
            lt, ki = ctx.last_timings(), ctx.last_kernel()
            info[side] = dict(path=ctx.last_path(), kernel=ki["name"], launches=lt["score_launches"], valu_ops_per_cell=ki["valu_ops_per_cell"],
                              rows_per_lane=ki["rows_per_lane"], cells=lt["cells"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"])
                t[side]["call_ms"].append(wall * 1e3)
    equal = {}
    ctx.set_option("no_affine_band", 1)
    try:
        for side in bands:
            exact = ctx.affine_extend_run(query, lefts, rights, band_lo=bands[side][0], band_hi=bands[side][1], **SCORING)
            equal[side] = all(np.array_equal(results[side][f], exact[f]) for f in fields)
    finally:
        ctx.set_option("no_affine_band", 0)
    line = dict(bench="affine_pairs_bench", mode="extend", band_half_widths=widths, pairs=args.pairs, read_len=READ_LEN,
                window=READ_LEN + FLANK, ref_len=args.ref_len, scoring="3/-3/5/1", steps=args.steps, results_equal_exact_kernel=equal)
    for side in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, gcups_kernel=info[side]["cells"] / max(k_us, 1e-9) / 1e3,
                          mean_score=float(results[side]["score"].mean()), mean_to_end_score=float(results[side]["to_end_score"][np.isfinite(results[side]["to_end_score"])].mean()))
        # the spread of the timed steps, beside the medians: a ratio of a few percent means nothing inside it
        line[side].update(kernel_ms_min=min(t[side]["kernel_us"]) / 1e3, kernel_ms_max=max(t[side]["kernel_us"]) / 1e3,
                          call_ms_min=min(t[side]["call_ms"]), call_ms_max=max(t[side]["call_ms"]))
    base = line["extend"]
    steps_ext, steps_band = float((rights - lefts + 15).sum()), float(sum(len(r) for r in reads))
    for side in bands:
        b = line[side]
        b["same_score_as_unbanded"] = float((results[side]["score"] == results["extend"]["score"]).mean())
        b["same_to_end_as_unbanded"] = float((results[side]["to_end_score"] == results["extend"]["to_end_score"]).mean())
        b["unreachable"] = float((results[side]["to_end_y"] < 0).mean())
        b["not_above_unbanded"] = bool((results[side]["score"] <= results["extend"]["score"]).all() and
                                       (results[side]["to_end_score"] <= results["extend"]["to_end_score"]).all())
        b["kernel_ratio_unbanded_over_band"] = base["kernel_ms"] / max(b["kernel_ms"], 1e-9)
        b["call_ratio_unbanded_over_band"] = base["call_ms"] / max(b["call_ms"], 1e-9)
        # ops of a lane per pair: steps x registers x ops per register — the pair instance streams the window's columns + 15 of skew
        # past its rows, the band kernel steps through the rows over all 16 R diagonals of its instance, whatever W is
        b["model_ratio_unbanded_over_band"] = (steps_ext * base["rows_per_lane"] * base["valu_ops_per_cell"]) / \
                                              (steps_band * b["rows_per_lane"] * b["valu_ops_per_cell"])
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if all(equal.values()) and all(line[s]["not_above_unbanded"] for s in bands) else 1


def zdrop_against_banded_extend(args, ctx, reads, query, lefts, rights):
    """The banded extension call and the z-drop call at every value of --zdrop, at every half width of --band, on the same pairs,
    alternating; one JSON line."""
    widths = [int(w) for w in str(args.band).split(",")]
    zdrops = [float(z) for z in str(args.zdrop).split(",")]
    scoring = dict(SCORING)
    if args.scoring is not None:
        scoring = dict(zip(("match", "mismatch", "gap_open", "gap_extend"), (float(v) for v in args.scoring.split(","))))
    sides = []
    for w in widths:
        sides.append(("band_w%d" % w, w, None))
        sides += [("zdrop_w%d_z%g" % (w, z), w, z) for z in zdrops]
    fields = ("score", "end_x", "end_y", "to_end_score", "to_end_y")
    t = {s[0]: dict(kernel_us=[], call_ms=[]) for s in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side, w, z in sides:                                    # alternating: all sides see the same clocks
            t0 = time.perf_counter()
            if z is None:
                got = ctx.affine_extend_run(query, lefts, rights, band_lo=-w, band_hi=w, **scoring)
            else:
                got = ctx.affine_extend_zdrop_run(query, lefts, rights, band_lo=-w, band_hi=w, zdrop=z, **scoring)
            wall = time.perf_counter() - t0
            lt, ki, c = ctx.last_timings(), ctx.last_kernel(), ctx.last_counters()
            info[side] = dict(path=ctx.last_path(), kernel=ki["name"], launches=lt["score_launches"], valu_ops_per_cell=ki["valu_ops_per_cell"],
                              rows_per_lane=ki["rows_per_lane"], cells=lt["cells"], zdrop_stopped=c["zdrop_stopped"], zdrop_rows_run=c["zdrop_rows_run"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"])
                t[side]["call_ms"].append(wall * 1e3)
    equal = {}
    ctx.set_option("no_affine_band", 1)
    try:
        for w in widths:                                            # once per width, at the first zdrop: the exact path's two steps
            side = "zdrop_w%d_z%g" % (w, zdrops[0])
            exact = ctx.affine_extend_zdrop_run(query, lefts, rights, band_lo=-w, band_hi=w, zdrop=zdrops[0], **scoring)
            equal[side] = all(np.array_equal(results[side][f], exact[f]) for f in fields + ("rows_done",))
    finally:
        ctx.set_option("no_affine_band", 0)
    rows = np.array([len(r) for r in reads], dtype=np.int64)
    line = dict(bench="affine_pairs_bench", mode="extend_zdrop", band_half_widths=widths, zdrops=zdrops, chimeric=args.chimeric, pairs=args.pairs,
                read_len=READ_LEN, window=READ_LEN + FLANK, ref_len=args.ref_len, scoring="%g/%g/%g/%g" % tuple(scoring.values()),
                steps=args.steps, rows_of_the_list=int(rows.sum()), wavefront_rows_of_the_list=int(((rows.sum() + 3) // 4)),
                results_equal_exact_path=equal)
    for side, w, z in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, mean_score=float(results[side]["score"].mean()),
                          kernel_ms_min=min(t[side]["kernel_us"]) / 1e3, kernel_ms_max=max(t[side]["kernel_us"]) / 1e3,
                          call_ms_min=min(t[side]["call_ms"]), call_ms_max=max(t[side]["call_ms"]))
        if z is None:
            continue
        b, base = line[side], line["band_w%d" % w]
        b["stopped_share"] = float((results[side]["rows_done"] < rows).mean())
        b["rows_done_sum"] = int(results[side]["rows_done"].sum())
        b["same_score_as_banded"] = float((results[side]["score"] == results["band_w%d" % w]["score"]).mean())
        # a wavefront holds four pairs and runs to the last of them: its rows against a quarter of the rows of the list
        b["wavefront_rows_share"] = b["zdrop_rows_run"] / max(1.0, rows.sum() / 4.0)
        b["kernel_ratio_zdrop_over_banded"] = b["kernel_ms"] / max(base["kernel_ms"], 1e-9)
        b["call_ratio_zdrop_over_banded"] = b["call_ms"] / max(base["call_ms"], 1e-9)
        b["model_ratio_zdrop_over_banded_all_rows"] = b["valu_ops_per_cell"] / base["valu_ops_per_cell"]
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if all(equal.values()) else 1


def banded_against_local(args, ctx, reads, query, lefts, rights, diag):
    """The unbanded local instance and the band kernel at every half width of --band on the same pairs, alternating; one JSON line."""
    widths = [int(w) for w in str(args.band).split(",")]
    sides = ["local"] + ["band_w%d" % w for w in widths]
    bands = {"band_w%d" % w: (diag - w, diag + w) for w in widths}
    t = {s: dict(kernel_us=[], call_ms=[]) for s in sides}
    info, results = {}, {}
    for step in range(args.warmup + args.steps):
        for side in sides:                                          # alternating: all sides see the same clocks
            kw = dict(band_lo=bands[side][0], band_hi=bands[side][1]) if side in bands else {}
            t0 = time.perf_counter()
            got = ctx.affine_pairs_run(query, lefts, rights, **kw, **SCORING)
            wall = time.perf_counter() - t0
            lt, ki = ctx.last_timings(), ctx.last_kernel()
            info[side] = dict(path=ctx.last_path(), kernel=ki["name"], launches=lt["score_launches"], valu_ops_per_cell=ki["valu_ops_per_cell"],
                              rows_per_lane=ki["rows_per_lane"], cells=lt["cells"])
            results[side] = got
            if step >= args.warmup:
                t[side]["kernel_us"].append(lt["score_us"])
                t[side]["call_ms"].append(wall * 1e3)
    equal = {}
    ctx.set_option("no_affine_band", 1)
    try:
        for side in bands:
            exact = ctx.affine_pairs_run(query, lefts, rights, band_lo=bands[side][0], band_hi=bands[side][1], **SCORING)
            equal[side] = all(np.array_equal(results[side][f], exact[f]) for f in ("score", "end_x", "end_y"))
    finally:
        ctx.set_option("no_affine_band", 0)
    line = dict(bench="affine_pairs_bench", band_half_widths=widths, pairs=args.pairs, read_len=READ_LEN, window=READ_LEN + 2 * FLANK,
                ref_len=args.ref_len, scoring="3/-3/5/1", steps=args.steps, results_equal_exact_kernel=equal)
    for side in sides:
        k_us, c_ms = statistics.median(t[side]["kernel_us"]), statistics.median(t[side]["call_ms"])
        line[side] = dict(info[side], kernel_ms=k_us / 1e3, call_ms=c_ms, gcups_kernel=info[side]["cells"] / max(k_us, 1e-9) / 1e3,
                          mean_score=float(results[side]["score"].mean()))
    base = line["local"]
    steps_local, steps_band = float((rights - lefts + 15).sum()), float(sum(len(r) for r in reads))
    for side in bands:
        b = line[side]
        b["same_score_as_unbanded"] = float((results[side]["score"] == results["local"]["score"]).mean())
        b["kernel_ratio_local_over_band"] = base["kernel_ms"] / max(b["kernel_ms"], 1e-9)
        b["call_ratio_local_over_band"] = base["call_ms"] / max(b["call_ms"], 1e-9)
        # ops of a lane per pair: steps x registers x ops per register — the local instance streams the window's columns + 15 of
        # skew past its rows, the band kernel steps through the rows over all 16 R diagonals of its instance, whatever W is
        b["model_ratio_local_over_band"] = (steps_local * base["rows_per_lane"] * base["valu_ops_per_cell"]) / \
                                           (steps_band * b["rows_per_lane"] * b["valu_ops_per_cell"])
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
