"""Affine-gap database search on the UniProt-shaped batch: synth's 561 356 protein sequences (bench.py's config 4) against the
144-letter query P02232 under a seeded 20-letter integer table in [-4, 11] with gaps 11 / 1, inputs resident.

  * the whole batch, score and end cell (Context.affine_batch_run): sw_affine_prof_kernel;
  * next to it the linear engine's score-only call on the same batch with identity scoring 3 / -3 / 2 (the float32 profile pass under
    option no_wave_f16, and the packed float16 pass the library takes by default);
  * A/B against the former dispatch (option no_affine_prof: every sequence a whole problem of sw_affine_exact_kernel), alternating in
    one process, score-only and with the traceback.  The former path refuses sequences beyond the exact kernel's LDS (about 5 600
    rows) and takes seconds for the whole batch, and the traceback of half a million alignments fills ~10^11 window cells on either
    path: both A/B pairs run on a SUBSAMPLE — the first --sub sequences of at most --sub-max-len rows — and the line says so.

Prints ONE JSON line and writes it to --out; kernel times are those of mi355_sw_last_timings (device events), medians over --steps.

    python tools/affine_db_bench.py [--sequences 561356 --sub 16384 --steps 5 --warmup 1 --out profiles/affine_db_n1.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AA20 = b"ACDEFGHIKLMNPQRSTVWY"
OPEN, EXTEND = 11.0, 1.0
LINEAR_MODEL_OPS = 4.5                                             # sw_wave_prof_kernel<TRACK>: add, max3, sub, or, half a max3


def seeded_table(seed=11):
    rng = np.random.default_rng(seed)
    t = rng.integers(-4, 12, (20, 20))
    t = np.triu(t) + np.triu(t, 1).T
    t[np.arange(20), np.arange(20)] = rng.integers(4, 12, 20)
    aa = np.frombuffer(AA20, dtype=np.uint8)
    lut = np.full((256, 256), -4.0, dtype=np.float32)
    lut[np.ix_(aa, aa)] = t
    return lut


def med(v):
    return statistics.median(v) if v else None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=561_356)
    ap.add_argument("--sub", type=int, default=16384)
    ap.add_argument("--sub-max-len", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_db_n1.json"))
    args = ap.parse_args(argv)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    lens = pgs.synth.lognormal_lengths(5, args.sequences)
    tot = int(lens.sum())
    res = pgs.synth.protein(5, tot)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    y = pgs.synth.P02232
    lut = seeded_table()
    kw = dict(gap_open=OPEN, gap_extend=EXTEND, lut=lut)
    ctx = pgs.Context(0)
    ctx.set_reference(y)
    line = dict(bench="affine_db_bench", sequences=args.sequences, residues=tot, query_len=len(y), steps=args.steps,
                scoring=dict(affine="seeded 20-letter table in [-4, 11], open 11 / extend 1", linear="identity 3 / -3 / 2"))

    # ---- the whole batch: the new kernel, and the linear engine's pass as context ------------------------------------------------
    ctx.batch_upload_packed(res, offs)
    t = dict(affine=dict(kernel_us=[], total_us=[]), linear_f32=dict(kernel_us=[], total_us=[]), linear_default=dict(kernel_us=[], total_us=[]))
    info = {}

    def linear(f32):
        ctx.set_option("no_wave_f16", 1 if f32 else 0)
        try:
            ctx.batch_run(semantics=pgs.F32, flags=pgs.capi.SCORE_ONLY, raw=True)
        finally:
            ctx.set_option("no_wave_f16", 0)

    runs = dict(affine=lambda: ctx.affine_batch_run(**kw), linear_f32=lambda: linear(True), linear_default=lambda: linear(False))
    for step in range(args.warmup + args.steps):
        for name, fn in runs.items():
            fn()
            lt = ctx.last_timings()
            if step >= args.warmup:
                t[name]["kernel_us"].append(lt["score_us"])
                t[name]["total_us"].append(lt["total_us"])
            info[name] = dict(path=ctx.last_path(), cells=lt["cells"], kernel=ctx.last_kernel())
    cells = float(tot) * len(y)
    k_us = med(t["affine"]["kernel_us"])
    line["affine_full"] = dict(kernel=info["affine"]["kernel"]["name"], path=info["affine"]["path"], kernel_ms=k_us / 1e3,
                               call_device_ms=med(t["affine"]["total_us"]) / 1e3, cells=info["affine"]["cells"],
                               tcups=info["affine"]["cells"] / k_us / 1e6, valu_ops_per_cell=info["affine"]["kernel"]["valu_ops_per_cell"])
    for name in ("linear_f32", "linear_default"):
        # (the linear engine's batch path reports its passes in the call's device time)
        d_us = med(t[name]["total_us"])
        line[name] = dict(path=info[name]["path"], call_device_ms=d_us / 1e3, cells=cells, tcups_of_call=cells / d_us / 1e6)
    line["model"] = dict(affine_ops_per_cell=line["affine_full"]["valu_ops_per_cell"], linear_f32_ops_per_cell=LINEAR_MODEL_OPS,
                         predicted_rate_ratio=LINEAR_MODEL_OPS / line["affine_full"]["valu_ops_per_cell"],
                         measured_rate_ratio_call=line["affine_full"]["call_device_ms"] and line["linear_f32"]["call_device_ms"] / line["affine_full"]["call_device_ms"])

    # ---- A/B against the former dispatch on a subsample --------------------------------------------------------------------------
    keep = [k for k in range(args.sequences) if lens[k] <= args.sub_max_len][:args.sub]
    sub_lens = lens[keep]
    sub_offs = np.concatenate([[0], np.cumsum(sub_lens)]).astype(np.int64)
    sub = np.empty(int(sub_lens.sum()), dtype=np.uint8)
    for j, k in enumerate(keep):
        sub[sub_offs[j]:sub_offs[j + 1]] = res[offs[k]:offs[k + 1]]
    ctx.batch_upload_packed(sub, sub_offs)
    sub_cells = float(sub_lens.sum()) * len(y)
    ab = {(mode, side): dict(kernel_us=[], total_us=[], trace_us=[]) for mode in ("score", "trace") for side in ("new", "former")}
    paths = {}
    for step in range(args.warmup + args.steps):
        for mode in ("score", "trace"):
            for side in ("new", "former"):                         # alternating: both sides see the same clocks
                ctx.set_option("no_affine_prof", 1 if side == "former" else 0)
                try:
                    if mode == "score":
                        ctx.affine_batch_run(**kw)
                    else:
                        ctx.affine_batch_trace(**kw)
                finally:
                    ctx.set_option("no_affine_prof", 0)
                lt = ctx.last_timings()
                paths[(mode, side)] = ctx.last_path()
                if step >= args.warmup:
                    ab[(mode, side)]["kernel_us"].append(lt["score_us"] + lt["locate_us"])   # [0] new kernel, [1] exact kernel
                    ab[(mode, side)]["total_us"].append(lt["total_us"])
                    ab[(mode, side)]["trace_us"].append(lt["trace_us"])
    line["subsample"] = dict(sequences=len(keep), residues=int(sub_lens.sum()), cells=sub_cells, max_len=int(sub_lens.max()),
                             note="the first %d sequences of at most %d rows: the former path refuses longer ones and takes seconds for the whole batch; "
                                  "the traceback of the whole batch fills ~1e11 window cells on either path" % (args.sub, args.sub_max_len))
    for mode in ("score", "trace"):
        new, old = ab[(mode, "new")], ab[(mode, "former")]
        line["ab_" + mode] = dict(new_path=paths[(mode, "new")], former_path=paths[(mode, "former")],
                                  new_score_kernel_ms=med(new["kernel_us"]) / 1e3, former_score_kernel_ms=med(old["kernel_us"]) / 1e3,
                                  new_call_device_ms=med(new["total_us"]) / 1e3, former_call_device_ms=med(old["total_us"]) / 1e3,
                                  new_trace_kernel_ms=med(new["trace_us"]) / 1e3, former_trace_kernel_ms=med(old["trace_us"]) / 1e3,
                                  speedup_score_kernel=med(old["kernel_us"]) / max(med(new["kernel_us"]), 1e-9),
                                  speedup_call=med(old["total_us"]) / max(med(new["total_us"]), 1e-9),
                                  new_tcups=sub_cells / max(med(new["kernel_us"]), 1e-9) / 1e6)
    ctx.close()
    text = json.dumps(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
