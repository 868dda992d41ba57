"""Affine-gap sweep against the plain float16 linear sweep on the bench shape: 2048 x 150 bp reads against the 50 Mbp synthetic
reference (seeds of bench.py), inputs resident.  Times Context.affine_batch_run at 3 / -3 / open 5 / extend 1 and, alternating with
it in the same process, the linear batch_run(flags=SCORE_ONLY) under option no_f16_mirror (the plain float16 cell), then
Context.affine_batch_trace (score, end cell and traceback) and the linear batch_run with its traceback on the same resident batch.
Prints ONE JSON line; the kernel times are those of mi355_sw_last_timings (device events around the sweep launches; [2] around the
traceback kernels), medians over --steps.

    python tools/affine_bench.py [--steps 5 --warmup 1 --reads 2048 --read-len 150 --ref-len 50000000]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    args = ap.parse_args(argv)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    ctx = pgs.Context(0)
    ref = pgs.synth.dna(3, args.ref_len)
    reads, _ = pgs.synth.reads_from_ref(ref, 4, args.reads, args.read_len)
    ctx.set_reference(ref.tobytes())
    ctx.batch_upload([r.tobytes() for r in reads])
    ctx.set_option("no_f16_mirror", 1)
    runs = {"affine": lambda: ctx.affine_batch_run(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0),
            "linear": lambda: ctx.batch_run(flags=pgs.capi.SCORE_ONLY, raw=True),
            "affine_trace": lambda: ctx.affine_batch_trace(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0),
            "linear_trace": lambda: ctx.batch_run(raw=True)}
    t = {k: dict(kernel_us=[], total_us=[], trace_us=[]) for k in runs}
    info, cells = {}, {}
    for step in range(args.warmup + args.steps):
        for name, fn in runs.items():
            fn()
            lt = ctx.last_timings()
            if step >= args.warmup:
                t[name]["kernel_us"].append(lt["score_us"])
                t[name]["total_us"].append(lt["total_us"])
                t[name]["trace_us"].append(lt["trace_us"])
            info[name], cells[name] = ctx.last_kernel(), lt["cells"]
    line = dict(bench="affine_bench", reads=args.reads, read_len=args.read_len, ref_len=args.ref_len, steps=args.steps,
                scoring=dict(affine="3/-3/open 5/extend 1", linear="3/-3/2, option no_f16_mirror"))
    for name in ("affine", "linear"):
        k_us = statistics.median(t[name]["kernel_us"])
        line[name] = dict(kernel=info[name]["name"], kernel_us=k_us, call_device_us=statistics.median(t[name]["total_us"]),
                          cells=cells[name], tcups=cells[name] / k_us / 1.0e6, valu_ops_per_cell=info[name]["valu_ops_per_cell"],
                          chunk_len=info[name]["chunk_len"], warm=info[name]["warm"])
    line["tcups_ratio_affine_to_linear"] = line["affine"]["tcups"] / line["linear"]["tcups"]
    line["model_ratio"] = line["linear"]["valu_ops_per_cell"] / line["affine"]["valu_ops_per_cell"]
    # the traceback: the trace kernel's own time ([2]) and the call's device time, next to the score-only affine call above and to
    # the linear engine's [2] (traceback windows + walks) for the same batch without SCORE_ONLY
    for name in ("affine_trace", "linear_trace"):
        line[name] = dict(trace_kernel_us=statistics.median(t[name]["trace_us"]), sweep_us=statistics.median(t[name]["kernel_us"]),
                          call_device_us=statistics.median(t[name]["total_us"]))
    line["trace_us_ratio_affine_to_linear"] = line["affine_trace"]["trace_kernel_us"] / max(line["linear_trace"]["trace_kernel_us"], 1e-9)
    line["affine_trace_share_of_call"] = line["affine_trace"]["trace_kernel_us"] / max(line["affine_trace"]["call_device_us"], 1e-9)
    ctx.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
