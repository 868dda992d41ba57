#!/usr/bin/env python3
"""Prints what the affine pairs calls of this checkout compute and report for one seeded workload, one JSON line per call and no
times: the SHA-256 of every output array, mi355_sw_last_path, every field of mi355_sw_last_kernel, and the launches and cells of
mi355_sw_last_timings.  Two checkouts whose outputs are equal as files behave alike on this workload (a refactor of the host path:
profiles/affine_pairs_host_dump_*.jsonl).

The workload: 3000 pairs of reads of 1, 37, 75, 150, 250, 512 and 513 rows and an empty query, drawn from the first 200 kbp of a
1.2 Mbp reference (the one window beyond 2^20 columns, of a 37-row read, needs the length), with flanks of 20..300 columns; for the
banded calls bands of 9, 33, 100 and 300 diagonals, bands that cover the matrix and bands that miss it.  Each of local, end-to-end
and banded runs as run and as trace, on the default dispatch and under its A/B option; two calls that must be refused close the list.

    python tools/affine_pairs_dump.py > dump.jsonl
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

pgs = bench.load_package()

SCORING = dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0)
LENS = (1, 37, 150, 512, 513, 75, 250, 0)
NPAIRS, REF_LEN, READS_FROM = 3000, 1_200_000, 200_000


def workload():
    ref = pgs.synth.dna(4711, REF_LEN)
    reads, offs = [], []
    for k in range(64):
        m = LENS[k % len(LENS)]
        x, off = pgs.synth.read_from_ref(ref[:READS_FROM], 4800 + k, m) if m else (np.zeros(0, dtype=np.uint8), 1000 + k)
        reads.append(x.tobytes())
        offs.append(off)
    r = pgs.synth.splitmix64(4999, NPAIRS)
    q, left, right, blo, bhi = [], [], [], [], []
    for k in range(NPAIRS):
        i = int(r[k] % np.uint64(len(reads)))
        m, fl = len(reads[i]), (20, 50, 100, 300)[int((r[k] >> np.uint64(8)) % np.uint64(4))]
        lo, hi = max(0, offs[i] - fl), min(REF_LEN, offs[i] + m + fl)
        if k == 1234:                                                  # a 37-row read against more than 2^20 columns
            i = 1
            lo, hi = 0, (1 << 20) + 5
        n, d = hi - lo, offs[i] - lo                                   # the read's own diagonal
        W = (None, 0, 9, 33, 100, 300)[k % 6]
        band = (-10 ** 9, 10 ** 9) if W is None else (n + 5, n + 50) if W == 0 else (d - W // 2, d - W // 2 + W - 1)
        q.append(i); left.append(lo); right.append(hi); blo.append(band[0]); bhi.append(band[1])
    return ref.tobytes(), reads, q, left, right, blo, bhi


def digest(v):
    if isinstance(v, np.ndarray):
        return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    return hashlib.sha256("\n".join(v).encode()).hexdigest()


def report(ctx, name, fn, *args, **kw):
    line = dict(call=name)
    try:
        got = fn(*args, **kw)
        line["sha256"] = {k: digest(got[k]) for k in sorted(got)}
    except pgs.MI355Error as e:
        line["error"] = [e.code, str(e)]
    t = ctx.last_timings()
    line.update(last_path=ctx.last_path(), last_kernel=ctx.last_kernel(), score_launches=t["score_launches"], cells=t["cells"])
    print(json.dumps(line, sort_keys=True), flush=True)


def main():
    ref, reads, q, left, right, blo, bhi = workload()
    ctx = pgs.Context(0)
    try:
        ctx.set_reference(ref)
        ctx.batch_upload(reads)
        for form, option, kw in (("local", "no_affine_pairs", {}), ("end_to_end", "no_affine_pairs", dict(mode="end_to_end")),
                                 ("banded", "no_affine_band", dict(band_lo=blo, band_hi=bhi))):
            for off in (0, 1):
                ctx.set_option(option, off)
                try:
                    for what, fn in (("run", ctx.affine_pairs_run), ("trace", ctx.affine_pairs_trace)):
                        report(ctx, "%s %s%s" % (form, what, " " + option if off else ""), fn, q, left, right, **kw, **SCORING)
                finally:
                    ctx.set_option(option, 0)
        # 513 rows against 200 000 columns: outside the list kernels and beyond 2^26 cells, unbanded and under a band
        report(ctx, "refused run", ctx.affine_pairs_run, [0, 4], [0, 0], [100, 200_000], **SCORING)
        report(ctx, "refused banded trace", ctx.affine_pairs_trace, [0, 4], [0, 0], [100, 200_000], band_lo=[0, 0], band_hi=[5, 50], **SCORING)
        report(ctx, "local run after the refusals", ctx.affine_pairs_run, q[:100], left[:100], right[:100], **SCORING)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
