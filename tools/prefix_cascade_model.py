"""CPU model of the prefix filter's heights (prefix_chain): how many reads of a batch a row-P pass of P rows cannot
certify, for each listed start height and both folds (slack 0: row P folded at every step; slack (MK - 1) g = 6: every 4th step).

Two parts, numpy only (one maximum.accumulate per matrix row):
  * background flags: `--prefixes` random `--prefix-len`-letter prefixes against `--bg-len` columns of uniform DNA.  For every
    P and every x, the sub-chunks (E = 256 columns) whose row-P maximum reaches smax P - x, scaled to the reference length, as a
    mean per read.  x = deficit + slack with deficit = smax m - B0: the threshold of a read is T = smax P - x;
  * deficits of a batch: every read of the bench batch (synth.reads_from_ref(dna(3, ref), 4, reads, m)) scored exactly against the
    window at its origin.
A read is predicted to offend at (P, slack) when its threshold is not positive above the bound (x >= smax P, or the alignment cannot
end below row P) or when the expected number of background flags at its x exceeds the per-query cap (64).  `thin`: per start height,
what the thin stage (P2 = 38) takes off that — the reads it rescues, its items and a bound on its survivors.  Prints ONE JSON line.

    python tools/prefix_cascade_model.py [--bg-len 5000000 --prefixes 10 --ref-len 50000000 --reads 2048 --read-len 150]

--heights takes the prefix rows P to model (default: twice the rows per lane above); with it the line also carries `flows`: the rows
swept per batch, a full sweep counted as read-len rows, by a chain that starts at P[i] with one second pass at P[j]
(sw_prefix_kernel's heights: --heights 18,20,22,24,26,28,30,32,38, slack 0).

--per-read takes sets of prefix rows, ';' between the sets (their union goes to --heights): the seeded flow (prefix_seeded), where B0
is known before any sweep and every read takes the lowest height of the set that can certify it — `per_read`: flags by deficit, rows
swept per read, reads per height (--per-read "26,32,38;16,20,26,32,38" --heights 16,20,26,32,38).

--certify adds `certify`: the reads of the batch that lemma L21 settles from the windows of their seed hits (floor(d / min(g, smax))
below the read's seeds in the table) and the heights the residual reads take (of the last --per-read set, else of --heights).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUB = 256
CAP = 64
MATCH, MISMATCH, GAP = 3.0, -3.0, 2.0
THIN_P2 = 38                                                         # kThinP2 of host_score.h
HEIGHTS = (11, 12, 13, 14, 16, 19)                                   # rows per lane: P = 2 R (13, 16, 19 are compiled)


def rows(x, y, keep):
    """Rows `keep` (1-based) of the local-alignment matrix of x against y, linear gaps: {row: values by column}."""
    ys = np.frombuffer(y, dtype=np.uint8) if isinstance(y, bytes) else y
    n = len(ys)
    jg = GAP * np.arange(n + 1, dtype=np.float32)
    prev = np.zeros(n + 1, dtype=np.float32)
    out = {}
    for i in range(1, max(keep) + 1):
        a = np.empty(n + 1, dtype=np.float32)
        a[0] = 0.0
        np.maximum(prev[1:] - GAP, prev[:-1] + np.where(ys == x[i - 1], MATCH, MISMATCH).astype(np.float32), out=a[1:])
        np.maximum(a, 0.0, out=a)
        prev = np.maximum.accumulate(a + jg) - jg
        if i in keep:
            out[i] = prev
    return out


def background(pgs, bg_len, prefixes, prefix_len, scale, heights=None):
    """flags[P][x] = mean number of sub-chunks per read whose row-P maximum reaches smax P - x, x = 0 .. smax P, scaled by `scale`."""
    y = pgs.synth.dna(77, bg_len)
    nsub = bg_len // SUB
    flags = {}
    for k in range(prefixes):
        x = pgs.synth.dna(7700 + k, prefix_len)
        got = rows(x, y, {P for P in (heights or [2 * R for R in HEIGHTS]) if P <= prefix_len})
        for P, row in got.items():
            top = row[1:nsub * SUB + 1].reshape(nsub, SUB).max(axis=1)
            hist = np.bincount(top.astype(np.int64), minlength=int(MATCH) * P + 1)
            reach = np.cumsum(hist[::-1])                             # reach[x] = sub-chunks with maximum >= smax P - x
            flags.setdefault(P, np.zeros(int(MATCH) * P + 1))
            flags[P] += reach[:int(MATCH) * P + 1] * (scale / prefixes)
    return flags


def deficits(pgs, ref_len, reads, m):
    ref = pgs.synth.dna(3, ref_len)
    batch, offs = pgs.synth.reads_from_ref(ref, 4, reads, m)
    out = np.empty(reads, dtype=np.int64)
    for k in range(reads):
        lo, hi = max(0, int(offs[k]) - 32), min(ref_len, int(offs[k]) + m + 48)
        H = rows(batch[k], ref[lo:hi], set(range(1, m + 1)))
        out[k] = int(MATCH * m - max(float(r.max()) for r in H.values()))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--bg-len", type=int, default=5_000_000)
    ap.add_argument("--prefixes", type=int, default=10)
    ap.add_argument("--prefix-len", type=int, default=38)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--heights", type=lambda v: [int(t) for t in v.split(",")], default=None, help="prefix rows P to model, comma separated")
    ap.add_argument("--thin-cap", type=int, default=1024, help="flags a read may list for the thin stage (host_score.h thin_flag_cap)")
    ap.add_argument("--per-read", type=lambda v: [[int(t) for t in s.split(",")] for s in v.split(";")], default=None,
                    help="sets of prefix rows for a height per read, e.g. '26,32,38;16,20,26,32,38' (give the union to --heights)")
    ap.add_argument("--certify", action="store_true",
                    help="the reads settled by the windows of their seed hits (L21) and the residual reads per height (of the last --per-read set)")
    args = ap.parse_args(argv)
    import __graft_entry__ as entry
    pgs = entry._load_package()
    m = args.read_len
    flags = background(pgs, args.bg_len, args.prefixes, max([args.prefix_len] + (args.heights or [])), args.ref_len / args.bg_len, args.heights)
    d = deficits(pgs, args.ref_len, args.reads, m)
    line = dict(tool="prefix_cascade_model", bg_len=args.bg_len, prefixes=args.prefixes, ref_len=args.ref_len, reads=args.reads, read_len=m,
                cap=CAP, flags_per_read={str(P): {str(x): round(float(f[x]), 1) for x in (18, 24, 30, 36, 42) if x < len(f)} for P, f in sorted(flags.items())},
                deficit_above={str(t): int((d > t).sum()) for t in (12, 20, 26, 30, 36, 42)}, offenders={})
    for P, f in sorted(flags.items()):
        for slack in (0, 6):
            x = d + slack
            hopeless = (x >= MATCH * P) | (MATCH * m - d <= MATCH * P)
            over = np.zeros(len(d), dtype=bool)
            ok = ~hopeless
            over[ok] = f[np.minimum(x[ok], len(f) - 1)] > CAP
            line["offenders"]["P=%d,slack=%d" % (P, slack)] = dict(bound=int(hopeless.sum()), cap=int(over.sum()), total=int((hopeless | over).sum()))
    # the thin stage: a read over the cap whose flags number at most `thin_cap` is evaluated on P2 = 38 rows, flag
    # by flag, instead of offending.  Per start height P: the reads still over the thin cap, the items per thinned read (background
    # flags at the read's own deficit, the mean over the reads the stage takes) and, as a bound on what survives, the background
    # flags of row P2 at the same deficit.
    if THIN_P2 in flags:
        line["thin"] = dict(P2=THIN_P2, thin_cap=args.thin_cap)
        keep = flags[THIN_P2]
        for P, f in sorted(flags.items()):
            if P >= THIN_P2:
                continue
            ok = ~((d >= MATCH * P) | (MATCH * m - d <= MATCH * THIN_P2))
            items = f[np.minimum(d[ok], len(f) - 1)]
            take = items <= args.thin_cap
            over_cap = items > CAP
            line["thin"]["P=%d" % P] = dict(
                over_thin_cap=int((~take).sum()), rescued=int((take & over_cap).sum()), items_total=round(float(items[take].sum()), 1),
                items_per_read=round(float(items[take].mean()), 2) if take.any() else 0.0,
                items_of_rescued=round(float(items[take & over_cap].sum()), 1),
                survivors_per_read=round(float(keep[np.minimum(d[ok][take], len(keep) - 1)].mean()), 3) if take.any() else 0.0)
    if args.heights:
        # rows swept by start -> second with slack 0: everybody at P[i], the start's offenders at P[j], the second pass's on all rows
        off = {P: line["offenders"]["P=%d,slack=0" % P]["total"] for P in sorted(flags)}
        line["heights"] = sorted(flags)
        line["flows"] = {"%d->%d" % (a, b): args.reads * a + off[a] * b + off[b] * m for a in sorted(flags) for b in sorted(flags) if a < b}
        line["flows"].update({"%d" % a: args.reads * a + off[a] * m for a in sorted(flags)})
    if args.per_read:
        line["per_read"] = per_read(flags, d, m, args.per_read)
    if args.certify:
        line["certify"] = certify(pgs, flags, d, args, args.per_read[-1] if args.per_read else sorted(flags))
    print(json.dumps(line))


def certify(pgs, flags, d, args, heights):
    """Reads an intact seed must find: a read with u seeds in the table (disjoint k-mers, none periodic; k by the
    library's rule) and deficit d is settled by the windows of its hits when floor(d / min(g, smax)) < u — its hits taken to be within
    the cap, as all but a repeat's are.  The others keep their height of `heights` (per_read's rule)."""
    m = args.read_len
    k = pgs.capi.seed_k(4, m, args.ref_len)
    ref = pgs.synth.dna(3, args.ref_len)
    batch = pgs.synth.reads_from_ref(ref, 4, args.reads, m)[0]
    u = np.array([pgs.capi.seed_usable(r.tobytes(), k) for r in batch], dtype=np.int64) if k else np.zeros(len(d), dtype=np.int64)
    settled = (d // int(min(GAP, MATCH)) < u) & (u > 0)
    rest = d[~settled]
    residual = per_read(flags, rest, m, [heights]) if len(rest) else {}
    residual.pop("flags_by_deficit", None)
    return dict(k=k, seeds_per_read=dict(min=int(u.min()), max=int(u.max())), settled=int(settled.sum()), reads=len(d),
                residual_reads=int(len(rest)), residual_deficits=dict(min=int(rest.min()), max=int(rest.max())) if len(rest) else None,
                residual=residual)


def per_read(flags, d, m, height_sets):
    """The seeded flow (prefix_seeded): B0 of every read is known before any sweep, and the read takes the lowest height
    of the set whose bound its B0 clears and whose expected background flags at its deficit stay within the cap; a read no height
    takes is swept on all m rows.  Per set of heights: the expected flags by deficit, the rows swept per read, the reads per height
    and the flags (thin items, where the thin stage takes them) the passes are expected to draw."""
    out = {}
    for hs in height_sets:
        hs = [P for P in sorted(hs) if P in flags]
        rows_swept, groups, items = 0, {}, 0.0
        for dd in d:
            pick = None
            for P in hs:
                if dd >= MATCH * P or MATCH * m - dd <= MATCH * max(P, m - P):
                    continue
                f = float(flags[P][min(int(dd), len(flags[P]) - 1)])
                if f <= CAP:
                    pick = P
                    items += f
                    break
            pick = pick or m
            rows_swept += pick
            groups[pick] = groups.get(pick, 0) + 1
        out[",".join(str(P) for P in hs)] = dict(
            rows_per_read=round(rows_swept / len(d), 2), against_26=round(rows_swept / len(d) / 26.0, 3),
            reads_per_height={str(P): n for P, n in sorted(groups.items())}, expected_flags=round(items, 1))
    out["flags_by_deficit"] = {str(P): {str(x): round(float(f[x]), 1) for x in (0, 6, 12, 18, 24, 30) if x < len(f)} for P, f in sorted(flags.items())}
    return out


if __name__ == "__main__":
    main()
