#!/usr/bin/env python3
"""One process of tests/test_gpu_big_batch.py: MI355_SW_POOL_THREADS is read once per process, so every value of it is a fresh one.
usage: big_batch_worker.py N CONFIG     (CONFIG: a key of big_batch_cases.CONFIGS; the variable comes with the environment)
On one context, for each of the three routes (result objects, the struct-of-arrays view with its strings, the view without
traceback): a call on the batch that PRECEDES the checked one, then the checked call, every field of every item against the oracle.
Prints ONE line of JSON: {"n", "config", "value", "routes": {route: {"mismatches", "examples", "path", "counters", "seconds"}}}."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import big_batch_cases as bb  # noqa: E402
from conftest import load_package  # noqa: E402
from oracle import binding as ob  # noqa: E402


def call(ctx, pgs, route, xs, sc):
    """One call of `route` on the batch xs; the results as a list of dicts (the fields the route delivers)."""
    kw = dict(semantics=0, match=sc[0], mismatch=sc[1], gap=sc[2])
    if route == "objects":
        got = ctx.align_batch(xs, **kw)
        return got, ctx.last_path(), ctx.last_counters()
    ctx.batch_upload(xs)
    raw = ctx.batch_run(raw=True, flags=pgs.capi.SCORE_ONLY if route == "score_view" else 0, **kw)
    path, counters = ctx.last_path(), ctx.last_counters()
    n = len(xs)
    score, pos, ex, ey = raw["score"].tolist(), raw["pos"].tolist(), raw["end_x"].tolist(), raw["end_y"].tolist()
    if route == "view":
        cons = [ctx.consensus(k) for k in range(n)]
        got = [dict(score=score[k], pos=pos[k], end_x=ex[k], end_y=ey[k], cons_x=cons[k][0], cons_y=cons[k][1]) for k in range(n)]
    else:                                                            # (no traceback: pos and the strings are not made)
        got = [dict(score=score[k], end_x=ex[k], end_y=ey[k]) for k in range(n)]
    return got, path, counters


def main(argv):
    n, config = int(argv[1]), argv[2]
    options, sc = bb.CONFIGS[config][:2]
    pgs = load_package()
    y = bb.make_y()
    dictionary = bb.make_dictionary(y)
    rec = bb.oracle_records(ob, dictionary, y, sc)
    cur, prev = bb.seq(n).tolist(), bb.seq(n, bb.STRIDE).tolist()
    xs_cur, xs_prev = [dictionary[d] for d in cur], [dictionary[d] for d in prev]
    ctx = pgs.Context(0)
    for o in options:
        ctx.set_option(o)
    ctx.set_reference(y)
    out = dict(n=n, config=config, value=os.environ.get("MI355_SW_POOL_THREADS"), routes={})
    for route in bb.ROUTES:
        t0 = time.time()
        call(ctx, pgs, route, xs_prev, sc)
        got, path, counters = call(ctx, pgs, route, xs_cur, sc)
        keys = bb.KEYS if route != "score_view" else ("score", "end_x", "end_y")
        bad, examples = 0, []
        if len(got) != n:
            bad, examples = n, ["%d results for %d items" % (len(got), n)]
        else:
            for k in range(n):
                g, e = got[k], rec[cur[k]]
                for key in keys:
                    if g[key] != e[key]:
                        bad += 1
                        if len(examples) < 5:
                            examples.append("item %d (%s, |x| = %d): %s got %r expected %r" % (k, bb.CLASSES[cur[k] % 4], len(xs_cur[k]), key, g[key], e[key]))
                        break
        out["routes"][route] = dict(mismatches=bad, examples=examples, path=path, seconds=round(time.time() - t0, 3),
                                    counters={k: counters[k] for k in ("pooled_loops", "beyond_f16", "left_window")})
    ctx.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
