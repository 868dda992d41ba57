"""Big batches of small alignments on the worker pool: every item once, at any part count.

From 49 152 items (or from 1024 when MI355_SW_POOL_THREADS is set) the per-item host loops behind the kernels — the defaults, the
device-built and the host-built lists' results, the result objects, the view — run as parts on csrc/host_common.h's worker pool.
Here NO item is left out: score, pos, end_x, end_y and both strings of every index against the oracle (score, end_x, end_y on the
route without traceback), on the three routes of tests/stress_small_batches.py, under every configuration of
tests/big_batch_cases.py (each asserted from the call's path and counters to have ENGAGED), one below and one above the threshold
with the variable unset, and at 1, 3, 8, 16 and 64 parts.  Every checked call follows a call on the same context whose results differ
at every index (tests/test_big_batch_ref.py), so an item that a loop skips shows what the call before left there.

The variable is read once per process: each (value, N, configuration) is a fresh child (tests/big_batch_worker.py, all three routes
in it), started with subprocess.run, one after another; the children are shared by the tests of the routes.  After a child that
ended by a signal, by an abort or at its timeout no further child is started, and what is left fails with that reason."""
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_batch_cases as bb  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "big_batch_worker.py")

_children = {}                                                       # (value, n, config) -> the child's JSON, or the reason there is none
_stopped = []                                                        # why no further child is started (a child died or hung)

CASES = [(v, n, c, r) for v, n, configs in bb.PLAN for c in configs for r in bb.ROUTES]


def _child(value, n, config):
    key = (value, n, config)
    if key in _children:
        return _children[key]
    if _stopped:
        pytest.fail("not started: " + _stopped[0], pytrace=False)
    env = {k: v for k, v in os.environ.items() if k != "MI355_SW_POOL_THREADS"}
    if value is not None:
        env["MI355_SW_POOL_THREADS"] = value
    what = "big_batch_worker.py %d %s under MI355_SW_POOL_THREADS=%s" % (n, config, value)
    limit = 120 if n > 40000 else 60                                 # (seconds; a child takes 2 to 6)
    try:
        r = subprocess.run([sys.executable, WORKER, str(n), config], env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _stopped.append("%s did not end within %d s" % (what, limit))
        _children[key] = _stopped[0]
        pytest.fail(_stopped[0], pytrace=False)
    if r.returncode < 0 or r.returncode in (134, 139):
        _stopped.append("%s ended with status %d: %s" % (what, r.returncode, r.stderr[-1500:]))
        _children[key] = _stopped[0]
        pytest.fail(_stopped[0], pytrace=False)
    lines = [line for line in r.stdout.splitlines() if line.startswith("{")]
    if r.returncode != 0 or len(lines) != 1:
        _children[key] = "%s failed with status %d: %s" % (what, r.returncode, (r.stdout + r.stderr)[-1500:])
    else:
        _children[key] = json.loads(lines[0])
    return _children[key]


@pytest.mark.parametrize("value,n,config,route", CASES,
                         ids=["%s-%d-%s-%s" % ("unset" if v is None else v, n, c, r) for v, n, c, r in CASES])
def test_every_item_of_a_big_batch(value, n, config, route):
    out = _child(value, n, config)
    assert isinstance(out, dict), out
    assert (out["n"], out["config"], out["value"]) == (n, config, value)
    got = out["routes"][route]
    print("%s N=%d %s %s: %d mismatches, %.3f s, counters %r, path %s"
          % (value, n, config, route, got["mismatches"], got["seconds"], got["counters"], " ".join(got["path"])))
    assert got["mismatches"] == 0, "%d of %d items differ from the oracle: %s" % (got["mismatches"], n, "; ".join(got["examples"]))
    # the path the case is about engaged
    path = " ".join(got["path"])
    _, _, must, must_not = bb.CONFIGS[config]
    for pat in must:
        assert re.search(pat, path), (pat, path)
    for pat in must_not:
        assert not re.search(pat, path), (pat, path)
    pooled = got["counters"]["pooled_loops"]
    if bb.expect_pooled(value, n):
        assert pooled >= 1, got["counters"]
    else:
        assert pooled == 0, got["counters"]
    if config == "beyond":                                           # items the float16 pass left undecided, handled later among the others
        assert got["counters"]["beyond_f16"] >= 1, got["counters"]
