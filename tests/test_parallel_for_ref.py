"""csrc/host_common.h's parallel_for — the split of the per-item host loops of a big batch into parts for the worker pool — on the
CPU: the header's OWN text (from `class WorkerPool {` to the end of parallel_for) is pasted into tests/cpp/parallel_for_cover.cpp and
built with g++ as a stand-alone program, no GPU and no HIP.  MI355_SW_POOL_THREADS is read once per process, so every value of it
is a process of its own.  Per process, for the default threshold and for the one PoolFromScope sets, and for every n around the
thresholds: every item is visited exactly once, no part is called with a range outside [0, n], the parts see the caller's option
and device bindings and the pool threads get their own back, and a loop takes the pool exactly where the two thresholds say.

Before the part count was clamped in front of the step (`nt` parts of ceil(n / nt) items, of which the pool ran the first 8), the
values 9, 16, 64 and 100000 failed here and no other did: 112 of 1024 items never visited under 9, 512 of 1024 and 24 576 of
49 152 under 16, 896 of 1024 under 64, all but 24 of 200 003 under 100000 (at n = 200 000: 22 216, 100 000, 175 000, 199 984)."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "host_common.h")
HARNESS = os.path.join(ROOT, "tests", "cpp", "parallel_for_cover.cpp")

BEGIN = "class WorkerPool {"
FUNC = "template <class F>\nvoid parallel_for(size_t n, F fn) {"
END = "}  // parallel_for"
PLACE = "// @@HOST_COMMON_SLICE@@"

VALUES = (None, "1", "2", "3", "7", "8", "9", "16", "64", "100000")
NS = (0, 1, 1023, 1024, 1025, 8191, 49151, 49152, 49153, 131071, 131072, 200003)
POOL_MAX_PARTS = 8                                                   # seven workers and the caller
POOL_FROM = {"default": 131072, "scoped": 49152}                     # items from which a loop pools; with the variable set: 1024
POOL_FROM_WHEN_SET = 1024


def _slice():
    """The text under test; every marker must be there exactly once and in order, or the cut would silently move."""
    src = open(HEADER).read()
    for m in (BEGIN, FUNC, END):
        assert src.count(m) == 1, "csrc/host_common.h: marker %r occurs %d times, the test cuts by it" % (m, src.count(m))
    a, f, b = src.index(BEGIN), src.index(FUNC), src.index(END)
    assert a < f < b, "csrc/host_common.h: markers out of order"
    body = src[f + len(FUNC):b]
    assert "\n}" not in body, "csrc/host_common.h: %r no longer closes parallel_for itself" % END
    return src[a:b] + "}\n"


def _build(tmp, name, extra):
    harness = open(HARNESS).read()
    assert harness.count(PLACE) == 1
    cpp = tmp / (name + ".cpp")
    cpp.write_text(harness.replace(PLACE, _slice()))
    exe = tmp / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + extra + [str(cpp), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def cover(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("parallel_for"), "cover", [])


def _env(value):
    env = {k: v for k, v in os.environ.items() if k not in ("MI355_SW_POOL_THREADS", "MI355_SW_POOL_SPIN_US")}
    if value is not None:
        env["MI355_SW_POOL_THREADS"] = value
    return env


def _expected(value, scope, n):
    """(pooled, calls of fn): what the thresholds and the part count say."""
    if value is None:
        parts = POOL_MAX_PARTS
        pooled = n >= POOL_FROM[scope]
    else:
        parts = min(max(1, int(value)), POOL_MAX_PARTS)
        pooled = parts > 1 and n >= POOL_FROM_WHEN_SET
    return pooled, (parts if pooled else 1)


def _check(rows, value, ns, repeat=1):
    assert len(rows) == 2 * len(ns) * repeat
    seen = set()
    bad = []
    for r in rows:
        seen.add((r["scope"], r["n"]))
        assert r["pool_from"] == POOL_FROM[r["scope"]], r
        pooled, calls = _expected(value, r["scope"], r["n"])
        want = dict(missed=0, twice=0, bad_range=0, wrong_binding=0, caller_kept=1, restore_wrong=0, calls=calls,
                    pooled_loops=int(pooled))
        got = {k: r[k] for k in want}
        # a part runs on a pool thread exactly when the loop pooled: part 0 on the caller, the others off it
        if got != want or r["off_caller"] != calls - 1:
            bad.append((r["scope"], r["n"], {k: (got[k], want[k]) for k in want if got[k] != want[k]}, "off_caller %d" % r["off_caller"]))
    assert seen == {(s, n) for s in POOL_FROM for n in ns}
    assert not bad, "MI355_SW_POOL_THREADS=%s: (scope, n, {field: (got, expected)}) %r" % (value, bad)


@pytest.mark.parametrize("value", VALUES, ids=lambda v: "unset" if v is None else v)
def test_every_item_once(cover, value):
    r = subprocess.run([cover] + [str(n) for n in NS], env=_env(value), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    _check([json.loads(line) for line in r.stdout.splitlines()], value, NS)


def test_thresholds_are_the_documented_ones():
    """What _expected restates is what the header and INTEGRATION.md say."""
    src = open(HEADER).read()
    assert "thread_local size_t tl_pool_from = %d;" % POOL_FROM["default"] in src
    assert "PoolFromScope() { tl_pool_from = %d; }" % POOL_FROM["scoped"] in src
    assert "static constexpr int kMaxParts = %d;" % POOL_MAX_PARTS in src
    assert "n < %d) { fn((size_t)0, n); return; }" % POOL_FROM_WHEN_SET in src


def test_split_under_thread_sanitizer(tmp_path):
    """The same program with -fsanitize=thread, 16 parts asked for, the three n around the pooled threshold, twenty times over
    (stand-alone binary, nothing preloaded; the recipe of tests/test_abi.py::test_worker_pool_under_thread_sanitizer)."""
    exe = _build(tmp_path, "cover_tsan", ["-fsanitize=thread"])
    ns, repeat = (49151, 49152, 49153), 20
    # the child runs without address-space randomisation (ADDR_NO_RANDOMIZE, as `setarch -R`): on kernels that randomise
    # mappings with more bits than this TSAN runtime knows, it otherwise stops with "unexpected memory mapping"
    personality = C.CDLL(None, use_errno=True).personality
    personality.argtypes, personality.restype = [C.c_ulong], C.c_int
    r = subprocess.run([exe, "--repeat", str(repeat)] + [str(n) for n in ns], env=_env("16"), capture_output=True, text=True, timeout=300,
                       preexec_fn=lambda: personality(personality(0xFFFFFFFF) | 0x0040000))
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    _check([json.loads(line) for line in r.stdout.splitlines()], "16", ns, repeat)
