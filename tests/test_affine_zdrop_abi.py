"""The interface of the banded extension under the z-drop stop rule (no GPU needed): mi355_sw_affine_extend_run_zdrop / _trace_zdrop
are declared in include/mi355_sw.h, the built library exports them, the header states the rule, the Python binding has the arguments,
the stop rule is a fourth mode of the one band body behind the one dispatch, and without a context every call comes back as
MI355_SW_EINVAL and writes nothing (this machine may have no device at all).  The checks of this call's own arguments — NULL bands,
a negative or NaN zdrop — need a context to be reached: here only their place in the source is pinned, in front of the first device
work; tests/test_gpu_affine_zdrop.py (test_errors_leave_the_context_usable) provokes each of them."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
SYMBOLS = ("mi355_sw_affine_extend_run_zdrop", "mi355_sw_affine_extend_trace_zdrop")
EINVAL = -22


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _flat(text):
    return re.sub(r"\s*\n \*\s*", " ", text)


def test_symbols_declared_exported_and_listed(pgs):
    header = _read(ROOT, "include", "mi355_sw.h")
    L = pgs.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*const\s+mi355_sw_extend_list\s*\*\s*list\s*,"
                         r"\s*const\s+int64_t\s*\*\s*band_lo\s*,\s*const\s+int64_t\s*\*\s*band_hi\s*,\s*float\s+zdrop\s*,"
                         r"\s*const\s+mi355_sw_affine_params\s*\*\s*params\s*,[^;]*int64_t\s*\*\s*rows_done[^;]*\)\s*;" % name, header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None
    for counter in ("zdrop_stopped", "zdrop_rows_run"):
        assert '"%s"' % counter in _read(CSRC, "mi355_sw.hip") and counter in header


def test_the_rule_is_stated_in_the_header():
    header = _read(ROOT, "include", "mi355_sw.h")
    at = header.index("banded extension with a z-drop stop rule")
    assert at > header.index("global alignment between two anchors")              # a new section behind the global one
    section = _flat(header[at:header.index("mi355_sw_affine_extend_trace_zdrop", at)])
    for needle in ("zdrop >= 0", "(B, bi, bj) = (0, 0, 0)", "0 <= j <= n", "c_i = the smallest such column", "i + band_lo > n",
                   "strictly greater", "d = |(i - bi) - (c_i - bj)|", "B - r_i - d gap_extend > zdrop", "Row m is never tested",
                   "rows_done[k] = the stop row s (1 <= s < m), or m", "on the first rows_done[k] letters of x",
                   "to_end_score = -INFINITY and to_end_y = -1", "first maximum in column-major order", "not a port",
                   "zdrop = +INFINITY: the call IS mi355_sw_affine_extend_run_band", "bands are required", "zdrop negative or NaN",
                   "zdrop < 2^24", "r_i + d gap_extend < B - floor(zdrop)", "4 398 rows", "affine_band_extz[R=..]",
                   "affine_exact_band_rows", "sw_affine_band_extz_kernel<R=..>", "zdrop_stopped", "zdrop_rows_run", "L24",
                   "no_affine_band"):
        assert needle in section, needle
    design = _read(ROOT, "DESIGN.md")
    assert re.search(r"\bL24\b", design) and design.index("L24") > design.index("L23")


def test_python_signatures(pgs):
    for name, base in (("affine_extend_zdrop_run", "affine_extend_run"), ("affine_extend_zdrop_trace", "affine_extend_trace")):
        p = inspect.signature(getattr(pgs.capi.Context, name)).parameters
        q = inspect.signature(getattr(pgs.capi.Context, base)).parameters
        assert list(p) == list(q) + ["zdrop"], name                     # the arguments of the banded call, then zdrop
        assert all(p[k].default == q[k].default for k in q if k != "self")
    p = inspect.signature(pgs.AffineSWAligner.extend_pairs_zdrop).parameters
    q = inspect.signature(pgs.AffineSWAligner.extend_pairs).parameters
    assert list(p) == list(q) + ["zdrop"] and list(p)[-2:] == ["band", "zdrop"]


def test_without_a_context_einval_and_nothing_written_and_the_checks_stand_before_the_work(pgs):
    L = pgs.capi.lib()
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    blo, bhi = (C.c_int64 * n)(-4, -4), (C.c_int64 * n)(4, 4)
    el = pgs.capi.ExtendList()
    el.npairs = n
    el.query, el.lefts, el.rights = qa, la, ra
    sc, ts = (C.c_float * n)(7, 7), (C.c_float * n)(7, 7)
    ex, ey, ty, rd = (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()
    te = (C.c_uint8 * n)(0, 1)
    for lst in (C.byref(el), None):                                   # without a context every call is EINVAL
        for lo, hi in ((blo, bhi), (None, None), (blo, None)):
            for z in (20.0, -1.0, float("nan"), float("inf")):
                zf = C.c_float(z)
                assert L.mi355_sw_affine_extend_run_zdrop(None, lst, lo, hi, zf, C.byref(p), sc, ex, ey, ts, ty, rd) == EINVAL
                assert L.mi355_sw_affine_extend_run_zdrop(None, lst, lo, hi, zf, None, sc, ex, ey, None, None, None) == EINVAL
                assert L.mi355_sw_affine_extend_trace_zdrop(None, lst, lo, hi, zf, C.byref(p), te, res, ts, ty, rd) == EINVAL
    assert list(sc) == [7, 7] and list(ts) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7] and list(ty) == [7, 7] and list(rd) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)
    # the checks stand in the shared front of the extension calls, the band checks in front of the two of this call, zdrop's last
    src = _read(CSRC, "mi355_sw.hip")
    a = src.index("band_lo and band_hi must both be given, or neither")
    b = src.index("z-drop extension: band_lo and band_hi are required")
    c = src.index("z-drop extension: zdrop must be >= 0")
    d = src.index("rc = affine_extend(ctx, ctx->ref, ctx->batch, el")
    assert a < b < c < d and "!(zdrop >= 0.0f)" in src[b:d]            # (a NaN fails the comparison)


def test_the_stop_rule_is_a_mode_of_the_one_band_body():
    kernel = _read(CSRC, "sw_affine_band_kernel.h")
    assert re.search(r"void sw_affine_band_extz_kernel\([^)]*\)\s*\{\s*using MODE = AffineBandExtZ;\s*#include \"sw_affine_band_body\.inc\"\s*\}", kernel)
    assert re.search(r"struct\s+AffineBandExtZ\s*:\s*AffineBandExt\s*\{\s*static constexpr bool kZdrop = true;\s*\};", kernel)
    assert kernel.count("static constexpr bool kZdrop = false;") == 3           # a line of its own in each of the three other modes
    body = _read(CSRC, "sw_affine_band_body.inc")
    loop = body[body.index("for (int it = 0; it < steps; ++it) {"):]
    assert "if (__builtin_amdgcn_ballot_w64(zstop == 0 && row < m) == 0) { zrun = row; break; }" in loop
    assert "__syncthreads" not in loop and "while" not in loop           # a bounded loop with a break, no barrier in or behind it
    assert "(uint32_t)j <= (uint32_t)n" in loop                          # padding columns are masked out of the row maximum
    host = _read(CSRC, "host_affine.h")
    m = re.search(r"struct\s+AffineBandExtZMode\s*\{(.*?)\n\};", host, re.S)
    assert m and re.search(r"return\s+&sw_affine_band_extz_kernel<R>\s*;", m.group(1)) and "affine_band_extz[R=%d]" in m.group(1)
    assert re.search(r"affine_list_stage\(AffineBandFamily<AffineBandExtZMode>\{", host)
    assert len(re.findall(r"\bint affine_extend\(", host)) == 1          # the extension itself takes the z-drop: no copy
    fill = _read(CSRC, "sw_affine_kernel.h")
    assert re.search(r"affine_exact_fill_model<false,\s*kAffineModelExt,\s*true,\s*true>", fill) and "sw_affine_exact_rows_band_kernel" in fill
    assert "affine_exact_band_rows" in host and "kAffineExactRowsMax = 4398" in host
