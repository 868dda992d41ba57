"""The interface of the anchored seed extension inside a diagonal band (no GPU needed): mi355_sw_affine_extend_run_band / _trace_band
are declared in include/mi355_sw.h, the built library exports the symbols, the header states the model, the Python binding has the
arguments, every instance of the band kernel has its extension sibling behind one dispatch, and an argument error — no context —
comes back as MI355_SW_EINVAL before any device work and writes nothing (this machine may have no device at all)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
SYMBOLS = ("mi355_sw_affine_extend_run_band", "mi355_sw_affine_extend_trace_band")
EINVAL = -22


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _header():
    return _read(ROOT, "include", "mi355_sw.h")


def _flat(text):
    return re.sub(r"\s*\n \*\s*", " ", text)


def test_symbols_declared_and_exported(pgs):
    header = _header()
    L = pgs.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*const\s+mi355_sw_extend_list\s*\*\s*list\s*,"
                         r"\s*const\s+int64_t\s*\*\s*band_lo\s*,\s*const\s+int64_t\s*\*\s*band_hi\s*,"
                         r"\s*const\s+mi355_sw_affine_params\s*\*\s*params\s*," % name, header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None
    # the list's layout is the unbanded call's: the bands are arguments, not fields
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mi355_sw_extend_list\s*;", header)
    assert m and "band" not in m.group(1)
    assert [f[0] for f in pgs.capi.ExtendList._fields_] == ["npairs", "query", "q_lo", "q_hi", "lefts", "rights", "backward"]


def test_the_model_is_stated_in_the_header():
    header = _header()
    at = header.index("anchored seed extension inside a diagonal band")
    assert at > header.index("anchored seed extension, forward and backward")     # a new section after the anchored one
    section = _flat(header[at:header.index("mi355_sw_affine_extend_trace_band", at)])
    for needle in ("band_lo[k] <= j - i <= band_hi[k]", "band_lo <= 0 <= band_hi", "H = E = F = -infinity", "because the model has no floor",
                   "band_lo <= n - m", "to_end_score = -INFINITY and to_end_y = -1", "the host fills it in",
                   "lo_e = max(band_lo, -m), hi_e = min(band_hi, n), W = hi_e - lo_e + 1", "clipped to min(n, m + hi_e) columns",
                   "a rows + 3 gap_open + (W + 1) gap_extend - smin < 2^24", "smax (rows + 1) < 2^18",
                   "affine_band_ext[R=..]", "affine_exact_band", "sw_affine_band_ext_kernel<R=..>", "L22",
                   "score -INFINITY, end 0 / 0, pos 0 and empty strings", "never runs on an unbanded kernel", "no_affine_band"):
        assert needle in section, needle
    design = _read(ROOT, "DESIGN.md")
    assert re.search(r"\bL22\b", design) and design.index("L22") > design.index("L21")


def test_python_signatures(pgs):
    for name, lead in (("affine_extend_run", ()), ("affine_extend_trace", ("to_end",))):
        p = inspect.signature(getattr(pgs.capi.Context, name)).parameters
        names = list(p)
        assert names[:7] == ["self", "query", "lefts", "rights", "q_lo", "q_hi", "backward"], name
        assert names[-2:] == ["band_lo", "band_hi"], name                # after every argument the call had
        assert names[7:-2] == ["match", "mismatch", "gap_open", "gap_extend", "lut"] + list(lead), name
        assert p["band_lo"].default is None and p["band_hi"].default is None
    p = inspect.signature(pgs.AffineSWAligner.extend_pairs).parameters
    assert list(p)[:6] == ["query", "lefts", "rights", "q_lo", "q_hi", "backward"]
    assert list(p)[-1] == "band" and p["band"].default is None
    assert p["traceback"].default is False and p["to_end"].default is None and p["context"].default is None


def test_argument_errors_come_before_any_device_work(pgs):
    L = pgs.capi.lib()
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    blo, bhi = (C.c_int64 * n)(-4, -4), (C.c_int64 * n)(4, 4)
    el = pgs.capi.ExtendList()
    el.npairs = n
    el.query, el.lefts, el.rights = qa, la, ra
    sc, ts = (C.c_float * n)(7, 7), (C.c_float * n)(7, 7)
    ex, ey, ty = (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()
    te = (C.c_uint8 * n)(0, 1)
    for lst in (C.byref(el), None):                                   # without a context every call is EINVAL
        for lo, hi in ((blo, bhi), (None, None), (blo, None), (None, bhi)):
            assert L.mi355_sw_affine_extend_run_band(None, lst, lo, hi, C.byref(p), sc, ex, ey, ts, ty) == EINVAL
            assert L.mi355_sw_affine_extend_run_band(None, lst, lo, hi, None, sc, ex, ey, None, None) == EINVAL
            assert L.mi355_sw_affine_extend_trace_band(None, lst, lo, hi, C.byref(p), te, res, ts, ty) == EINVAL
            assert L.mi355_sw_affine_extend_trace_band(None, lst, lo, hi, C.byref(p), None, res, None, None) == EINVAL
    assert list(sc) == [7, 7] and list(ts) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7] and list(ty) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)


def test_every_band_instance_has_its_extension_sibling():
    kernel = _read(CSRC, "sw_affine_band_kernel.h")
    assert re.search(r"template\s*<\s*int\s+R\s*>\s*__global__[^\n]*\bsw_affine_band_ext_kernel\(", kernel)
    assert re.search(r"template\s*<\s*int\s+R\s*>\s*__global__[^\n]*\bsw_affine_band_kernel\(", kernel)   # an entry point of its own, not a flag
    # each entry point only names its mode and includes the one body; the extension's traits: no floor, the key, the row-m fold, two results
    for name, mode in (("sw_affine_band_kernel", "AffineBandLocal"), ("sw_affine_band_ext_kernel", "AffineBandExt")):
        assert re.search(r"void %s\([^)]*\)\s*\{\s*using MODE = %s;\s*#include \"sw_affine_band_body\.inc\"\s*\}" % (name, mode), kernel), name
    m = re.search(r"struct\s+AffineBandExt\s*\{(.*?)\n\};", kernel, re.S)
    assert m and re.search(r"kFloor = false, kKey = true, kRowM = true, kCorner = false;", m.group(1)) and re.search(r"kOuts = 2;", m.group(1))
    m = re.search(r"struct\s+AffineBandLocal\s*\{(.*?)\n\};", kernel, re.S)
    assert m and re.search(r"kFloor = true, kKey = true, kRowM = false, kCorner = false;", m.group(1)) and re.search(r"kOuts = 1;", m.group(1))
    assert len(re.findall(r"constexpr\s+int\s+kBandR\[\]", kernel)) == 1
    host = _read(CSRC, "host_affine.h")
    # one dispatch over kBandR (the band family's) asks the mode for the instance of an R; the extension mode names its kernel once
    assert len(re.findall(r"with_listed_R<kBandR>\(R,[^;]*M::template kernel<decltype\(r\)::value>\(c\)", host, re.S)) == 1
    m = re.search(r"struct\s+AffineBandExtMode\s*\{(.*?)\n\};", host, re.S)
    assert m and re.search(r"template\s*<\s*int\s+R\s*>[^;]*return\s+&sw_affine_band_ext_kernel<R>\s*;", m.group(1))
    assert host.count("sw_affine_band_ext_kernel<") == 2             # that pick and the kernel's name
    assert re.search(r"affine_list_stage\(AffineBandFamily<AffineBandExtMode>\{", host) and "affine_band_ext[R=%d]" in host
    assert re.search(r"kOuts\s*=\s*2\s*;.*?keep_all\(const AffineCall &\)\s*\{\s*return\s+true;", m.group(1), re.S)
    assert "affine_band_ext_exact" in host and re.search(r"bool\s+affine_ext_exact\(", host)
    # the anchored model under a band is an instance of the exact fill; the end-to-end guard stays
    fill = _read(CSRC, "sw_affine_kernel.h")
    assert "the banded end-to-end model is not defined" in fill
    assert "sw_affine_exact_ext_band_kernel" in fill and "sw_affine_trace_ext_band_kernel" in fill
    assert re.search(r"affine_exact_fill_model<false,\s*kAffineModelExt,\s*true>", fill)
    assert re.search(r"affine_trace_body<kAffineModelExt,\s*true>", fill)
