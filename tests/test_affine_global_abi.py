"""The interface of the global alignment between two anchors (no GPU needed): mi355_sw_affine_global_run / _trace are declared in
include/mi355_sw.h, the built library exports the symbols, the header states the model and the admission test of lemma L23, the Python
binding has the arguments, every instance of the pair kernel and of the band kernel has its global sibling behind one dispatch, and an
argument error — no context — comes back as MI355_SW_EINVAL before any device work and writes nothing (this machine may have no device
at all)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
SYMBOLS = ("mi355_sw_affine_global_run", "mi355_sw_affine_global_trace")
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
    for name, last in zip(SYMBOLS, (r"float\s*\*\s*score", r"mi355_sw_result\s*\*\s*outs")):
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*const\s+mi355_sw_extend_list\s*\*\s*list\s*,"
                         r"\s*const\s+int64_t\s*\*\s*band_lo\s*,\s*const\s+int64_t\s*\*\s*band_hi\s*,"
                         r"\s*const\s+mi355_sw_affine_params\s*\*\s*params\s*,\s*%s\s*\)\s*;" % (name, last), header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None
    # two calls with bands as arguments, not four symbols; the list and the mode enum stay what they were
    assert not re.search(r"mi355_sw_affine_global_\w+_band", header)
    assert [f[0] for f in pgs.capi.ExtendList._fields_] == ["npairs", "query", "q_lo", "q_hi", "lefts", "rights", "backward"]
    assert pgs.capi.AFFINE_MODES == {"local": 0, "end_to_end": 1}


def test_the_model_is_stated_in_the_header():
    header = _header()
    at = header.index("global alignment between two anchors")
    assert at > header.index("anchored seed extension inside a diagonal band")      # a new section after the banded extension
    section = _flat(header[at:header.index("mi355_sw_affine_global_trace", at)])
    for needle in ("H(m, n)", "end_x = m and end_y = n always", "band_lo <= n - m <= band_hi", "score = -INFINITY",
                   "score -INFINITY, end 0 / 0, pos 0 and empty strings", "no kernel runs for such a pair",
                   "m = 0, n = 0: score 0", "m >= 1, n = 0: score -(o + (m-1) e)", "m = 0, n >= 1: score -(o + (n-1) e)",
                   "n = 0 needs band_lo <= -m, and m = 0 needs band_hi >= n", "lo_e = max(band_lo, -m), hi_e = min(band_hi, n), W = hi_e - lo_e + 1",
                   "stops at (0,0) and nowhere else", "pos = 1 when n >= 1, else 0",
                   "affine_pair_glob[R=..]", "affine_band_glob[R=..]", "affine_exact_band", "affine_trace",
                   "sw_affine_pair_glob_kernel<R=..>", "sw_affine_band_glob_kernel<R=..>", "L23",
                   "3 gap_open + (rows + columns) gap_extend - smin < 2^24 and smax rows + gap_open < 2^24",
                   "a rows + 3 gap_open + (W + 1) gap_extend - smin < 2^24 and smax rows + gap_open < 2^24",
                   "The kernels form no key", "never runs on an unbanded kernel", "no_affine_pairs", "no_affine_band"):
        assert needle in section, needle
    assert "2^18 does not apply" in section                        # L23 dropped the key inequality: say so where the others state it
    design = _read(ROOT, "DESIGN.md")
    assert re.search(r"\bL23\b", design) and design.index("L23") > design.index("L22")


def test_python_signatures(pgs):
    for name in ("affine_global_run", "affine_global_trace"):
        p = inspect.signature(getattr(pgs.capi.Context, name)).parameters
        assert list(p) == ["self", "query", "lefts", "rights", "q_lo", "q_hi", "backward", "match", "mismatch", "gap_open", "gap_extend", "lut",
                           "band_lo", "band_hi"], name
        assert [p[k].default for k in ("q_lo", "q_hi", "backward", "lut", "band_lo", "band_hi")] == [None] * 6
        assert [p[k].default for k in ("match", "mismatch", "gap_open", "gap_extend")] == [3.0, -3.0, 5.0, 1.0]
    p = inspect.signature(pgs.AffineSWAligner.global_pairs).parameters
    assert list(p)[:6] == ["query", "lefts", "rights", "q_lo", "q_hi", "backward"]
    assert list(p)[-3:] == ["traceback", "context", "band"]
    assert p["traceback"].default is False and p["context"].default is None and p["band"].default is None
    assert list(p)[6:-3] == list(inspect.signature(pgs.AffineSWAligner.extend_pairs).parameters)[6:11]


def test_argument_errors_come_before_any_device_work(pgs):
    L = pgs.capi.lib()
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    blo, bhi = (C.c_int64 * n)(-4, -4), (C.c_int64 * n)(4, 4)
    el = pgs.capi.ExtendList()
    el.npairs = n
    el.query, el.lefts, el.rights = qa, la, ra
    sc = (C.c_float * n)(7, 7)
    res = (pgs.capi.Result * n)()
    for lst in (C.byref(el), None):                                   # without a context every call is EINVAL
        for lo, hi in ((blo, bhi), (None, None), (blo, None), (None, bhi)):
            for par in (C.byref(p), None):
                assert L.mi355_sw_affine_global_run(None, lst, lo, hi, par, sc) == EINVAL
                assert L.mi355_sw_affine_global_run(None, lst, lo, hi, par, None) == EINVAL
                assert L.mi355_sw_affine_global_trace(None, lst, lo, hi, par, res) == EINVAL
                assert L.mi355_sw_affine_global_trace(None, lst, lo, hi, par, None) == EINVAL
    assert list(sc) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)


def test_every_instance_has_its_global_sibling():
    pair, band = _read(CSRC, "sw_affine_pair_kernel.h"), _read(CSRC, "sw_affine_band_kernel.h")
    for text, names in ((pair, ("sw_affine_pair_glob_kernel", "sw_affine_pair_ext_kernel", "sw_affine_pair_e2e_kernel", "sw_affine_pair_kernel")),
                        (band, ("sw_affine_band_glob_kernel", "sw_affine_band_ext_kernel", "sw_affine_band_kernel"))):
        for name in names:                                            # entry points of their own, not flags
            assert re.search(r"template\s*<\s*int\s+R\s*>\s*__global__[^\n]*\b%s\(" % name, text), name
    assert len(re.findall(r"constexpr\s+int\s+kPairR\[\]", pair)) == 1 and len(re.findall(r"constexpr\s+int\s+kBandR\[\]", band)) == 1

    def code(name):                                                   # a body file without its comments
        return re.sub(r"//[^\n]*", "", _read(CSRC, name))
    def mode(text, name):
        m = re.search(r"struct\s+%s\s*\{(.*?)\n\};" % name, text, re.S)
        assert m, name
        return m.group(1)
    # the global entry points only name their mode and include the one body of their geometry
    for text, name, md, inc in ((pair, "sw_affine_pair_glob_kernel", "AffinePairGlob", "sw_affine_pair_body.inc"),
                                (band, "sw_affine_band_glob_kernel", "AffineBandGlob", "sw_affine_band_body.inc")):
        assert re.search(r"void %s\([^)]*\)\s*\{\s*using MODE = %s;\s*#include \"%s\"\s*\}" % (name, md, re.escape(inc)), text), name
    # the global modes' traits: no key, no floor, no row-m fold; the corner and one result
    assert re.search(r"kRow0 = true, kKey = false, kRowM = false, kCorner = true;", mode(pair, "AffinePairGlob")) and "kOuts = 1;" in mode(pair, "AffinePairGlob")
    assert re.search(r"kFloor = false, kKey = false, kRowM = false, kCorner = true;", mode(band, "AffineBandGlob")) and "kOuts = 1;" in mode(band, "AffineBandGlob")
    # the key, the floors and the folds of the bodies stand under exactly those traits: no key, no fold ...
    pb, bb = code("sw_affine_pair_body.inc"), code("sw_affine_band_body.inc")
    assert pb.count("WaveKeyFold") == 1 and pb.count("slot_first_max") == 1 and bb.count("WaveKeyFold") == 1 and bb.count("slot_first_max") == 1
    assert re.search(r"if constexpr \(MODE::kKey\) \{\s*asm\(\"v_max_f32 %0, 0, %1\" : \"=v\"\(hp\) : \"v\"\(h\)\);\s*WaveKeyFold::cell<R>\(r, hp, mx, tpend\);\s*\}", pb)
    assert re.search(r"if constexpr \(MODE::kKey\) WaveKeyFold::cell<R>\(r, MODE::kFloor \? h : fmaxf\(h, 0\.0f\), mx, tpend\);", bb)
    for b in (pb, bb):
        assert re.search(r"if constexpr \(MODE::kKey\) \{[^}]*\{[^}]*\}[^}]*slot_first_max\(bv, bi, bj\);\s*\}", b)
        assert re.search(r"static_assert\(MODE::kOuts == \(MODE::kKey \? 1 : 0\) \+ \(MODE::kRowM \? 1 : 0\) \+ \(MODE::kCorner \? 1 : 0\)", b)
    # ... no floor, in the cell or on the answer: the pair body has none in the cell at all, the band body's stands under kFloor
    assert not re.search(r"v_add_f32_e64|fmed3f|clamp", pb) and pb.count("v_max_f32 %0, 0,") == 1
    assert bb.count("fmed3f") == 1 and "MODE::kFloor ? __builtin_amdgcn_fmed3f(Ho[r] + s, 0.0f, 1.0f) : Ho[r] + s;" in bb and bb.count("fmaxf(h, 0.0f)") == 1
    # ... the row-m fold under kRowM
    assert re.search(r"if constexpr \(MODE::kRowM\) \{\s*const bool take_e = hm > best;", pb) and pb.count("hm > best") == 1
    assert re.search(r"if constexpr \(MODE::kRowM\) \{\s*#pragma unroll\s*for \(int r = 0; r < R; \+\+r\) \{\s*const int j = col0 \+ it \+ r;", bb) and bb.count("h > eval") == 1
    # the capture statements, under the corner's trait, and the one result where a problem's last result goes
    assert "if constexpr (kSelM) hm = wsel[r] ? h : hm;" in pb and "constexpr bool kSelM = MODE::kRowM || MODE::kCorner;" in pb
    assert "if constexpr (MODE::kCorner) corner = t == tcap ? hm : corner;" in pb and "const int tcap = n - 1;" in pb
    assert "if (it + 1 == m)" in bb and "n - m - lo" in bb
    assert re.search(r"if constexpr \(MODE::kCorner\) \{\s*#pragma unroll\s*for \(int r = 0; r < R; \+\+r\) corner = dsel == r \? Ho\[r\] \+ ov : corner;", bb)
    for b in (pb, bb):
        assert "sa.best[NO * (size_t)pid + NO - 1] =" in b and "constexpr size_t NO = MODE::kOuts;" in b

    host = _read(CSRC, "host_affine.h")
    # one dispatch over kPairR and one over kBandR (the two families') ask the mode for the instance of an R; each global name is
    # picked in exactly one place and named in exactly one
    assert len(re.findall(r"with_listed_R<kPairR>\(R,[^;]*M::template kernel<decltype\(r\)::value>\(c\)", host, re.S)) == 1
    assert len(re.findall(r"with_listed_R<kBandR>\(R,[^;]*M::template kernel<decltype\(r\)::value>\(c\)", host, re.S)) == 1
    assert host.count("sw_affine_pair_glob_kernel<") == 2 and host.count("sw_affine_band_glob_kernel<") == 2   # the pick and the name
    for fam, md, kern in (("AffinePairFamily", "AffineGlobMode", "sw_affine_pair_glob_kernel"), ("AffineBandFamily", "AffineBandGlobMode", "sw_affine_band_glob_kernel")):
        assert re.search(r"affine_list_stage\(%s<%s>\{" % (fam, md), host)
        m = mode(host, md)
        assert re.search(r"template\s*<\s*int\s+R\s*>[^;]*return\s+&%s<R>\s*;" % kern, m) and ('return "%s<R=%%d>";' % kern) in m
        assert re.search(r"kOuts\s*=\s*1\s*;.*?keep_all\(const AffineCall &\)\s*\{\s*return\s+true;", m, re.S)
    assert "affine_pair_glob[R=%d]" in host and "affine_band_glob[R=%d]" in host
    # the extension's item building and class table are shared, not copied
    assert len(re.findall(r"\brev_q_total - q\.off\[qi\]", host)) == 1 and host.count("affine_ext_item(c, el, k)") == 2
    assert host.count("affine_ext_plan(c, plan)") == 2
    # L23: no key inequality in the two admission tests; the extension's keep theirs
    for name in ("affine_glob_exact", "affine_band_glob_exact"):
        m = re.search(r"bool\s+%s\([^)]*\)\s*\{(.*?)\n\}" % name, host, re.S)
        assert m and "kAffineProfBound" not in m.group(1) and "16777216.0" in m.group(1), name
    for name in ("affine_ext_exact", "affine_band_ext_exact"):
        m = re.search(r"bool\s+%s\([^)]*\)\s*\{(.*?)\n\}" % name, host, re.S)
        assert m and "kAffineProfBound" in m.group(1), name
    # the corner is the exact fill's own result for a fourth model constant; there is no new trace kernel
    fill = _read(CSRC, "sw_affine_kernel.h")
    assert "kAffineModelGlob = 3" in fill and re.search(r"affine_exact_fill_model<false,\s*kAffineModelGlob,\s*BAND>", fill)
    assert "the banded end-to-end model is not defined" in fill
    assert len(re.findall(r"__global__[^\n]*\bsw_affine_trace\w*kernel\(", fill)) == 3
