"""The interface of the anchored seed extension (no GPU needed): mi355_sw_affine_extend_run / _trace and mi355_sw_extend_list are
declared in include/mi355_sw.h, the built library exports the symbols, the header states the model, the Python binding has the calls,
every instance of the pair kernel has its extension sibling behind one dispatch, the public mode enum keeps its two members, and an
argument error — no context — comes back as MI355_SW_EINVAL before any device work and writes nothing (this machine may have no
device at all)."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
SYMBOLS = ("mi355_sw_affine_extend_run", "mi355_sw_affine_extend_trace")
EINVAL = -22


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _header():
    return _read(ROOT, "include", "mi355_sw.h")


def test_symbols_declared_and_exported(pgs):
    header = _header()
    L = pgs.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*const\s+mi355_sw_extend_list\s*\*\s*list\s*,"
                         r"\s*const\s+mi355_sw_affine_params\s*\*\s*params\s*," % name, header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mi355_sw_extend_list\s*;", header)
    assert m
    fields = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", fields).strip() == ("size_t npairs; const int32_t *query; const int32_t *q_lo, *q_hi; "
                                                   "const int64_t *lefts, *rights; const uint8_t *backward;")
    # the binding's struct has the layout of the header's
    E = pgs.capi.ExtendList
    assert [f[0] for f in E._fields_] == ["npairs", "query", "q_lo", "q_hi", "lefts", "rights", "backward"]
    assert C.sizeof(E) == 7 * C.sizeof(C.c_void_p)


def test_the_model_is_stated_in_the_header():
    header = _header()
    for needle in ("H(0,j) = E(0,j) = -(o + (j-1) e)", "H(i,0) = F(i,0) = -(o + (i-1) e)", "H(0,0) = 0", "no zero floor",
                   "affine_pair_ext[R=..]", "sw_affine_pair_ext_kernel<R=..>", "the smallest such j",
                   "[q_hi - end_x, q_hi)", "[right - end_y, right)", "3 gap_open + (rows + columns) gap_extend - smin < 2^24", "L21"):
        assert needle in header, needle
    assert "reported as lengths" in re.sub(r"\s*\n \*\s*", " ", header)


def test_the_public_modes_stay_two(pgs):
    assert re.search(r"enum\s*\{\s*MI355_SW_AFFINE_LOCAL\s*=\s*0\s*,\s*MI355_SW_AFFINE_END_TO_END\s*=\s*1\s*\}", _header())
    assert pgs.capi.AFFINE_MODES == {"local": 0, "end_to_end": 1}


def test_python_signatures(pgs):
    for name, extra in (("affine_extend_run", ()), ("affine_extend_trace", ("to_end",))):
        p = inspect.signature(getattr(pgs.capi.Context, name)).parameters
        assert list(p)[:7] == ["self", "query", "lefts", "rights", "q_lo", "q_hi", "backward"], name
        for k in ("q_lo", "q_hi", "backward", "lut") + extra:
            assert p[k].default is None, (name, k)
        assert (p["match"].default, p["mismatch"].default, p["gap_open"].default, p["gap_extend"].default) == (3.0, -3.0, 5.0, 1.0)
    p = inspect.signature(pgs.AffineSWAligner.extend_pairs).parameters
    assert list(p)[:6] == ["query", "lefts", "rights", "q_lo", "q_hi", "backward"]
    assert p["traceback"].default is False and p["to_end"].default is None and p["context"].default is None


def test_argument_errors_come_before_any_device_work(pgs):
    L = pgs.capi.lib()
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    el = pgs.capi.ExtendList()
    el.npairs = n
    el.query, el.lefts, el.rights = qa, la, ra
    sc, ts = (C.c_float * n)(7, 7), (C.c_float * n)(7, 7)
    ex, ey, ty = (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()
    te = (C.c_uint8 * n)(0, 1)
    for lst in (C.byref(el), None):                                   # without a context every call is EINVAL
        assert L.mi355_sw_affine_extend_run(None, lst, C.byref(p), sc, ex, ey, ts, ty) == EINVAL
        assert L.mi355_sw_affine_extend_run(None, lst, None, sc, ex, ey, None, None) == EINVAL
        assert L.mi355_sw_affine_extend_trace(None, lst, C.byref(p), te, res, ts, ty) == EINVAL
        assert L.mi355_sw_affine_extend_trace(None, lst, C.byref(p), None, res, None, None) == EINVAL
    assert list(sc) == [7, 7] and list(ts) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7] and list(ty) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)


def test_every_instance_has_its_extension_sibling():
    kernel = _read(CSRC, "sw_affine_pair_kernel.h")
    assert re.search(r"template\s*<\s*int\s+R\s*>\s*__global__[^\n]*\bsw_affine_pair_ext_kernel\(", kernel)
    host = _read(CSRC, "host_affine.h")
    # one dispatch over kPairR (the pair family's) asks the mode for the instance of an R; the extension mode names its kernel once
    assert len(re.findall(r"with_listed_R<kPairR>\(R,[^;]*M::template kernel<decltype\(r\)::value>\(c\)", host, re.S)) == 1
    m = re.search(r"struct\s+AffineExtMode\s*\{(.*?)\n\};", host, re.S)
    assert m and re.search(r"template\s*<\s*int\s+R\s*>[^;]*return\s+&sw_affine_pair_ext_kernel<R>\s*;", m.group(1)) and host.count("&sw_affine_pair_ext_kernel<R>") == 1
    assert re.search(r"affine_list_stage\(AffinePairFamily<AffineExtMode>\{", host) and "affine_pair_ext[R=%d]" in host
    # the anchored model is a third model of the exact fill; the template head the other models are named by stays
    fill = _read(CSRC, "sw_affine_kernel.h")
    assert re.search(r"template\s*<\s*bool\s+TRACE\s*,\s*bool\s+E2E\s*=\s*false\s*,\s*bool\s+BAND\s*=\s*false\s*>", fill)
    assert "kAffineModelExt" in fill and "sw_affine_exact_ext_kernel" in fill and "sw_affine_trace_ext_kernel" in fill
