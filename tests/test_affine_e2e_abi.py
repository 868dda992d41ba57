"""The interface of the end-to-end mode of the affine pair lists (no GPU needed): the two _mode entry points and the two enum values
are declared in include/mi355_sw.h, the built library exports the symbols, the Python binding takes the mode, every instance of the
pair kernel is compiled for both modes, and an argument error — no context, whatever the mode — comes back as MI355_SW_EINVAL before
any device work (this machine may have no device at all)."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi355_sw_affine_pairs_run_mode", "mi355_sw_affine_pairs_trace_mode")
EINVAL = -22


def _header():
    with open(os.path.join(ROOT, "include", "mi355_sw.h")) as f:
        return f.read()


def test_symbols_declared_and_exported(pgs):
    header = _header()
    L = pgs.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*,\s*size_t\s+npairs\s*,\s*const\s+int32_t\s*\*\s*query\s*,"
                         r"\s*const\s+int64_t\s*\*\s*lefts\s*,\s*const\s+int64_t\s*\*\s*rights\s*,\s*const\s+mi355_sw_affine_params\s*\*"
                         % name, header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None


def test_enum_values(pgs):
    m = re.search(r"enum\s*\{\s*MI355_SW_AFFINE_LOCAL\s*=\s*(\d+)\s*,\s*MI355_SW_AFFINE_END_TO_END\s*=\s*(\d+)\s*\}", _header())
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert (pgs.capi.AFFINE_LOCAL, pgs.capi.AFFINE_END_TO_END) == (0, 1)
    assert pgs.capi.AFFINE_MODES == {"local": 0, "end_to_end": 1}


def test_the_model_is_stated_in_the_header():
    header = _header()
    for needle in ("no zero floor", "H(i,0) = F(i,0) = -(o + (i-1) e)", "the smallest such j", "affine_pair_e2e[R=..]", "< 2^24"):
        assert needle in header, needle


def test_python_takes_the_mode(pgs):
    for name in ("affine_pairs_run", "affine_pairs_trace"):
        p = inspect.signature(getattr(pgs.capi.Context, name)).parameters
        assert p["mode"].default == "local", name
    assert inspect.signature(pgs.AffineSWAligner.align_pairs).parameters["end_to_end"].default is False
    with pytest.raises(ValueError):
        pgs.capi.Context._pair_mode("global")


def test_argument_errors_come_before_any_device_work(pgs):
    L = pgs.capi.lib()
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    sc, ex, ey = (C.c_float * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()
    for mode in (0, 1, 2, -1, 77):                                    # without a context every call is EINVAL, good mode or bad
        assert L.mi355_sw_affine_pairs_run_mode(None, C.c_int(mode), C.c_size_t(n), qa, la, ra, C.byref(p), sc, ex, ey) == EINVAL
        assert L.mi355_sw_affine_pairs_trace_mode(None, C.c_int(mode), C.c_size_t(n), qa, la, ra, C.byref(p), res) == EINVAL
    assert list(sc) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)


def test_every_instance_is_compiled_for_both_modes():
    base = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
    with open(os.path.join(base, "sw_affine_pair_kernel.h")) as f:
        kernel = f.read()
    assert re.search(r"template\s*<\s*int\s+R\s*>\s*__global__[^\n]*\bsw_affine_pair_e2e_kernel\(", kernel)
    with open(os.path.join(base, "host_affine.h")) as f:
        host = f.read()
    # one dispatch over kPairR (the pair family's) asks the mode for the instance of an R, and the call's mode picks both in one place
    assert len(re.findall(r"with_listed_R<kPairR>\(R,[^;]*M::template kernel<decltype\(r\)::value>\(c\)", host, re.S)) == 1
    m = re.search(r"struct\s+AffinePairMode\s*\{(.*?)\n\};", host, re.S)
    assert m and re.search(r"template\s*<\s*int\s+R\s*>[^;]*c\.e2e\(\)\s*\?\s*&sw_affine_pair_e2e_kernel<R>\s*:\s*&sw_affine_pair_kernel<R>\s*;", m.group(1))
    assert host.count("&sw_affine_pair_e2e_kernel<R>") == 1 and host.count("&sw_affine_pair_kernel<R>") == 1
