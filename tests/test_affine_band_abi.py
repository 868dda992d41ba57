"""The interface of the banded affine pair lists (no GPU needed): the two _band entry points are declared in include/mi355_sw.h and
exported by the built library, the header states the model, the Python binding takes band_lo / band_hi / band, option no_affine_band
is listed, an argument error — no context — comes back as MI355_SW_EINVAL before any device work and writes nothing, and there is a
list of band-kernel instances that the host dispatches over."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-genomeseq_amd", "csrc")
SYMBOLS = ("mi355_sw_affine_pairs_run_band", "mi355_sw_affine_pairs_trace_band")
EINVAL = -22


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_symbols_declared_and_exported(pgs):
    header = _read(ROOT, "include", "mi355_sw.h")
    L = pgs.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*,\s*size_t\s+npairs\s*,\s*const\s+int32_t\s*\*\s*query\s*,"
                         r"\s*const\s+int64_t\s*\*\s*lefts\s*,\s*const\s+int64_t\s*\*\s*rights\s*,\s*const\s+int64_t\s*\*\s*band_lo\s*,"
                         r"\s*const\s+int64_t\s*\*\s*band_hi\s*,\s*const\s+mi355_sw_affine_params\s*\*" % name, header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None


def test_the_model_is_stated_in_the_header():
    header = _read(ROOT, "include", "mi355_sw.h")
    for needle in ("band_lo[k] <= j - i <= band_hi[k]", "H = E = F = -infinity", "out-of-band neighbour holds H = 0",
                   "lo_e = max(band_lo, 1 - m), hi_e = min(band_hi, n - 1)", "first maximum in column-major order among the in-band cells",
                   "the walk never leaves the band", "affine_band[R=..]", "no_affine_band", "never falls back to an unbanded kernel"):
        assert needle in header, needle


def test_option_is_listed(pgs):
    names = pgs.capi.lib().mi355_sw_option_names().decode().split(",")
    assert "no_affine_band" in names and "no_affine_pairs" in names


def test_python_takes_the_band(pgs):
    for name in ("affine_pairs_run", "affine_pairs_trace"):
        p = inspect.signature(getattr(pgs.capi.Context, name)).parameters
        assert p["band_lo"].default is None and p["band_hi"].default is None, name
        assert p["mode"].default == "local"
    assert inspect.signature(pgs.AffineSWAligner.align_pairs).parameters["band"].default is None
    lo, hi = pgs.capi.Context._pair_bands(-3, [1, 2, 3], 3)
    assert lo.dtype == np.int64 and lo.tolist() == [-3, -3, -3] and hi.tolist() == [1, 2, 3]
    assert pgs.capi.Context._pair_bands(None, None, 3) == (None, None)
    for bad in ((None, 3), (3, None), ([1, 2], [3, 4, 5])):
        with pytest.raises(ValueError):
            pgs.capi.Context._pair_bands(bad[0], bad[1], 3)


def test_argument_errors_come_before_any_device_work(pgs):
    L = pgs.capi.lib()
    p, keep = pgs.capi.make_affine_params()
    n = 2
    qa, la, ra = (C.c_int32 * n)(0, 1), (C.c_int64 * n)(0, 10), (C.c_int64 * n)(100, 200)
    bl, bh = (C.c_int64 * n)(-5, -5), (C.c_int64 * n)(5, 5)
    sc, ex, ey = (C.c_float * n)(7, 7), (C.c_int64 * n)(7, 7), (C.c_int64 * n)(7, 7)
    res = (pgs.capi.Result * n)()
    for mode in (0, 1, 2, -1):                                        # without a context every call is EINVAL, bands or none
        for lo, hi in ((bl, bh), (None, None), (bl, None), (None, bh), (bh, bl)):
            assert L.mi355_sw_affine_pairs_run_band(None, C.c_int(mode), C.c_size_t(n), qa, la, ra, lo, hi, C.byref(p), sc, ex, ey) == EINVAL
            assert L.mi355_sw_affine_pairs_trace_band(None, C.c_int(mode), C.c_size_t(n), qa, la, ra, lo, hi, C.byref(p), res) == EINVAL
    assert list(sc) == [7, 7] and list(ex) == [7, 7] and list(ey) == [7, 7]
    assert all(r.cons_x is None and r.cons_len == 0 for r in res)


def test_there_is_an_instance_list_and_it_is_dispatched():
    kernel = _read(CSRC, "sw_affine_band_kernel.h")
    m = re.search(r"constexpr\s+int\s+kBandR\[\]\s*=\s*\{([^}]*)\}", kernel)
    Rs = [int(v) for v in m.group(1).split(",")]
    assert Rs == sorted(set(Rs)) and len(Rs) >= 3 and 16 * Rs[-1] >= 256 and 16 * Rs[0] <= 32      # W <= 256, a narrow band pays little
    assert re.search(r"template\s*<\s*int\s+R\s*>\s*__global__[^\n]*\bsw_affine_band_kernel\(", kernel)
    host = _read(CSRC, "host_affine.h")
    # one dispatch over kBandR (the band family's) asks the mode for the instance of an R; the local mode names its kernel once
    assert len(re.findall(r"with_listed_R<kBandR>\(R,[^;]*M::template kernel<decltype\(r\)::value>\(c\)", host, re.S)) == 1
    m = re.search(r"struct\s+AffineBandMode\s*\{(.*?)\n\};", host, re.S)
    assert m and re.search(r"template\s*<\s*int\s+R\s*>[^;]*return\s+&sw_affine_band_kernel<R>\s*;", m.group(1)) and host.count("&sw_affine_band_kernel<R>") == 1
    # the band kernel's family runs on the list stage it shares with the pair kernel
    assert re.search(r"int\s+affine_list_stage\(", host) and re.search(r"affine_list_stage\(AffineBandFamily<AffineBandMode>\{", host) and "affine_band[R=%d]" in host
    # the shared fill takes the band as a template parameter whose default is the unbanded code
    assert re.search(r"template\s*<\s*bool\s+TRACE\s*,\s*bool\s+E2E\s*=\s*false\s*,\s*bool\s+BAND\s*=\s*false\s*>", _read(CSRC, "sw_affine_kernel.h"))
    assert '#include "sw_affine_band_kernel.h"' in _read(CSRC, "mi355_sw.hip")
