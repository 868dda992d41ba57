"""CPU-side checks of the affine-gap boundary: the three calls are declared in include/mi355_sw.h, exported by the library and listed
in capi.EXPORTS, the A/B option exists, and without a GPU nothing is computed (no CPU fallback)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AFFINE = ("mi355_sw_affine_align", "mi355_sw_affine_batch_run", "mi355_sw_affine_score_ranges")


def test_affine_symbols_declared_exported_and_listed(pgs):
    text = open(os.path.join(ROOT, "include", "mi355_sw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = pgs.capi.lib()
    for name in AFFINE:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared in include/mi355_sw.h" % name
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pgs.capi.EXPORTS
    assert re.search(r"\}\s*mi355_sw_affine_params\s*;", text)
    for field in ("lut", "match", "mismatch", "gap_open", "gap_extend"):
        assert field in [f[0] for f in pgs.capi.AffineParams._fields_]


def test_no_affine_sweep_is_an_option(pgs):
    assert "no_affine_sweep" in pgs.capi.option_names()


def test_python_interface(pgs):
    import inspect
    for name in ("affine_align", "affine_batch_run", "affine_score_ranges"):
        sig = inspect.signature(getattr(pgs.Context, name))
        got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
        assert got == dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None), name
    la = pgs.AffineSWAligner("ACGT", "ACGT")
    assert la.getScore() == -1.0 and la.getEnd() == (0, 0)


def test_no_cpu_fallback(pgs):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pgs.MI355Error):
        pgs.Context(0).affine_align("ACGT", "ACGT")
    with pytest.raises(pgs.MI355Error):
        pgs.AffineSWAligner("GGTTGACTA", "TGTTACGG").calculateScore()
