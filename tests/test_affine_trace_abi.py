"""CPU-side checks of the affine-gap traceback boundary: the two calls are declared in include/mi355_sw.h, exported by the library
and listed in capi.EXPORTS, the Python signatures and defaults are the documented ones, capi.cigar reads a reversed pair, and without
a GPU nothing is computed (no CPU fallback)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = ("mi355_sw_affine_align_trace", "mi355_sw_affine_batch_trace")
DEFAULTS = dict(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None)


def test_trace_symbols_declared_exported_and_listed(pgs):
    text = open(os.path.join(ROOT, "include", "mi355_sw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = pgs.capi.lib()
    for name in TRACE:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/mi355_sw.h" % name
        assert "mi355_sw_affine_params" in m.group(1) and re.search(r"mi355_sw_result\s*\*", m.group(1)), m.group(1)
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pgs.capi.EXPORTS


def test_header_states_the_rule_and_no_longer_says_no_traceback():
    text = open(os.path.join(ROOT, "include", "mi355_sw.h")).read()
    assert "No traceback" not in text
    for word in ("state M", "state E", "state F", "REVERSED", "begin_x"):
        assert word in text, word


def test_python_interface(pgs):
    for name in ("affine_align_trace", "affine_batch_trace"):
        sig = inspect.signature(getattr(pgs.Context, name))
        got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
        assert got == DEFAULTS, name
    assert list(inspect.signature(pgs.Context.affine_align_trace).parameters)[:3] == ["self", "x", "y"]
    sig = inspect.signature(pgs.AffineSWAligner.__init__)
    assert sig.parameters["traceback"].default is False
    la = pgs.AffineSWAligner("ACGT", "ACGT", traceback=True)
    assert la.getScore() == -1.0 and la.getEnd() == (0, 0)
    assert (la.getPos(), la.getConsensus_x(), la.getConsensus_y(), la.getBegin(), la.getCigar()) == (0, "", "", (0, 0), "")
    la = pgs.AffineSWAligner("ACGT", "ACGT")                        # the default is unchanged: score and end cell only
    assert la.getScore() == -1.0 and la.getEnd() == (0, 0)
    with pytest.raises(RuntimeError):
        la.getCigar()


def test_cigar_of_a_reversed_pair(pgs):
    cigar = pgs.capi.cigar
    assert cigar("", "") == ""
    assert cigar("GCA", "GCA") == "3M"
    assert cigar("TG-CA", "TGACA") == "2M1D2M"                      # reversed: forward AC-GT / ACAGT
    assert cigar("TTGCA", "T--CA") == "2M2I1M"                      # forward ACGTT / AC--T
    assert cigar("A-T", "AC-") == "1I1D1M"                          # forward T-A / -CA
    with pytest.raises(ValueError):
        cigar("AC", "A")


def test_no_cpu_fallback(pgs):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pgs.MI355Error):
        pgs.Context(0).affine_align_trace("ACGT", "ACGT")
    with pytest.raises(pgs.MI355Error):
        pgs.Context(0).affine_batch_trace()
    with pytest.raises(pgs.MI355Error):
        pgs.AffineSWAligner("GGTTGACTA", "TGTTACGG", traceback=True).calculateScore()
