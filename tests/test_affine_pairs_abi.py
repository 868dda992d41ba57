"""The interface of the affine pair lists (no GPU needed): both entry points are declared in include/mi355_sw.h and exported by the
built library, option no_affine_pairs is listed, and the Python binding has the two methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi355_sw_affine_pairs_run", "mi355_sw_affine_pairs_trace")


def test_symbols_declared_and_exported(pgs):
    with open(os.path.join(ROOT, "include", "mi355_sw.h")) as f:
        header = f.read()
    L = pgs.capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*mi355_sw_ctx\s*\*\s*ctx\s*,\s*size_t\s+npairs\s*,\s*const\s+int32_t\s*\*\s*query\s*,"
                         r"\s*const\s+int64_t\s*\*\s*lefts\s*,\s*const\s+int64_t\s*\*\s*rights\s*,\s*const\s+mi355_sw_affine_params\s*\*"
                         % name, header), name
        assert name in pgs.capi.EXPORTS
        assert getattr(L, name) is not None


def test_option_is_listed_and_names_stay_unique(pgs):
    names = pgs.capi.option_names()
    assert "no_affine_pairs" in names
    assert len(names) == len(set(names))


def test_context_has_the_methods(pgs):
    for name in ("affine_pairs_run", "affine_pairs_trace"):
        assert callable(getattr(pgs.capi.Context, name))


def test_instance_list_of_the_kernel():
    with open(os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "sw_affine_pair_kernel.h")) as f:
        m = re.search(r"constexpr\s+int\s+kPairR\[\]\s*=\s*\{([^}]*)\}", f.read())
    rs = [int(v) for v in m.group(1).split(",")]
    assert 1 <= len(rs) <= 8 and rs == sorted(set(rs)) and rs[0] >= 1 and rs[-1] == 32      # 1..512 rows, five key bits
    assert min(16 * r for r in rs if 16 * r >= 150) - 150 <= 10                                # a 150-row read: at most 10 padding rows
