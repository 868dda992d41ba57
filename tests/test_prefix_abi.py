"""The prefix filter's options and counter are part of the C-ABI's lists (no GPU): mi355_sw_option_names names no_prefix and
prefix_min_cols, which mi355_sw_set_option and the environment take, and the test hook prefix_tiles, which only mi355_sw_set_option
takes (as fault_inject: an environment variable must not change what mi355_sw_score_ranges returns); the header documents the two
options with the counter prefix_certified."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_and_counter_are_listed(pgs):
    names = pgs.capi.option_names()
    for key in ("no_prefix", "prefix_min_cols", "prefix_tiles"):
        assert key in names, key
    with open(os.path.join(ROOT, "include", "mi355_sw.h")) as f:
        header = f.read()
    for word in ("prefix_certified", "no_prefix", "prefix_min_cols"):
        assert word in header, word
    with open(os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "host_common.h")) as f:
        common = f.read()
    macros = [l for l in common.splitlines() if "X(no_prefix)" in l or "X(prefix_min_cols)" in l]
    assert len(macros) == 2 and not any("prefix_tiles" in l for l in macros), "prefix_tiles must not be read from the environment"
    with open(os.path.join(ROOT, "parallel-genomeseq_amd", "csrc", "mi355_sw.hip")) as f:
        assert 'k == "prefix_certified"' in f.read()
