"""The low step tiles of the seeded prefix flow (host_score.h kR2Step, kLowStepKernels) stand outside kScoreShapes, the table that
tests/test_lone_strip_instances_ref.py partitions among the raw-maxima modules.  Their owner is tests/test_gpu_prefix_low_tiles.py: the
heights it iterates are the header's list — a height added to kR2Step without a case fails here, without a GPU — and no instance of
kScoreShapes is a two-lane tile of one of those heights."""
import lone_strip_instances as ls
import score_instances as si
import test_gpu_prefix_low_tiles as low


def test_the_gpu_module_iterates_the_headers_list():
    lists = si.lists_in_header()
    assert lists["kR2Step"] == tuple(low.LOW) == (8, 10)
    assert max(lists["kR2Step"]) < min(lists["kR8M"])                 # prefix_heights_seeded: ascending


def test_no_instance_of_kScoreShapes_is_a_low_tile():
    insts, _ = ls.instances_in_header()                               # (R, sem, strips, SL, twin, comb, mk, rowp)
    lowR = set(si.lists_in_header()["kR2Step"])
    assert not [i for i in insts if i[3] == 2 and i[0] in lowR]
    assert {i[0] for i in insts if i[3] == 2} == set(si.R8M)
