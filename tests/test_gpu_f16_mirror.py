"""GPU parity of the mirrored float16 score cells (sw_score_kernel kSemF16M, DESIGN.md §3.3 lemma L14): the same results as
today's float16 cells (option no_f16_mirror) and as the oracle, on the batches that take them (150 bp, both engines; 300 bp)
and on one where the 1024 bound fails (400 bp at 3 / -3 / 2), which keeps the plain float16 cell."""
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

from switch_inputs import build

pytestmark = pytest.mark.gpu

KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")


def _input(pgs, name):
    if name in ("batch150_f32", "batch150_u8"):
        kind, qs, ref, sem = build(pgs, name)
        return qs, ref, sem
    m = {"batch300_f32": 300, "batch400_f32": 400}[name]
    ref = pgs.synth.dna(9111, 200_000)
    qs = [pgs.synth.read_from_ref(ref, 9900 + k, m, sub_rate=0.02, indel_rate=0.004)[0].tobytes() for k in range(24)]
    qs.append(pgs.synth.dna(9901, m).tobytes())                           # one unrelated read: a low score
    return qs, ref.tobytes(), 0


@pytest.mark.parametrize("name,mirrored", [("batch150_f32", True), ("batch150_u8", True), ("batch300_f32", True),
                                           ("batch400_f32", False)])
def test_mirrored_cells_match(pgs, oracle, name, mirrored):
    qs, ref, sem = _input(pgs, name)
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda q: oracle.align(q, ref, sem), qs))
    c = pgs.Context(0)
    try:
        res_on = c.align_batch(qs, ref, semantics=sem)
        path_on = " ".join(c.last_path())
        kname = c.last_kernel()["name"]
        c.set_option("no_f16_mirror", True)
        res_off = c.align_batch(qs, ref, semantics=sem)
        path_off = " ".join(c.last_path())
    finally:
        c.close()
    assert re.search(r"score\[cell=f16", path_on), path_on
    assert re.search(r"score\[cell=f16", path_off), path_off
    assert "mirror=" not in path_off, path_off
    if mirrored:
        assert re.search(r"score\[cell=f16[^\]]*,mirror=1\]", path_on), path_on
        assert "mirrored" in kname, kname
    else:
        assert "mirror=" not in path_on, path_on
    for k, (a, b, e) in enumerate(zip(res_on, res_off, exp)):
        for f in KEYS:
            assert a[f] == b[f], "%s, alignment %d: %s differs with and without mirrored cells: %r vs %r" % (name, k, f, a[f], b[f])
            assert a[f] == e[f], "%s, alignment %d: %s differs from the oracle: %r vs %r" % (name, k, f, a[f], e[f])
