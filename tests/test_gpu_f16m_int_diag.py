"""GPU checks of the mirrored float16 cells' integer diagonal term (sw_score_kernel kSemF16M): the same
results as the clamped float16 add (option no_f16m_int_diag) and as the oracle, on the batches that take mirrored cells — 150 bp
under both engines, 300 bp, and exact 340 bp reads at 3 / -3 / 2 where H reaches 1020 — and the device's clamp of
v_pk_minimum3_f16, which now carries the zero floor."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from switch_inputs import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")


def _input(pgs, name):
    if name in ("batch150_f32", "batch150_u8"):
        kind, qs, ref, sem = build(pgs, name)
        return qs, ref, sem
    ref = pgs.synth.dna(9121, 200_000)
    if name == "batch300_f32":
        qs = [pgs.synth.read_from_ref(ref, 9920 + k, 300, sub_rate=0.02, indel_rate=0.004)[0].tobytes() for k in range(24)]
    else:
        # exact copies of the reference (H = 3 * 340 = 1020, the top of the range) and a few with one substitution or indel
        qs = [pgs.synth.read_from_ref(ref, 9940 + k, 340, sub_rate=0.0, indel_rate=0.0)[0].tobytes() for k in range(12)]
        qs += [pgs.synth.read_from_ref(ref, 9960 + k, 340, sub_rate=0.003, indel_rate=0.003)[0].tobytes() for k in range(11)]
    qs.append(pgs.synth.dna(9921, len(qs[0])).tobytes())                  # one unrelated read: a low score
    return qs, ref.tobytes(), 0


@pytest.mark.parametrize("name", ["batch150_f32", "batch150_u8", "batch300_f32", "batch340_exact_f32"])
def test_int_diag_matches(pgs, oracle, name):
    qs, ref, sem = _input(pgs, name)
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda q: oracle.align(q, ref, sem), qs))
    c = pgs.Context(0)
    try:
        res_on = c.align_batch(qs, ref, semantics=sem)
        path_on = " ".join(c.last_path())
        kname_on = c.last_kernel()["name"]
        c.set_option("no_f16m_int_diag", True)
        res_off = c.align_batch(qs, ref, semantics=sem)
        path_off = " ".join(c.last_path())
        kname_off = c.last_kernel()["name"]
    finally:
        c.close()
    # the switch engages: both runs on mirrored cells, the integer diagonal only without the option
    assert re.search(r"score\[cell=f16[^\]]*,idiag=1,mirror=1\]", path_on), path_on
    assert re.search(r"score\[cell=f16[^\]]*,mirror=1\]", path_off), path_off
    assert "idiag=" not in path_off, path_off
    assert "mirrored, integer diagonal" in kname_on, kname_on
    assert "mirrored" in kname_off and "integer diagonal" not in kname_off, kname_off
    if name == "batch340_exact_f32":
        assert max(e["score"] for e in exp) == 1020.0
    for k, (a, b, e) in enumerate(zip(res_on, res_off, exp)):
        for f in KEYS:
            assert a[f] == b[f], "%s, alignment %d: %s differs with and without the integer diagonal: %r vs %r" % (name, k, f, a[f], b[f])
            assert a[f] == e[f], "%s, alignment %d: %s differs from the oracle: %r vs %r" % (name, k, f, a[f], e[f])


def test_minimum3_clamp_on_device(tmp_path):
    # v_pk_minimum3_f16 ... clamp: halves above 1.0 come out as 1.0, values in [0.5, 1] unchanged (the kernel's domain)
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "mirror_int_diag_rate.bin")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-o", exe, os.path.join(ROOT, "tools", "ubench", "mirror_int_diag_rate.hip")],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe, "clamp"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 in the kernel's domain -> ok" in r.stdout, r.stdout
