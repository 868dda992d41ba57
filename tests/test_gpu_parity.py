"""GPU parity: the HIP path (through the C-ABI) against the golden fixtures made with the real
reference, and against the CPU oracle on seeded inputs.  Integer outputs (pos, argmax, consensus)
bit-exact; scores are small integers held in float -> tolerance 0 (north_star allows 1e-5)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCORE_TOL = 0.0


@pytest.fixture(scope="module")
def ctx(pgs):
    c = pgs.Context(0)
    yield c
    c.close()


def _pmap(fn, items, workers=8):
    """fn over items on a few threads (the oracle is a C library behind ctypes: its calls release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    items = list(items)
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(fn, items))


def _cmp(got, exp, what):
    assert abs(got["score"] - exp["score"]) <= SCORE_TOL, "%s: score %r != %r" % (what, got["score"], exp["score"])
    for k in ("pos", "end_x", "end_y", "cons_x", "cons_y"):
        if k in exp and exp[k] != -1:
            assert got[k] == exp[k], "%s: %s differs: got %r expected %r" % (what, k, got[k], exp[k])


def test_reference_gtest_cases(pgs, ctx):
    # test/test_localaligner.cpp:24-27, :53-58 through the mirrored class
    la = pgs.SWAligner("GGTTGACTA", "TGTTACGG", matrix=pgs.Similarity_Matrix_Skewed, context=ctx)
    la.calculateScore()
    assert la.getScore() == 13 and la.getPos() == 2
    assert la.getConsensus_x() == "CAGTTG" and la.getConsensus_y() == "CA-TTG"


def test_kat(ctx, golden):
    for c in golden["kat"]:
        _cmp(ctx.align(c["x"], c["y"], c["sem"], c["match"], c["mismatch"], c["gap"]), c["expect"], c["name"])


def test_matrices_and_skewed_equals_normal(ctx, golden):
    # test/test_skewedmatrix.cpp:39-66 + commented matrix test_localaligner.cpp:33-42 + square quirk
    for c in golden["matrix"]:
        H = ctx.fill_matrix(c["x"], c["y"], c["sem"], c["match"], c["mismatch"], c["gap"])
        exp = np.array(c["cells"], dtype=np.float32).reshape(len(c["x"]) + 1, len(c["y"]) + 1)
        assert np.array_equal(H, exp), (c["x"], c["y"], c["sem"])


def test_align_cases(ctx, golden):
    for k, c in enumerate(golden["align"]):
        _cmp(ctx.align(c["x"], c["y"], c["sem"], c["match"], c["mismatch"], c["gap"]), c["expect"], "align[%d]" % k)


def test_alignlut_cases(ctx, golden, pgs):
    for k, c in enumerate(golden["alignlut"]):
        lut = pgs.synth.make_lut(c["seed"], c["scale"])
        _cmp(ctx.align(c["x"], c["y"], c["sem"], gap=c["gap"], lut=lut), c["expect"], "alignlut[%d]" % k)


def test_split_cases(ctx, golden):
    for k, c in enumerate(golden["split"]):
        got = ctx.align_split(c["x"], c["y"], c["npiece"], c["ratio"], c["sm"], c["la"], c["match"], c["mismatch"], c["gap"])
        _cmp(got, c["expect"], "split[%d]" % k)


def test_no_match_defined(ctx):
    r = ctx.align("AAAA", "CCCCCC")
    assert r["score"] == 0 and r["pos"] == 0 and r["cons_x"] == "" and r["end_x"] == 0


def test_empty_inputs(ctx):
    assert ctx.align("", "ACGT")["score"] == 0
    assert ctx.align("ACGT", "")["score"] == 0


@pytest.mark.parametrize("sem,name", [(0, "f32"), (1, "u8")])
def test_data_small_digest(ctx, data_small, sem, name):
    """Config 1 (sw_solve_small) at full size through the batched path."""
    res = ctx.align_batch(data_small["reads"], data_small["ref"], semantics=sem)
    lines = ["%d,%g,%d,%s,%s\n" % (k, r["score"], r["pos"], r["cons_x"], r["cons_y"]) for k, r in enumerate(res)]
    for k, exp in enumerate(data_small["first"][name]):
        _cmp(res[k], exp, "data_small[%s][%d]" % (name, k))
    assert hashlib.sha256("".join(lines).encode()).hexdigest() == data_small["digests"][name]


def test_data_small_split_digest(ctx, data_small):
    lines = []
    for k, read in enumerate(data_small["reads"]):
        r = ctx.align_split(read, data_small["ref"], 17, 2.0, 1, 1)
        lines.append("%d,%g,%d,%s,%s\n" % (k, r["score"], r["pos"], r["cons_x"], r["cons_y"]))
    assert hashlib.sha256("".join(lines).encode()).hexdigest() == data_small["digests"]["u8_npiece17"]


@pytest.mark.parametrize("sem", [0, 1])
def test_config2_single_read_vs_1mbp(ctx, oracle, pgs, sem):
    """Config 2: one 150 bp synthetic read vs a 1 Mbp synthetic reference, bit-match vs the oracle."""
    ref = pgs.synth.dna(1, 1_000_000)
    read, off = pgs.synth.read_from_ref(ref, 2, 150)
    exp = oracle.align(read.tobytes(), ref.tobytes(), sem)
    got = ctx.align(read, ref, sem)
    _cmp(got, exp, "cfg2 sem=%d" % sem)
    assert abs(got["pos"] - (off + 1)) < 40


@pytest.mark.parametrize("sem", [0, 1])
def test_batch_vs_oracle(ctx, oracle, pgs, sem):
    """Ragged batch (lengths 20..250) against a 300 kbp reference, incl. reads that match nowhere."""
    ref = pgs.synth.dna(11, 300_000)
    reads = []
    for k in range(48):
        ln = [20, 33, 64, 100, 125, 150, 151, 200, 250][k % 9]
        r, _ = pgs.synth.read_from_ref(ref, 100 + k, ln, sub_rate=0.03, indel_rate=0.01)
        reads.append(r.tobytes())
    reads.append(pgs.synth.dna(999, 150).tobytes())          # unrelated read
    reads.append(b"N" * 40)                                   # matches nothing
    res = ctx.align_batch(reads, ref, semantics=sem)
    for k, (q, got) in enumerate(zip(reads, res)):
        _cmp(got, oracle.align(q, ref.tobytes(), sem), "batch[%d] sem=%d" % (k, sem))


def test_ties_and_repeats(ctx, oracle):
    unit = "ACGTTGCA"
    for sem in (0, 1):
        for x, y in [(unit * 4, unit * 5000), ("A" * 120, "A" * 30000), (unit * 12, ("T" * 50 + unit * 12) * 300)]:
            _cmp(ctx.align(x, y, sem), oracle.align(x, y, sem), "repeat sem=%d |y|=%d" % (sem, len(y)))


def test_full_size_planted_reads(ctx, pgs):
    """Config-3 shape at full reference size (50 Mbp): exact substrings must be found where they were
    cut (size-independent property; the oracle cannot hold a 150 x 50M matrix in a few seconds)."""
    ref = pgs.synth.dna(3, 50_000_000)
    offs = (pgs.synth.splitmix64(4, 64) % np.uint64(len(ref) - 150)).astype(np.int64)
    offs[0], offs[1] = 0, len(ref) - 150                       # both ends of the reference
    reads = [ref[o:o + 150].tobytes() for o in offs]
    ctx.set_reference(ref)
    ctx.batch_upload(reads)
    for sem in (0, 1):
        res = ctx.batch_run(semantics=sem)
        for o, r in zip(offs, res):
            if sem == 0:
                assert r["score"] == 450 and r["end_x"] == 150 and r["end_y"] == o + 150
                # consensus is stored end -> start; the greedy-by-value walk (smithwaterman.cpp:40-78)
                # follows the diagonal while scores are high, and may wander / overshoot near the start
                rev = ref[o:o + 150].tobytes()[::-1].decode()
                assert r["cons_x"][:100] == rev[:100] and r["cons_y"][:100] == rev[:100]
                assert r["pos"] <= o + 20 and len(r["cons_x"]) >= 140
            else:
                assert r["score"] == 255 and r["end_x"] == 85 and r["end_y"] == o + 85


def _cpp_test_binary(name):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if name in ("test_dropin_eigen.bin", "test_reference_gtests.bin"):
        return os.path.join(root, "oracle", "_ref", name)                 # built with the reference driver (oracle/build_ref.sh)
    exe = os.path.join(root, "tests", "cpp", name)
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build()
    return exe


def test_reference_gtest_files_compiled_in_place():
    """The reference's OWN test files (/root/reference/test/main.cpp, test_localaligner.cpp, test_skewedmatrix.cpp, …), compiled
    where they lie against include/parseq/*.h and a build-owned minimal <gtest/gtest.h> (oracle/build_ref.sh), run on the
    GPU: SWAligner_Test.Example_small_sequence_alignment / Verify_consensus_strings, SimilarityMatrix.SkewedMatrixIndex /
    SkewedMatrixDP — the four real tests of the reference.  Prebuilt where the reference exists (the binary
    travels to the GPU box); where it did not travel this is SKIPPED, not passed."""
    import os
    import subprocess
    exe = _cpp_test_binary("test_reference_gtests.bin")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_reference_gtests.bin was not built (needs the reference sources at build time)")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and "[  PASSED  ] 4 tests." in out, out
    for name in ("SWAligner_Test.Example_small_sequence_alignment", "SWAligner_Test.Verify_consensus_strings",
                 "SimilarityMatrix.SkewedMatrixIndex", "SimilarityMatrix.SkewedMatrixDP"):
        assert "[       OK ] " + name in out, out


def test_cpp_dropin_binary():
    """What the reference's gtest files do not cover of include/parseq/*.h (tests/cpp/test_dropin.cpp) runs on the GPU."""
    import os
    import subprocess
    exe = _cpp_test_binary("test_dropin.bin")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"ALL OK" in p.stdout, p.stdout.decode()
    # OMPParallelLocalAligner over a device set (MI355_SW_DEVICES -> mi355_sw_multi_align_split): same answers
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       env=dict(os.environ, MI355_SW_DEVICES="0,0"))
    assert p.returncode == 0 and b"ALL OK" in p.stdout, p.stdout.decode()
    # the reference's append-on-repeat behaviour of the consensus strings, opt-in (smithwaterman.cpp:40-78, :80-108)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       env=dict(os.environ, PARSEQ_APPEND_CONSENSUS="1"))
    assert p.returncode == 0 and b"ALL OK" in p.stdout and b"consensus appended on repeat" in p.stdout, p.stdout.decode()


def test_cpp_dropin_binary_with_eigen():
    """The same source compiled against the reference's vendored Eigen (oracle/build_ref.sh): Eigen::VectorXf
    getTimings(), const Eigen::MatrixXf &get_matrix(), MatrixX8u raw storage.  The binary is prebuilt where the reference
    exists (it travels to the GPU box); where it did not travel this leg is SKIPPED, not passed."""
    import os
    import subprocess
    exe2 = _cpp_test_binary("test_dropin_eigen.bin")
    if not os.path.exists(exe2):
        pytest.skip("oracle/_ref/test_dropin_eigen.bin was not built (needs the reference's vendored Eigen zip at build time)")
    p = subprocess.run([exe2], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"ALL OK" in p.stdout and b"Eigen signatures: ok" in p.stdout, p.stdout.decode()


def test_cpp_multi_device_binary():
    """mi355_sw_multi_* (one handle, several devices: pieces / alignments dealt to devices, packed-key merge on the
    host and through RCCL) == the single-device calls; on a one-GPU box with device sets {0}, {0,0}, {0,0,0}."""
    import subprocess
    exe = _cpp_test_binary("test_multi.bin")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and b"ALL OK" in p.stdout, p.stdout.decode()
    for name in (b"{0} ok", b"{0,0} ok", b"{0,0,0} ok", b"{0} rccl ok"):
        assert name in p.stdout, p.stdout.decode()


def test_cpp_multi_device_binary_two_devices():
    """The {0,1}, {0,1}+RCCL, {1,0,1} and all-devices+RCCL sets of tests/cpp/test_multi.cpp: only where the box has a second
    GPU — SKIPPED (not passed) on a one-GPU box."""
    import subprocess
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: the two-device sets of tests/cpp/test_multi.cpp did not run")
    exe = _cpp_test_binary("test_multi.bin")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0 and b"ALL OK" in p.stdout, p.stdout.decode()
    for name in (b"{0,1} ok", b"{0,1} rccl ok", b"{1,0,1} ok", b"all rccl ok"):
        assert name in p.stdout, p.stdout.decode()


def test_multi_context_vs_oracle(oracle, pgs):
    """MultiContext (two contexts on this GPU) against the ORACLE: split with ties across pieces and fractional
    scoring (the winner is picked on float keys), and a ragged batch with its best index."""
    m = pgs.MultiContext([0, 0])
    try:
        ref = pgs.synth.dna(61, 90_000).tobytes()
        q = ref[20_000:20_300]
        ref = ref[:70_000] + q + ref[70_300:]                              # second identical hit in a later piece
        for sm, la, npiece, sc in ((0, 0, 5, {}), (1, 1, 7, {}), (0, 1, 6, dict(match=2.5, mismatch=-1.5, gap=0.5))):
            got = m.align_split(q, ref, npiece, 2.0, sm, la, **sc)
            exp = oracle.align_split(q, ref, npiece, 2.0, sm, la, **sc)
            _cmp(got, exp, ("multi split", sm, la, npiece))
            assert got["piece"] == exp["piece"]
        refa = np.frombuffer(ref, dtype=np.uint8)
        reads = [pgs.synth.read_from_ref(refa, 900 + k, [33, 64, 150, 151, 400, 700][k % 6])[0].tobytes() for k in range(40)]
        for sem in (0, 1):
            res, best = m.align_batch(reads, ref, semantics=sem)
            exp = _pmap(lambda r: oracle.align(r, ref, sem), reads)
            for g, e in zip(res, exp):
                _cmp(g, e, ("multi batch", sem))
            scores = [e["score"] for e in exp]
            assert best == scores.index(max(scores))
    finally:
        m.close()


def test_score_ranges_and_ref_sharding(ctx, oracle, pgs):
    """mi355_sw_score_ranges (per-piece maxima, plocalaligner.cpp:110-129) and the reference-sharding
    driver of dist.py with GPU callables (world size 1 here; world size 2 is covered with gloo on CPU)."""
    from parallel_genomeseq_amd import dist as pd
    ref = pgs.synth.dna(6, 400_000)
    q = ref[70_000:70_150].tobytes()
    refb = ref.tobytes()
    refb = refb[:300_000] + q + refb[300_150:]
    for sm, la, npiece in ((0, 0, 8), (1, 1, 17), (1, 0, 4)):
        ranges = pgs.capi.make_string_range(npiece, len(q), len(refb), 2.0)
        ctx.set_reference(refb)
        ctx.batch_upload([q])
        mx = ctx.score_ranges(ranges, semantics=sm)
        assert mx.shape == (npiece, 1)
        for k, (l, r) in enumerate(ranges):
            assert mx[k, 0] == oracle.score_only(q, refb[l:r], sm), (sm, k)
        res, piece = pd.align_split_sharded(
            ranges, lambda pieces: [ctx.score_ranges([ranges[p] for p in pieces], semantics=sm)[i, 0] for i, p in enumerate(pieces)],
            lambda p: ctx.align(q, refb[ranges[p][0]:ranges[p][1]], la))
        exp = oracle.align_split(q, refb, npiece, 2.0, sm, la)
        assert piece == exp["piece"]
        for k in ("score", "pos", "cons_x", "cons_y"):
            assert res[k] == exp[k], (sm, la, npiece, k)


@pytest.mark.parametrize("sem", [0, 1])
def test_long_queries_strip_mined(ctx, oracle, pgs, sem):
    """Queries longer than one 512-row strip (config-5 shape at oracle-sized reference): the strip-mined
    score kernel hands the bottom row of each strip to the next one through global scratch."""
    ref = pgs.synth.dna(61, 120_000)
    refb = ref.tobytes()
    for k, m in enumerate((512, 513, 700, 1500, 2100)):
        q, off = pgs.synth.read_from_ref(ref, 700 + k, m, sub_rate=0.02, indel_rate=0.005)
        exp = oracle.align(q.tobytes(), refb, sem)
        _cmp(ctx.align(q, refb, sem), exp, "long m=%d sem=%d" % (m, sem))
    # a batch mixing short and long queries runs entirely on the strip-mined instance
    qs = [pgs.synth.read_from_ref(ref, 900 + k, m)[0].tobytes() for k, m in enumerate((100, 1300, 150, 600, 40))]
    for q, got in zip(qs, ctx.align_batch(qs, refb, semantics=sem)):
        _cmp(got, oracle.align(q, refb, sem), "mixed batch sem=%d |q|=%d" % (sem, len(q)))


def test_config5_shape_reduced(ctx, oracle, pgs):
    """Config 5 at reduced reference: one 10 kbp query, reference split with overlap = 2x query
    (OMPParallelLocalAligner), against the oracle's serial split aligner; and whole-reference == split."""
    ref = pgs.synth.dna(6, 400_000)
    q, off = pgs.synth.read_from_ref(ref, 7, 10_000, sub_rate=0.01, indel_rate=0.001)
    qb, refb = q.tobytes(), ref.tobytes()
    whole = ctx.align(qb, refb, 0)
    assert whole["score"] == oracle.score_only(qb, refb, 0)
    assert abs(whole["pos"] - (off + 1)) < 200
    got = ctx.align_split(qb, refb, 4, 2.0, 0, 0)
    assert got["score"] == whole["score"] and got["pos"] == whole["pos"] and got["cons_x"] == whole["cons_x"]
    # exact check of score + argmax on a size the float32 oracle can hold (10 kbp x 60 kbp = 2.4 GB)
    sub = refb[max(0, off - 20_000):off + 40_000]
    exp = oracle.align(qb, sub, 0)
    _cmp(ctx.align(qb, sub, 0), exp, "cfg5 reduced")


def _drivers_dir():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "parallel-genomeseq_amd", "drivers")
    if not os.path.exists(os.path.join(d, "sw_solve_small.bin")):
        import subprocess
        subprocess.check_call(["make", "-C", d])
    return d


def test_driver_sw_solve_small(data_small, tmp_path):
    """The sw_solve_small-shaped driver on the reference's own data_small inputs (config 1): CSV rows
    `<input_line>, <pos>, <score>`; sums equal SURVEY.md Appendix B for both engines and for the
    17-piece split configuration of the reference's USEOMP build."""
    import os
    import subprocess
    d = _drivers_dir()
    fa = tmp_path / "genome.fa"
    ref = data_small["ref"]
    fa.write_text(">22_5K\n" + "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60)) + "\n")
    csv = tmp_path / "truth.csv"
    csv.write_text("index,QNAME,SEQ,POS\n" + "".join("%d,22_5K-1170,%s,%d\n" % (k, r, p) for k, (r, p) in
                                                       enumerate(zip(data_small["reads"], data_small["sam_pos"]))))
    for extra, name, ssum, psum in ((["--engine=f32"], "f32", 437131, 2750571), (["--engine=u8"], "u8", 298350, 2688127),
                                    (["--engine=u8", "--npiece=17", "--overlap=2.0"], None, 298350, 2669362)):
        out = tmp_path / "out.csv"
        p = subprocess.run([os.path.join(d, "sw_solve_small.bin"), str(fa), str(csv), str(out)] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and b"GCUP:" in p.stdout, p.stdout.decode()
        rows = out.read_text().splitlines()
        assert rows[0] == "index,QNAME,SEQ,POS,pos_pred,score" and len(rows) == 1171
        pos = [int(r.split(", ")[1]) for r in rows[1:]]
        sc = [float(r.split(", ")[2]) for r in rows[1:]]
        assert rows[1].startswith("0,22_5K-1170,GGTGGAGG") and sum(sc) == ssum and sum(pos) == psum
        if name:
            for k, e in enumerate(data_small["first"][name]):
                assert pos[k] == e["pos"] and sc[k] == e["score"]


def test_driver_sw_solve_big_and_uniprot(pgs, oracle, tmp_path):
    import os
    import subprocess
    d = _drivers_dir()
    ref = pgs.synth.dna(1, 200_000)
    reads = [pgs.synth.read_from_ref(ref, 40 + k, 150)[0].tobytes().decode() for k in range(3)]
    (tmp_path / "ref.fa").write_text(ref.tobytes().decode() + "\n")
    (tmp_path / "reads.csv").write_text("index,QNAME,SEQ,POS\n" + "".join("%d,r%d,%s,0\n" % (k, k, r) for k, r in enumerate(reads)))
    for npiece in ("0", "2"):
        p = subprocess.run([os.path.join(d, "sw_solve_big.bin"), npiece, "2", str(tmp_path / "ref.fa"), str(tmp_path / "reads.csv")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and b"[INFO] GCUPS avg:" in p.stdout, p.stdout.decode()
    # UniProt-shaped batch: each database sequence is the FIRST argument, the query the SECOND
    query = pgs.synth.protein(9, 144).tobytes().decode()
    db = [pgs.synth.protein(100 + k, n).tobytes().decode() for k, n in enumerate((30, 200, 361, 700, 90))]
    db[2] = db[2][:100] + query[20:120] + db[2][200:]
    (tmp_path / "q.fasta").write_text(">sp|Q\n" + query[:60] + "\n" + query[60:] + "\n")
    (tmp_path / "db.fasta").write_text("".join(">s%d\n%s\n" % (k, s) for k, s in enumerate(db)))
    out = tmp_path / "u.csv"
    # single device; two contexts dealt the sequences (host merge); one device with the RCCL merge of the best key
    for extra in ([], ["--devices=0,0"], ["--devices=0", "--rccl"]):
        p = subprocess.run([os.path.join(d, "sw_solve_uniprot.bin"), str(tmp_path / "q.fasta"), str(tmp_path / "db.fasta"), str(out)] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and b"best: sequence 2" in p.stdout, p.stdout.decode()
        assert (b"devices" in p.stdout) == bool(extra) and (b"RCCL" in p.stdout) == ("--rccl" in extra)
        rows = out.read_text().splitlines()
        assert rows[0] == "read,pos_pred,score" and len(rows) == 6
        for k, s in enumerate(db):
            e = oracle.align(s, query, oracle.F32)
            seq, pos, sc = rows[1 + k].split(", ")
            assert seq == s[:126] and int(pos) == e["pos"] and float(sc) == e["score"]


def test_protein_alphabet_and_high_bytes(ctx, oracle, pgs):
    """Large alphabets (LDS profile > 64 KiB on the 32-row instances), table scoring on proteins, and bytes
    >= 128 (the reference compares raw chars / casts to uint8, no case folding)."""
    ref = pgs.synth.protein(71, 30_000).tobytes()
    lut = pgs.synth.make_lut(12345, 1.0)
    for k, m in enumerate((60, 144, 400, 700)):
        q = bytearray(ref[5000 + 997 * k:5000 + 997 * k + m])
        for i in range(0, m, 17):
            q[i] = ord("W")
        q = bytes(q)
        for sem in (0, 1):
            _cmp(ctx.align(q, ref, sem), oracle.align(q, ref, sem), "protein identity m=%d sem=%d" % (m, sem))
        _cmp(ctx.align(q, ref, 0, gap=3.0, lut=lut), oracle.align(q, ref, 0, gap=3.0, lut=lut), "protein lut m=%d" % m)
    rng = np.random.default_rng(5)
    hi = rng.integers(120, 256, size=20_000, dtype=np.uint8).tobytes()
    q = hi[7000:7090]
    for sem in (0, 1):
        _cmp(ctx.align(q, hi, sem), oracle.align(q, hi, sem), "high bytes sem=%d" % sem)
    assert ctx.align("acgtacgtacgt", "ACGTACGTACGT" * 100)["score"] == 0        # no case folding


def test_float32_instance(ctx, oracle, pgs):
    """The float32-cell instance of the score kernel: fractional tables / gaps (std::function scoring of the
    float engine) and integer scores beyond the 16-bit cell range, on references too large for the
    whole-matrix path; incl. the strip-mined variant.  Scores are dyadic rationals here, so float sums are
    exact and the comparison is bit-exact; tolerance stated by north_star is 1e-5."""
    ref = pgs.synth.dna(81, 200_000)
    refb = ref.tobytes()
    lutq = pgs.synth.make_lut(777, 0.25)
    reads = [pgs.synth.read_from_ref(ref, 300 + k, m, sub_rate=0.03, indel_rate=0.01)[0].tobytes()
             for k, m in enumerate((40, 150, 151, 300, 640))]
    for q, got in zip(reads, ctx.align_batch(reads, refb, semantics=0, gap=1.5, lut=lutq)):
        _cmp(got, oracle.align(q, refb, 0, gap=1.5, lut=lutq), "f32 lut x0.25 gap 1.5 |q|=%d" % len(q))
    for q in reads[1:3]:
        _cmp(ctx.align(q, refb, 0, 2.5, -1.75, 0.5), oracle.align(q, refb, 0, 2.5, -1.75, 0.5), "f32 2.5/-1.75/0.5")
    # integer scores whose bound exceeds 16 bits: 2000 rows x 20 = 40000
    q = pgs.synth.read_from_ref(ref, 999, 2000, sub_rate=0.02, indel_rate=0.004)[0].tobytes()
    exp = oracle.align(q, refb, 0, 20.0, -15.0, 8.0)
    assert exp["score"] > 32767
    _cmp(ctx.align(q, refb, 0, 20.0, -15.0, 8.0), exp, "f32 score > 2^15")


def test_non_dyadic_fractional_scoring(ctx, oracle, pgs):
    """Scorings whose float32 additions ROUND (0.1, 0.3, 0.7 and a table scaled by 0.37 are not dyadic): the regime where
    north_star's 1e-5 tolerance, the 2^-k scaling of the float32 score instance and the warm-up margins (proved in real
    arithmetic, widened by the rounding slack of host_common.h make_margin) could bite.  References long enough for the
    TILED float32 instance (several tiles per query, warm-up columns in front of each), single calls and batches,
    one strip-mined query.  Compared bit-exact against the oracle (same operation order as dp_func,
    similaritymatrix.cpp:49-54); a mismatch reports the largest |delta|."""
    ref = pgs.synth.dna(83, 300_000)
    refb = ref.tobytes()
    reads = [pgs.synth.read_from_ref(ref, 500 + k, m, sub_rate=0.04, indel_rate=0.01)[0].tobytes()
             for k, m in enumerate((40, 150, 151, 152, 300, 511, 640))]
    worst = 0.0
    bad = []
    for sc in (dict(match=0.7, mismatch=-0.3, gap=0.1), dict(match=0.1, mismatch=-0.3, gap=0.7),
               dict(match=1.1, mismatch=-0.9, gap=0.37), dict(match=3.3, mismatch=-3.3, gap=2.2)):
        exp = _pmap(lambda q: oracle.align(q, refb, 0, **sc), reads)
        got = ctx.align_batch(reads, refb, semantics=0, **sc)
        assert ctx.last_kernel()["dtype"] == "f32" and ctx.last_kernel()["cells"] > 0        # the tiled float32 instance ran
        got += [ctx.align(q, refb, 0, **sc) for q in reads[1:4]]
        exp += exp[1:4]
        for g, e in zip(got, exp):
            worst = max(worst, abs(g["score"] - e["score"]))
            if any(g[k] != e[k] for k in ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")):
                bad.append((sc, len(e["cons_x"]), g["score"], e["score"], g["pos"], e["pos"]))
    lut = (pgs.synth.make_lut(4711, 1.0) * np.float32(0.37)).astype(np.float32)
    exp = _pmap(lambda q: oracle.align(q, refb, 0, gap=0.53, lut=lut), reads)
    for g, e in zip(ctx.align_batch(reads, refb, semantics=0, gap=0.53, lut=lut), exp):
        worst = max(worst, abs(g["score"] - e["score"]))
        if any(g[k] != e[k] for k in ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")):
            bad.append(("lut x0.37", len(e["cons_x"]), g["score"], e["score"], g["pos"], e["pos"]))
    # one strip-mined query (2500 rows) on a shorter reference (the oracle holds the whole float matrix)
    sub = refb[:120_000]
    q = pgs.synth.read_from_ref(ref[:120_000], 777, 2500, sub_rate=0.03, indel_rate=0.01)[0].tobytes()
    for sc in (dict(match=0.7, mismatch=-0.3, gap=0.1), dict(match=1.1, mismatch=-0.9, gap=0.37)):
        g, e = ctx.align(q, sub, 0, **sc), oracle.align(q, sub, 0, **sc)
        worst = max(worst, abs(g["score"] - e["score"]))
        if any(g[k] != e[k] for k in ("score", "pos", "end_x", "end_y", "cons_x", "cons_y")):
            bad.append((sc, "2500 rows", g["score"], e["score"], g["pos"], e["pos"]))
    assert not bad, "max |delta score| = %g; %r" % (worst, bad[:5])


def test_tiny_gap_has_no_rounding_safe_margin(ctx, oracle, pgs):
    """A gap penalty within a factor 64 of half an ulp of the largest cell value (float32 H - g may stall): the margins
    of DESIGN.md §3.3 do not exist, so the problem takes the whole-matrix path (small) or fails loudly (large) — never
    the tiled instance.  Also the overflow of the margin's integer cast (gap = 1e-20)."""
    ref = pgs.synth.dna(84, 3000).tobytes()
    q = ref[1000:1100]
    for gap in (1e-20, 1e-6):
        g, e = ctx.align(q, ref, 0, 3.25, -3.5, gap), oracle.align(q, ref, 0, 3.25, -3.5, gap)
        _cmp(g, e, "tiny gap %g" % gap)
    mid = pgs.synth.dna(85, 300_000).tobytes()                         # whole-matrix path (the LDS anti-diagonal kernel)
    _cmp(ctx.align(mid[5000:5600], mid, 0, 3.25, -3.5, 1e-6), oracle.align(mid[5000:5600], mid, 0, 3.25, -3.5, 1e-6), "tiny gap, 600 x 300k")
    assert ctx.last_kernel()["cells"] == 0                             # not the tiled score kernel
    big = pgs.synth.dna(85, 40_000_000).tobytes()                      # beyond the whole-matrix scratch budget
    with pytest.raises(pgs.MI355Error) as ei:
        ctx.align(big[5000:5600], big, 0, 3.25, -3.5, 1e-6)
    assert ei.value.code == -95                                        # MI355_SW_ENOTSUP, with a message


def test_full_size_against_lean_oracle(ctx, oracle, pgs):
    """Config 3 at FULL reference size against the oracle: 150 bp x 50 Mbp does not fit a matrix (30 GB), so the
    oracle's rolling-column locate gives (score, argmax) for the whole reference, and the traceback is checked
    against the oracle's full aligner on the 20 kbp of reference that end at the argmax (the walk reads nothing
    to the right of it; SURVEY.md App. A.5 validates the window)."""
    from concurrent.futures import ThreadPoolExecutor
    ref = pgs.synth.dna(3, 50_000_000)
    refb = ref.tobytes()
    reads = [pgs.synth.read_from_ref(ref, 4 + 31 * k, 150, sub_rate=0.02, indel_rate=0.004)[0].tobytes() for k in range(3)]
    reads.append(pgs.synth.dna(4242, 150).tobytes())                 # unrelated read: background maximum, ties likely
    jobs = [(q, sem) for q in reads for sem in (0, 1)]
    with ThreadPoolExecutor(8) as ex:                                  # ctypes releases the GIL
        exp = list(ex.map(lambda js: oracle.locate(js[0], refb, js[1]), jobs))
    ctx.set_reference(ref)
    ctx.batch_upload(reads)
    got = {0: ctx.batch_run(semantics=0), 1: ctx.batch_run(semantics=1)}
    for (q, sem), (mx, ix, iy) in zip(jobs, exp):
        r = got[sem][reads.index(q)]
        assert (r["score"], r["end_x"], r["end_y"]) == (mx, ix, iy), (sem, reads.index(q))
        # traceback: never conditional — the oracle walks from the FULL-size argmax (the uint8 storage order depends on
        # the full problem's ncols, so the start cell is not re-derived on the window); the window only supplies H
        lo = max(0, iy - 20_000)
        w = oracle.trace_from(q, refb[lo:iy], sem, ix, iy - lo)
        assert w["score"] == mx                                        # the window is long enough: H(start) is exact
        assert (r["cons_x"], r["cons_y"], r["pos"]) == (w["cons_x"], w["cons_y"], w["pos"] + lo), (sem, reads.index(q))


def test_fuzz_paths_vs_oracle(ctx, oracle, pgs):
    """Seeded fuzz across the host's path selection: tile shapes (8/16 lanes, every R class edge), strip
    threshold, short-reference threshold (1024), uint8 |y| <= |x|+1 rule, unusual scorings (large match, small
    gap -> long warm-up, fractional -> float32 instance), repeats and low-complexity inputs."""
    rng = np.random.default_rng(20261003)
    lens = [1, 2, 15, 16, 17, 63, 64, 65, 100, 104, 105, 127, 128, 129, 150, 152, 153, 160, 200, 208, 209, 255, 256, 257,
            300, 511, 512, 513, 600]
    scorings = [(3.0, -3.0, 2.0)] * 4 + [(2.0, -1.0, 1.0), (5.0, -4.0, 3.0), (10.0, -2.0, 1.0), (1.0, -1.0, 4.0),
                                         (3.5, -2.25, 1.5), (2.0, -7.0, 2.0), (100.0, -90.0, 60.0)]
    nbad = 0
    for t in range(220):
        m = int(rng.choice(lens))
        n = int(rng.choice([1, 7, 150, 151, 152, 600, 1023, 1024, 1025, 3000, 9000, 40000]))
        kind = t % 5
        if kind == 0:
            unit = pgs.synth.dna(int(rng.integers(1, 1 << 30)), int(rng.integers(1, 9))).tobytes()
            ref = (unit * (n // len(unit) + 1))[:n]
        else:
            ref = pgs.synth.dna(int(rng.integers(1, 1 << 30)), n).tobytes()
        if kind in (1, 2) and n > m + 2:
            o = int(rng.integers(0, n - m))
            q = bytearray(ref[o:o + m])
            for i in range(m):
                if rng.random() < 0.04:
                    q[i] = b"ACGT"[int(rng.integers(0, 4))]
            q = bytes(q)
        elif kind == 0:
            q = (ref * 3)[:m] if len(ref) >= 1 else b"A" * m
            q = (q * (m // max(1, len(q)) + 1))[:m]
        else:
            q = pgs.synth.dna(int(rng.integers(1, 1 << 30)), m).tobytes()
        sem = int(rng.integers(0, 2))
        ma, mi, g = scorings[int(rng.integers(0, len(scorings)))]
        exp = oracle.align(q, ref, sem, ma, mi, g)
        got = ctx.align(q, ref, sem, ma, mi, g)
        for k in ("score", "pos", "end_x", "end_y", "cons_x", "cons_y"):
            if got[k] != exp[k]:
                nbad += 1
                print("FUZZ MISMATCH t=%d m=%d n=%d sem=%d sc=%s key=%s got=%r exp=%r" % (t, m, n, sem, (ma, mi, g), k, got[k], exp[k]))
                break
    assert nbad == 0


def test_fuzz_batches_and_splits(ctx, oracle, pgs):
    """Seeded fuzz of ragged batches (several length classes in one call, odd counts, empty and unmatched
    reads) and of the split aligner with all four engine combinations."""
    rng = np.random.default_rng(77)
    for t in range(6):
        n = int(rng.choice([2000, 9000, 70000]))
        ref = pgs.synth.dna(int(rng.integers(1, 1 << 30)), n).tobytes()
        qs = []
        for k in range(int(rng.integers(3, 40))):
            m = int(rng.choice([0, 1, 30, 64, 100, 125, 150, 151, 250, 400, 520, 700]))
            if m and rng.random() < 0.7 and n > m + 1:
                o = int(rng.integers(0, n - m))
                qs.append(ref[o:o + m])
            else:
                qs.append(pgs.synth.dna(int(rng.integers(1, 1 << 30)), m).tobytes() if m else b"")
        for sem in (0, 1):
            for q, got in zip(qs, ctx.align_batch(qs, ref, semantics=sem)):
                _cmp(got, oracle.align(q, ref, sem), "fuzz batch t=%d sem=%d |q|=%d" % (t, sem, len(q)))
    for t in range(24):
        n = int(rng.choice([3000, 20000, 60000]))
        m = int(rng.choice([20, 60, 150, 300]))
        ref = pgs.synth.dna(int(rng.integers(1, 1 << 30)), n).tobytes()
        o = int(rng.integers(0, n - m))
        q = ref[o:o + m]
        npiece = int(rng.choice([1, 2, 3, 5, 8, 17]))
        ratio = float(rng.choice([2.0, 1.0, 1.5]))
        sm, la = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        ma, mi, g = [(3.0, -3.0, 2.0), (2.0, -1.0, 1.0), (4.0, -6.0, 3.0)][t % 3]
        if oracle.make_string_range(npiece, m, n, ratio) is None:
            continue
        exp = oracle.align_split(q, ref, npiece, ratio, sm, la, ma, mi, g)
        got = ctx.align_split(q, ref, npiece, ratio, sm, la, ma, mi, g)
        assert got["piece"] == exp["piece"]
        _cmp(got, {k: exp[k] for k in ("score", "pos", "cons_x", "cons_y")}, "fuzz split t=%d" % t)


def test_error_codes(ctx, pgs, oracle):
    """Error behaviour through the C-ABI: inputs outside kernel coverage fail loudly (no silent fallback), the
    reference's constructor asserts map to MI355_SW_ERANGE, bad arguments to MI355_SW_EINVAL."""
    ref = pgs.synth.dna(5, 3_000_000)
    q = ref[1000:1150].tobytes()
    big = pgs.synth.dna(6, 120_000_000)
    with pytest.raises(pgs.MI355Error) as e:
        ctx.align(q, big, 0, 3.0, -3.0, 0.0)                        # zero gap penalty: no finite warm-up margin, and the
    assert e.value.code == -95 and "coverage" in str(e.value)      # whole matrix exceeds the 16 GB decision scratch
    del big
    with pytest.raises(pgs.MI355Error) as e:
        ctx.align_split("A" * 100, "C" * 120, 4, 2.0)               # overlap > piece length (plocalaligner.cpp:52)
    assert e.value.code == -34
    with pytest.raises(pgs.MI355Error) as e:
        ctx.align(q, ref, 7)                                        # unknown semantics
    assert e.value.code == -22
    # a zero gap penalty has no finite warm-up margin: such problems run on the whole matrix while it fits the
    # scratch budget, and still match the oracle
    assert ctx.align("GGTTGACTA", "TGTTACGG", 0, 3.0, -3.0, 0.0)["score"] > 0
    sub = ref[:120_000].tobytes()
    _cmp(ctx.align(q, sub, 0, 3.0, -3.0, 0.0), oracle.align(q, sub, 0, 3.0, -3.0, 0.0), "zero gap, whole matrix")


@pytest.mark.parametrize("sem", [0, 1])
def test_long_query_pairs(ctx, oracle, pgs, sem):
    """Several long queries per length class, so that the packed (two queries per register) instances run on
    whole-wavefront tiles: one strip (<= 2048 rows) and strip-mined (> 2048 rows), odd counts included."""
    ref = pgs.synth.dna(91, 90_000)
    refb = ref.tobytes()
    qs = []
    for k, m in enumerate((900, 1000, 1024, 1800, 2048, 2000, 2500, 3000, 2600)):
        qs.append(pgs.synth.read_from_ref(ref, 1200 + k, m, sub_rate=0.03, indel_rate=0.006)[0].tobytes())
    for q, got in zip(qs, ctx.align_batch(qs, refb, semantics=sem)):
        _cmp(got, oracle.align(q, refb, sem), "long pairs sem=%d |q|=%d" % (sem, len(q)))


def test_reference_longer_than_2g_columns(ctx, pgs, oracle):
    """Maximum sizes: a 2.2 Gbp reference (column indices beyond 2^31).  Reads cut near the far end must be
    found at their 64-bit columns; a window around each hit is re-aligned by the oracle and the consensus and
    start position must agree after shifting by the window offset."""
    n = 2_200_000_000
    ref = np.empty(n, dtype=np.uint8)
    step = 100_000_000
    for k in range(0, n, step):                               # chunked: keeps host temporaries small
        ref[k:k + step] = pgs.synth.dna(1000 + k // step, min(step, n - k))
    offs = [n - 150, 2_147_483_648 - 75, 2_147_483_648 + 3, 2_190_000_123, 17]
    reads = []
    for k, o in enumerate(offs):
        r = ref[o:o + 150].copy()
        if k >= 2:
            r[40 + k] = ord("A") if r[40 + k] != ord("A") else ord("C")     # one substitution
        reads.append(r.tobytes())
    ctx.set_reference(ref)
    ctx.batch_upload(reads)
    for sem in (0, 1):
        res = ctx.batch_run(semantics=sem)
        for o, q, r in zip(offs, reads, res):
            lo = max(0, o - 600)
            exp = oracle.align(q, ref[lo:min(n, o + 750)].tobytes(), sem)
            assert r["score"] == exp["score"] and r["end_x"] == exp["end_x"], (sem, o)
            assert r["end_y"] == exp["end_y"] + lo and r["pos"] == exp["pos"] + lo, (sem, o, r["end_y"], r["pos"])
            assert r["cons_x"] == exp["cons_x"] and r["cons_y"] == exp["cons_y"], (sem, o)
    ctx.set_reference(b"ACGT")                                 # release the 2.2 GB device copy


@pytest.mark.parametrize("sem", [0, 1])
def test_very_long_queries_strip_rounds(ctx, oracle, pgs, sem):
    """Queries beyond one round of the pipelined strip kernel (16 wavefronts x 64 lanes x 16 rows = 16 384 rows):
    locate and traceback hand bottom rows from round to round through global memory."""
    ref = pgs.synth.dna(311, 45_000)
    refb = ref.tobytes()
    for k, m in enumerate((13_000, 20_000)):
        q = pgs.synth.read_from_ref(ref, 320 + k, m, sub_rate=0.02, indel_rate=0.004)[0].tobytes()
        _cmp(ctx.align(q, refb, sem), oracle.align(q, refb, sem), "very long sem=%d |q|=%d" % (sem, m))


def test_long_queries_table_scoring(ctx, oracle, pgs):
    """Queries beyond 512 rows with a substitution table (float engine): locate and traceback on the strip kernel's
    table instance (scores from LDS), including one beyond a single round of strips."""
    ref = pgs.synth.protein(411, 40_000)
    refb = ref.tobytes()
    lut = pgs.synth.make_lut(77)
    for k, (m, gap) in enumerate(((700, 2.0), (3_000, 3.0), (17_500, 2.0))):
        q = pgs.synth.read_from_ref(ref, 420 + k, m, sub_rate=0.05, indel_rate=0.01)[0].tobytes()
        _cmp(ctx.align(q, refb, 0, 3.0, -3.0, gap, lut), oracle.align(q, refb, 0, 3.0, -3.0, gap, lut), "table |q|=%d" % m)
    # identity-like scoring the compare-based instances refuse (mismatch >= 0) also goes through the table
    q = pgs.synth.read_from_ref(ref, 430, 2_500, sub_rate=0.05, indel_rate=0.01)[0].tobytes()
    _cmp(ctx.align(q, refb, 0, 2.0, 0.0, 3.0), oracle.align(q, refb, 0, 2.0, 0.0, 3.0), "mismatch 0")


def test_resident_reference_is_rechecked(ctx, oracle, pgs):
    """One-by-one calls keep the last reference resident and start on it while its content is re-hashed in the
    background: a same-length reference with different bytes must not be served from the stale copy."""
    n = 3_000_000
    ref_a = pgs.synth.dna(501, n)
    ref_b = ref_a.copy()
    ref_b[1_000_000:1_000_400] = pgs.synth.dna(502, 400)             # same length, 400 bases differ
    q = ref_b[1_000_100:1_000_250].tobytes()                           # exact match only in ref_b
    for sem in (0, 1):
        ra = ctx.align(q, ref_a.tobytes(), sem)
        rb = ctx.align(q, ref_b.tobytes(), sem)
        ra2 = ctx.align(q, ref_a.tobytes(), sem)
        assert rb["score"] == (450 if sem == 0 else 255)
        if sem == 0:
            assert ra["score"] < rb["score"]
        assert all(ra[k] == ra2[k] for k in ("score", "pos", "end_x", "end_y", "cons_x", "cons_y"))
        lo = 999_000
        exp = oracle.align(q, ref_b[lo:1_002_000].tobytes(), sem)
        assert rb["score"] == exp["score"] and rb["cons_x"] == exp["cons_x"] and rb["pos"] == exp["pos"] + lo
        sp = ctx.align_split(q, ref_b.tobytes(), 5, 2.0, sem, sem)
        assert sp["score"] == rb["score"] and sp["pos"] == rb["pos"]
        sp_a = ctx.align_split(q, ref_a.tobytes(), 5, 2.0, sem, sem)
        assert sp_a["score"] == ra["score"]


def test_no_positive_score_possible(ctx, oracle, pgs):
    """Scoring that cannot produce a positive cell (uint8 engine with a match score that truncates to 0; float engine
    with non-positive scores): the defined no-match result, whatever the problem size."""
    ref = pgs.synth.dna(601, 20_000).tobytes()
    q = pgs.synth.dna(602, 15_000).tobytes()
    for sem, sc in ((1, (0.5, -0.25, 0.25)), (0, (0.0, -1.0, 1.0)), (0, (-1.0, -2.0, 2.0))):
        got = ctx.align(q, ref, sem, *sc)
        assert got["score"] == 0 and got["pos"] == 0 and got["cons_x"] == "" and got["end_x"] == 0
        small = oracle.align(q[:300], ref[:2000], sem, *sc)
        assert small["score"] == 0 and small["cons_x"] == ""


def test_float16_cells_at_their_exactness_bound(ctx, oracle, pgs):
    """Packed float16 cells are used while match * (|x| + 1) <= 2040 (integers up to 2048 are exact in float16).
    Perfect-match reads right at and just past that bound — past it the packed integer instance takes over —
    must give the exact scores, positions and consensus either way."""
    ref = pgs.synth.dna(701, 30_000)
    refb = ref.tobytes()
    for match, length in ((4.0, 509), (4.0, 510), (5.0, 407), (5.0, 408), (7.0, 290), (7.0, 291), (3.0, 512), (15.0, 135)):
        reads = [ref[o:o + length].tobytes() for o in (100, 7_777, 20_000)]
        reads.append(pgs.synth.read_from_ref(ref, 710 + length, length, sub_rate=0.02, indel_rate=0.004)[0].tobytes())
        got = ctx.align_batch(reads, refb, semantics=0, match=match, mismatch=-2.0, gap=1.0)
        for q, g in zip(reads, got):
            _cmp(g, oracle.align(q, refb, 0, match, -2.0, 1.0), "bound match=%g |q|=%d" % (match, length))
        assert got[0]["score"] == match * length


def test_float32_cells_scaling_extremes(ctx, oracle, pgs):
    """The float32 score instance holds H * 2^-k (a pure exponent shift, exact): large and tiny fractional scorings
    must reproduce the oracle's float results bit for bit."""
    ref = pgs.synth.dna(801, 25_000)
    refb = ref.tobytes()
    reads = [pgs.synth.read_from_ref(ref, 810 + k, 150 + 37 * k, sub_rate=0.03, indel_rate=0.006)[0].tobytes() for k in range(5)]
    for sc in ((1234.5, -777.25, 333.125), (0.001953125, -0.0009765625, 0.00048828125), (98765.0, -43210.5, 12345.75)):
        got = ctx.align_batch(reads, refb, semantics=0, match=sc[0], mismatch=sc[1], gap=sc[2])
        for q, g in zip(reads, got):
            _cmp(g, oracle.align(q, refb, 0, *sc), "scaling %r |q|=%d" % (sc, len(q)))
        one = ctx.align(reads[0], refb, 0, *sc)
        _cmp(one, oracle.align(reads[0], refb, 0, *sc), "scaling lone %r" % (sc,))


def test_strip_pipeline_wait_expiry_is_reported(ctx, oracle, pgs):
    """sw_strip_kernel's bounded waits: with the test hook fault_inject=strip_stall (mi355_sw_set_option only — the
    environment cannot switch it on) wavefront 0 of every workgroup never reports progress, the strip below runs into the
    spin limit, the workgroup raises its status word and DRAINS (nothing hangs), and the host reports an error instead of a
    result.  The context stays usable afterwards."""
    ref = pgs.synth.dna(86, 60_000)
    q = pgs.synth.read_from_ref(ref, 87, 1500, sub_rate=0.02, indel_rate=0.004)[0].tobytes()   # three strips of 640 rows
    refb = ref.tobytes()
    ctx.set_option("fault_inject", "strip_stall")
    try:
        with pytest.raises(pgs.MI355Error) as ei:
            ctx.align(q, refb, 0)
        assert "wait expired" in str(ei.value)
    finally:
        ctx.set_option("fault_inject", None)
    _cmp(ctx.align(q, refb, 0), oracle.align(q, refb, 0), "after the injected stall")


def test_config4_uniprot_shape_20k(ctx, oracle, pgs):
    """configs[3] shape under test at a meaningful size: 20 000 UniProt-shaped protein sequences (log-normal lengths,
    2 .. 35 000 residues) as FIRST argument against the 144-aa P02232 query as SECOND (src/mpi_sw_solve_uniprot.cpp:120),
    default scoring, float engine — EVERY (score, pos, end, consensus) against the oracle; the same batch through
    LPT partitions (dist.shard_lpt, the query-sharding layout of SURVEY.md §8e) fed to real GPU callables, and through
    two device contexts behind one handle, with the batch best (score, lowest index)."""
    from concurrent.futures import ThreadPoolExecutor
    from parallel_genomeseq_amd import dist as pd
    n = 20_000
    lens = pgs.synth.lognormal_lengths(5, n)
    allres = pgs.synth.protein(5, int(lens.sum()))
    offs = np.concatenate([[0], np.cumsum(lens)])
    seqs = [allres[offs[k]:offs[k + 1]].tobytes() for k in range(n)]
    query = pgs.synth.P02232
    assert len(query) == 144 and lens.min() >= 2
    with ThreadPoolExecutor(8) as ex:
        exp = list(ex.map(lambda s: oracle.align(s, query, 0), seqs))
    got = ctx.align_batch(seqs, query, semantics=0)
    for k, (g, e) in enumerate(zip(got, exp)):
        _cmp(g, e, "uniprot[%d] |x|=%d" % (k, lens[k]))
    scores = np.array([e["score"] for e in exp])
    # the same call as a struct-of-arrays view (mi355_sw_batch_run_view): arrays + strings read through the view
    raw = ctx.batch_run(semantics=0, raw=True)
    assert np.array_equal(raw["score"], scores.astype(np.float32))
    for key in ("pos", "end_x", "end_y"):
        assert raw[key].tolist() == [e[key] for e in exp], key
    assert raw["cons_len"].tolist() == [len(e["cons_x"]) for e in exp]
    for k in range(0, n, 37):
        assert ctx.consensus(k) == (exp[k]["cons_x"], exp[k]["cons_y"]), k
    # the host-built job lists (option no_devlist) must agree with the device-built ones
    ctx.set_option("no_devlist")
    try:
        for g, e in zip(ctx.align_batch(seqs[:3000], query, semantics=0), exp[:3000]):
            _cmp(g, e, "uniprot, host-built lists")
    finally:
        ctx.set_option("no_devlist", None)
    # four LPT partitions by cell count, each aligned on its own (what four ranks would do), scattered back
    parts = pd.shard_lpt(lens * len(query), 4)
    loads = [int(lens[p].sum()) for p in parts]
    assert max(loads) - min(loads) <= int(lens.max())
    raw = np.zeros(n, dtype=np.float32)
    pos = np.zeros(n, dtype=np.int64)
    for p in parts:
        out = ctx.align_batch([seqs[i] for i in p], query, semantics=0, raw=True)
        raw[p], pos[p] = out["score"], out["pos"]
    assert np.array_equal(raw, scores.astype(np.float32)) and pos.tolist() == [e["pos"] for e in exp]
    idx, res, gathered = pd.align_queries_sharded(lambda qs: ctx.align_batch(qs, query, semantics=0), seqs,
                                                  weights=lens * len(query))       # world size 1: the whole batch
    assert np.array_equal(gathered["score"], scores.astype(np.float32))
    assert pd.allreduce_best(float(scores.max()), int(scores.argmax())) == (float(scores.max()), int(scores.argmax()))
    m = pgs.MultiContext([0, 0])
    try:
        out, best = m.align_batch(seqs, query, semantics=0, raw=True)
        assert np.array_equal(out["score"], scores.astype(np.float32)) and out["pos"].tolist() == [e["pos"] for e in exp]
        assert best == int(scores.argmax())
    finally:
        m.close()


def test_config5_full_size_split_equals_whole(ctx, oracle, pgs):
    """configs[4] at FULL size (one 10 kbp query against 250 Mbp; the CPU oracle cannot hold 2.5e12 cells): the
    16-piece OMPParallelLocalAligner split (overlap 2.0, plocalaligner.cpp:44-67,105-143) must give the whole-reference
    result — on one context and with the pieces dealt to two contexts — the planted position is recovered, and the
    traceback is checked against the ORACLE on the 26 kbp window that ends at the argmax (long enough for the start
    cell to be exact: |x| + 3|x|/2 columns)."""
    n, m, npiece = 250_000_000, 10_000, 16
    ref = pgs.synth.dna(6, n)
    q, off = pgs.synth.read_from_ref(ref, 7, m, sub_rate=0.01, indel_rate=0.001)
    q = q.tobytes()
    ctx.set_reference(ref)
    ctx.batch_upload([q])
    ranges = pgs.capi.make_string_range(npiece, m, n, 2.0)
    assert ranges[1][0] == ranges[0][1] - 2 * m and ranges[-1][1] == n
    refb = ref.tobytes()
    for sem in (0, 1):
        whole = ctx.batch_run(semantics=sem)[0]
        if sem == 0:
            assert abs(whole["pos"] - (off + 1)) < 300 and whole["score"] > 20_000
        else:
            # 10 000 rows saturate the uint8 engine everywhere (random 10 kbp x 15 Mbp already scores ~7 700 in float): the
            # answer is the FIRST 255 in the skewed storage order — in the corner triangle at the end of the reference,
            # which that order visits early — not the planted copy
            assert whole["score"] == 255 and whole["end_x"] + whole["end_y"] > n
        mx = ctx.score_ranges(ranges, semantics=sem)[:, 0]
        assert mx.max() == whole["score"]
        winner = int(np.argmax(mx))                                   # first strictly greatest (plocalaligner.cpp:125)
        split = ctx.align_split(q, refb, npiece, 2.0, sem, sem)
        assert split["piece"] == winner
        if sem == 0:                                                  # (the uint8 storage order is piece-local: SURVEY App. A.6)
            for k in ("score", "pos", "end_y", "cons_x", "cons_y"):
                assert split[k] == whole[k], k
        lo = whole["end_y"] - (26_000 if sem == 0 else 40_000)
        w = oracle.trace_from(q, refb[lo:whole["end_y"]], sem, whole["end_x"], whole["end_y"] - lo)
        assert w["score"] == whole["score"]
        assert (w["cons_x"], w["cons_y"], w["pos"] + lo) == (whole["cons_x"], whole["cons_y"], whole["pos"])
        mm = pgs.MultiContext([0, 0])
        try:
            ms = mm.align_split(q, refb, npiece, 2.0, sem, sem)
        finally:
            mm.close()
        for k in ("score", "pos", "end_x", "end_y", "cons_x", "cons_y", "piece"):
            assert ms[k] == split[k], (sem, k)


def test_u8_unsaturated_sweep_edges(ctx, oracle, pgs):
    """The uint8 engine's score pass runs WITHOUT saturation and clamps the published maxima at 255 (host_score.h
    make_buckets).  Edges of that argument: maxima of exactly 252 / 255 / 258 before clamping (84, 85, 86 matches), a read
    that saturates, decays and hits again further right (later sub-chunks differ between the two recurrences; the first
    one decides), non-default uint8 scorings incl. mismatch penalty 0 and match 255, batches (packed float16 cells) and
    lone calls (float32 cells), against the oracle's saturating rule."""
    rng = np.random.default_rng(77)
    ref = pgs.synth.dna(91, 400_000)
    refb = bytearray(ref.tobytes())
    reads = []
    for k, m in enumerate((84, 85, 86, 150, 150, 300, 511)):
        at = 10_000 + 50_000 * k
        reads.append(bytes(refb[at:at + m]))
    long_read = bytes(refb[200_000:200_400])                         # 400 matches: saturates early
    refb[330_000:330_400] = long_read                                # ... and occurs again much further right
    degraded = bytearray(long_read)
    for i in range(90, 400, 7):                                      # saturate, decay, saturate again inside one hit
        degraded[i] = ord("ACGT"[("ACGT".index(chr(degraded[i])) + 1) % 4])
    reads += [long_read, bytes(degraded), pgs.synth.dna(92, 150).tobytes()]
    refb = bytes(refb)
    for early in (False, True):
        # (the SWEEP is what this test is about: once with the early exit of DESIGN.md L8a switched off, once as the library runs)
        ctx.set_option("no_u8_early", None if early else True)
        try:
            for sc in (dict(), dict(match=5.0, mismatch=-4.0, gap=3.0), dict(match=2.0, mismatch=0.0, gap=1.0),
                       dict(match=255.0, mismatch=-255.0, gap=200.0), dict(match=7.9, mismatch=-1.2, gap=1.99)):
                exp = _pmap(lambda q: oracle.align(q, refb, 1, **sc), reads)
                got = ctx.align_batch(reads, refb, semantics=1, **sc)
                for k, (g, e) in enumerate(zip(got, exp)):
                    _cmp(g, e, ("u8 batch", sc, k, early))
                for k in (0, 1, 2, 7, 8):
                    _cmp(ctx.align(reads[k], refb, 1, **sc), exp[k], ("u8 lone", sc, k, early))
            if not early:
                assert "unsaturated" in ctx.last_kernel()["name"]
        finally:
            ctx.set_option("no_u8_early", None)


def test_split_calls_on_the_single_alignment_chain(ctx, oracle, pgs):
    """OMPParallelLocalAligner with default scoring (what src/sw_solve_small.cpp:82 / sw_solve_big.cpp:78 construct) runs
    score kernel + solo kernel over ALL pieces in one chain (host_solo.h): the first piece with the strictly greatest
    maximum wins (plocalaligner.cpp:122-129) — equal hits in different pieces, 2 .. 64 pieces, both engines, reads that
    straddle a cut, a read with no good hit — against the oracle's serial split aligner."""
    ref = bytearray(pgs.synth.dna(95, 300_000).tobytes())
    q = bytes(ref[40_000:40_150])
    ref[220_000:220_150] = q                                         # the same hit again in a later piece
    refb = bytes(ref)
    refa = np.frombuffer(refb, dtype=np.uint8)
    reads = [q, pgs.synth.read_from_ref(refa, 96, 150)[0].tobytes(), pgs.synth.read_from_ref(refa, 97, 300)[0].tobytes(),
             pgs.synth.dna(98, 120).tobytes()]
    for npiece in (2, 7, 16, 64):
        ranges = oracle.make_string_range(npiece, 150, len(refb), 2.0)
        reads.append(refb[ranges[1][0] - 60:ranges[1][0] + 90])      # straddles the left edge of piece 1 (inside the overlap)
        for sem in (0, 1):
            for x in reads:
                got = ctx.align_split(x, refb, npiece, 2.0, sem, sem)
                exp = oracle.align_split(x, refb, npiece, 2.0, sem, sem)
                _cmp(got, exp, ("split", npiece, sem, len(x)))
                assert got["piece"] == exp["piece"]
        reads.pop()


def test_float_engine_saturating_sweep(ctx, oracle, pgs):
    """Float-engine reads beyond float16's exact range (match * (|x| + 1) > 2040, |x| <= 2048) are swept on packed
    float16 cells that SATURATE at 2048; every sub-chunk whose maximum reaches the cap is re-evaluated exactly
    (sw_strip_kernel in maximum mode) and the greatest exact value, first in storage order, wins (host_pipeline.h
    locate_saturated).  Cases: hits far above the cap at several places with different true scores (the later, better
    one must win), equal hits (the first one must win), a maximum of exactly 2048 and of 2046 / 2049, reads that never
    reach the cap next to ones that do, lone calls, and a background that saturates everywhere (flag budget exceeded:
    the exact int16 sweep takes over)."""
    ref = bytearray(pgs.synth.dna(301, 200_000).tobytes())
    def mutate(b, every, start):
        b = bytearray(b)
        for i in range(start, len(b), every):
            b[i] = ord("ACGT"[("ACGT".index(chr(b[i])) + 1) % 4])
        return bytes(b)
    r1000 = bytes(ref[20_000:21_000])
    ref[60_000:61_000] = mutate(r1000, 97, 40)                      # a worse copy first ... (both far above the cap)
    ref[150_000:151_000] = r1000                                    # ... an exact copy later: three places, best = 20 000
    ref[100_000:101_000] = mutate(r1000, 203, 11)
    r1500 = bytes(ref[30_000:31_500])
    ref[170_000:171_500] = r1500                                    # equal hits: the first wins
    r2048 = bytes(ref[40_000:42_048])
    refb = bytes(ref)
    refa = np.frombuffer(refb, dtype=np.uint8)
    reads = [r1000, mutate(r1000, 50, 7), r1500, r2048, bytes(ref[70_000:70_682]), bytes(ref[75_000:75_683]),
             bytes(ref[80_000:80_700]), pgs.synth.dna(302, 900).tobytes(),
             pgs.synth.read_from_ref(refa, 303, 1200, sub_rate=0.05, indel_rate=0.01)[0].tobytes(),
             pgs.synth.read_from_ref(refa, 304, 2000, sub_rate=0.25, indel_rate=0.05)[0].tobytes()]
    exp = _pmap(lambda q: oracle.align(q, refb, 0), reads)
    got = ctx.align_batch(reads, refb, semantics=0)
    name = ctx.last_kernel()["name"]
    for k, (g, e) in enumerate(zip(got, exp)):
        _cmp(g, e, ("saturating sweep", k, len(reads[k])))
    assert "f16x2" in name and "saturating" in name, name
    assert exp[0]["score"] == 3000.0 and exp[4]["score"] == 2046.0 and exp[5]["score"] == 2049.0
    _cmp(ctx.align(r1500, refb, 0), exp[2], "lone 1500")
    # exactly 2048 (the cap itself) and fractional scorings on the same path
    q512 = [bytes(ref[90_000:90_512]), bytes(ref[95_000:95_513]), mutate(bytes(ref[110_000:110_600]), 61, 3)]
    for sc in ((4.0, -3.0, 2.0), (3.5, -2.25, 1.75), (12.0, -9.0, 5.0)):
        got = ctx.align_batch(q512 + reads[:2], refb, semantics=0, match=sc[0], mismatch=sc[1], gap=sc[2])
        for q, g in zip(q512 + reads[:2], got):
            _cmp(g, oracle.align(q, refb, 0, *sc), ("saturating sweep", sc, len(q)))
    # a background that reaches the cap in a wide region: many flagged sub-chunks, all re-evaluated exactly
    poly = bytearray(refb)
    poly[100_000:180_000] = b"A" * 80_000
    poly = bytes(poly)
    pa = [b"A" * 800, b"A" * 700 + bytes(ref[10_000:10_200]), r1000]
    got = ctx.align_batch(pa, poly, semantics=0)
    for q, g in zip(pa, got):
        _cmp(g, oracle.align(q, poly, 0), ("saturated region", len(q)))
    # ... and everywhere: more flags than the budget (64 per query + 1024), the exact int16 sweep runs instead
    poly = b"A" * 450_000
    pa = [b"A" * 800, b"A" * 750 + b"C" + b"A" * 49, b"A" * 799 + b"C", b"C" + b"A" * 799]
    got = ctx.align_batch(pa, poly, semantics=0)
    assert "i16x2" in ctx.last_kernel()["name"], ctx.last_kernel()["name"]
    for q, g in zip(pa, got):
        _cmp(g, oracle.align(q, poly, 0), ("saturated background", len(q)))


def test_lone_reads_by_length_with_n(ctx, oracle, pgs):
    """One read per call — the reference drivers' unchanged loop — at 120 .. 2048 bp against a reference that contains `N`
    (six codes with the pad code: the code-pair profile of the twin tiles holds 36 pairs), both engines: the single-alignment
    chain (<= 320 rows), twin tiles with the code-pair profile (<= 512 rows), float32 cells on whole-wavefront tiles beyond,
    tile lengths off the power of two, and the few-problem strip instances of locate / traceback."""
    rng = np.random.default_rng(2024)
    ref = pgs.synth.dna(611, 300_000).copy()
    ref[rng.integers(0, len(ref), 600)] = ord("N")
    ref[150_000:150_040] = ord("N")
    refb = ref.tobytes()
    for k, m in enumerate((120, 150, 333, 400, 700, 1000, 2048)):
        q = pgs.synth.read_from_ref(ref, 620 + k, m, sub_rate=0.03, indel_rate=0.005)[0].copy()
        q[rng.integers(0, len(q), max(1, m // 60))] = ord("N")
        qb = q.tobytes()
        for sem in (0, 1):
            _cmp(ctx.align(qb, refb, sem), oracle.align(qb, refb, sem), ("lone read", m, sem))
    name = ctx.last_kernel()["name"]
    qb = pgs.synth.read_from_ref(ref, 640, 150)[0].tobytes()
    _cmp(ctx.align(qb, refb, 0), oracle.align(qb, refb, 0), "lone 150")
    assert "code-pair profile" in ctx.last_kernel()["name"], (name, ctx.last_kernel()["name"])


def test_sampled_maximum_candidates(ctx, oracle, pgs):
    """Batches sweep with the running maximum folded every 4th step (sw_score_kernel MK = 4): per sub-chunk the sweep holds a
    lower bound within 3 gaps of the truth, and every sub-chunk within that slack of the query's key is re-evaluated exactly.
    Edges of that argument: hits that END in the last columns of a sub-chunk / of a tile / of the reference (their value is
    seen by the next fold, possibly in the next sub-chunk, or only by the fold of the tile's last step), near-copies whose
    scores lie 1 .. 6 below the best one in other sub-chunks (candidates that must lose), equal copies (the first in the
    engine's storage order must win), both engines, against the oracle."""
    n = 3 * 65536 + 4096
    ref = bytearray(pgs.synth.dna(911, n).tobytes())
    reads = [bytes(ref[1000 + 331 * k:1000 + 331 * k + 150]) for k in range(6)]
    def put(at_end, seq):                                            # plant seq so that its last base sits at 0-based column at_end
        ref[at_end - len(seq) + 1:at_end + 1] = seq
    def worse(seq, nsub):                                            # nsub substitutions near the start: score - 6 each (3/-3/2)
        b = bytearray(seq)
        for t in range(nsub):
            b[5 + 9 * t] = ord("ACGT"[("ACGT".index(chr(b[5 + 9 * t])) + 1) % 4])
        return bytes(b)
    put(70_000 + 255 - 70_000 % 256, reads[0])                       # ends in the last column of a sub-chunk
    put(65536 - 1, reads[1])                                         # ... of a tile (65536-column tiles at this size, if chosen)
    put(n - 1, reads[2])                                             # ... of the reference
    put(120_000, reads[3]); put(150_000, reads[3])                   # equal copies
    put(90_001, worse(reads[4], 1))                                  # the original at 1000 + 331 * 4 stays the best; this one is 6 below
    put(180_002, reads[5][:149])                                     # 3 below the original (one base short)
    refb = bytes(ref)
    batch = reads + [worse(reads[0], 2), pgs.synth.dna(912, 150).tobytes()]
    for sem in (0, 1):
        got = ctx.align_batch(batch, refb, semantics=sem)
        name = ctx.last_kernel()["name"]
        for k, (q, g) in enumerate(zip(batch, got)):
            _cmp(g, oracle.align(q, refb, sem), ("sampled maximum", sem, k))
        assert "every 4th step" in name, name
    for sc in ((5.0, -4.0, 3.0), (2.0, -1.0, 1.0)):
        got = ctx.align_batch(batch, refb, semantics=0, match=sc[0], mismatch=sc[1], gap=sc[2])
        for k, (q, g) in enumerate(zip(batch, got)):
            _cmp(g, oracle.align(q, refb, 0, *sc), ("sampled maximum", sc, k))


def test_sampled_maximum_falls_back_on_repeats(ctx, oracle, pgs):
    """Reads with equal maxima in thousands of sub-chunks (poly-A against a poly-A reference) exceed the candidate budget of
    the sampled sweep (64 per query + 1024): the call repeats the sweep with the exact per-step maximum, and the first maximum
    in the engine's storage order still wins."""
    n = 600_000
    refb = b"A" * n
    batch = [b"A" * 150, b"A" * 149 + b"C", b"C" + b"A" * 149, b"A" * 100 + b"G" + b"A" * 49, b"A" * 150, b"A" * 148 + b"TT"]
    for sem in (0, 1):
        got = ctx.align_batch(batch, refb, semantics=sem)
        name = ctx.last_kernel()["name"]
        for k, (q, g) in enumerate(zip(batch, got)):
            _cmp(g, oracle.align(q, refb, sem), ("repeats", sem, k))
        assert "every 4th step" not in name, name
