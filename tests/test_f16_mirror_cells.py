"""Mirrored float16 cells (sw_score_kernel kSemF16M, DESIGN.md §3.3 lemma L14), emulated on the CPU op by op.

A register holds two cells as float16 N = 1 - H / 2048.  One step of a row is
    x = v_pk_add_f16 clamp(N_nw, -s / 2048)      (float16 add of both halves, clamped to [0, 1])
    N = v_pk_minimum3_f16(x, K_w, K_n)           (minimum of both halves)
    K = v_add_u32(N, g * 0x00010001)             (32-bit integer add on the bit pattern of the whole register)
with the border row and column at N = 1.0 (H = 0) and padding rows / columns scoring +8 (the profile's -8 with its sign bit
flipped).  The emulation runs the register as a uint32, both halves at once, and compares 2048 (1 - N) with the oracle's
matrix cell by cell.  CPU only."""
import numpy as np
import pytest

ZERO = 0x3C00                      # float16 1.0: H = 0
PAD = np.float16(8.0)              # padding entry of the mirrored profile (float16 -8 with its sign bit flipped)
ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _halves(u32):
    return u32.view(np.uint16).reshape(-1, 2).view(np.float16)


def _pack(f16):
    return np.ascontiguousarray(f16.astype(np.float16)).view(np.uint16).reshape(-1, 2).copy().view(np.uint32).reshape(-1)


def mirror_sweep(qa, qb, ref, match, mismatch, gap, rows, pad_cols=0):
    """Sweep query pairs (qa[k], qb[k]) against ref[k] with the three mirrored ops; every pair has its own scoring (match M,
    mismatch -X, gap G, given as the magnitudes M, X, G).
    rows >= every query length (the rows beyond a query score as padding), pad_cols padding columns after the reference.
    Returns H (pairs, 2, rows + 1, cols + 1) as float64 and the running minimum of N per half (pairs, 2)."""
    P = len(qa)
    cols = max(len(r) for r in ref) + pad_cols
    # mirrored profile -s / 2048 per (pair, half, row, column), padding +8
    prof = np.full((P, 2, rows, cols), PAD, dtype=np.float16)
    for k in range(P):
        for h, q in enumerate((qa[k], qb[k])):
            s = np.where(q[:, None] == ref[k][None, :], match[k], -mismatch[k]).astype(np.float32)
            prof[k, h, :len(q), :len(ref[k])] = (-s / 2048.0).astype(np.float16)
    g2 = (np.asarray(gap, dtype=np.uint32) * np.uint32(0x00010001))
    z2 = np.uint32(ZERO * 0x00010001)
    Hc = np.full((rows, P), z2, dtype=np.uint32)          # N of the previous column
    Kc = Hc + g2[None, :]                                 # K = N + g of the previous column
    out = np.empty((P, 2, rows + 1, cols + 1), dtype=np.float64)
    out[:, :, 0, :] = 0.0
    out[:, :, :, 0] = 0.0
    mn = np.full((P, 2), 1.0, dtype=np.float32)
    for j in range(cols):
        diag = np.full(P, z2, dtype=np.uint32)                # border row: H = 0
        ng = np.full(P, z2, dtype=np.uint32) + g2
        Hn = np.empty_like(Hc)
        Kn = np.empty_like(Kc)
        for i in range(rows):
            a = _halves(diag).astype(np.float32)
            s = prof[:, :, i, j].astype(np.float32)
            x = np.clip((a + s).astype(np.float16), np.float16(0.0), np.float16(1.0))      # add (one rounding), clamp
            n = np.minimum(np.minimum(x, _halves(Kc[i])), _halves(ng))                    # minimum3
            nb = _pack(n)
            with np.errstate(over="raise"):
                k = (nb.astype(np.uint64) + g2.astype(np.uint64))
            assert (k < (1 << 32)).all()
            k = k.astype(np.uint32)
            # no carry crossed the halves: each half of K is its own half of N plus g
            lo = (k & 0xFFFF).astype(np.int64) - (nb & 0xFFFF).astype(np.int64)
            assert (lo == np.asarray(gap)).all()
            diag = Hc[i]
            Hn[i] = nb
            Kn[i] = k
            ng = k
            mn = np.minimum(mn, n.astype(np.float32))
            out[:, :, i + 1, j + 1] = (1.0 - n.astype(np.float64)) * 2048.0
        Hc, Kc = Hn, Kn
    return out, mn


def _dna(rng, n):
    return ALPHA[rng.integers(0, 4, n)]


def _check(oracle, qa, qb, ref, match, mismatch, gap, rows, pad_cols=0):
    got, mn = mirror_sweep(qa, qb, ref, match, mismatch, gap, rows, pad_cols)
    for k in range(len(qa)):
        for h, q in enumerate((qa[k], qb[k])):
            exp = oracle.fill(q.tobytes(), ref[k].tobytes(), oracle.F32, float(match[k]), -float(mismatch[k]), float(gap[k]))
            m, n = len(q), len(ref[k])
            sub = got[k, h, :m + 1, :n + 1]
            bad = np.argwhere(sub != exp)
            assert bad.size == 0, "pair %d half %d scoring (%r, %r, %r): first mismatch at %r: %r vs %r" % (
                k, h, match[k], mismatch[k], gap[k], bad[0], sub[tuple(bad[0])], exp[tuple(bad[0])])
            # padding rows / columns never beat the real cells: the running maximum (published as 1 - N) is the oracle's
            assert (1.0 - float(mn[k, h])) * 2048.0 == float(exp.max())
            # every value of the sweep stays in the single binade [0.5, 1]
            assert 0.5 <= float(mn[k, h]) <= 1.0


def _cases(rng, scorings, pairs_per, len_lo, len_hi, ncols, identical=False):
    qa, qb, ref, M, X, G = [], [], [], [], [], []
    for (mt, mm, gp) in scorings:
        for _ in range(pairs_per):
            r = _dna(rng, ncols)
            la, lb = (int(v) for v in rng.integers(len_lo, len_hi + 1, 2))
            la = min(la, (1024 - mt) // mt)
            lb = min(lb, (1024 - mt) // mt)
            if identical or rng.random() < 0.5:
                # reads taken from the reference with a few substitutions: high scores, long diagonals
                o = int(rng.integers(0, max(1, ncols - la)))
                a = r[o:o + la].copy()
                if not identical:
                    a[rng.integers(0, len(a), max(1, len(a) // 25))] = _dna(rng, max(1, len(a) // 25))
            else:
                a = _dna(rng, la)
            b = _dna(rng, lb) if rng.random() < 0.5 else r[:lb].copy()
            qa.append(a); qb.append(b); ref.append(r); M.append(mt); X.append(mm); G.append(gp)
    return qa, qb, ref, np.array(M), np.array(X), np.array(G)


def test_mirror_ops_match_oracle_named_scorings(oracle):
    rng = np.random.default_rng(20261016)
    scorings = [(3, 3, 2), (1, 1, 1), (5, 4, 3), (2, 3, 1), (7, 1, 7)]
    qa, qb, ref, M, X, G = _cases(rng, scorings, 6, 20, 90, 140)
    rows = max(max(len(a) for a in qa), max(len(b) for b in qb)) + 3      # padding rows below every query
    _check(oracle, qa, qb, ref, M, X, G, rows, pad_cols=5)


def test_mirror_ops_match_oracle_random_scorings(oracle):
    # random integer scorings, gaps larger than the match score included
    rng = np.random.default_rng(7)
    scorings = [(int(rng.integers(1, 9)), int(rng.integers(0, 9)), int(rng.integers(1, 12))) for _ in range(12)]
    scorings += [(2, 1, 5), (1, 2, 9), (4, 4, 11)]
    qa, qb, ref, M, X, G = _cases(rng, scorings, 2, 10, 70, 110)
    rows = max(max(len(a) for a in qa), max(len(b) for b in qb)) + 2
    _check(oracle, qa, qb, ref, M, X, G, rows, pad_cols=3)


def test_mirror_ops_reach_1024_exactly(oracle):
    # an all-match run to H = 1024 (N = 0.5, the bottom of the binade), and one to 1020 = smax * maxlen + smax - smax at 3 / -3 / 2
    rng = np.random.default_rng(3)
    r1 = _dna(rng, 160)
    r2 = _dna(rng, 345)
    qa = [r1[10:138].copy(), r2[3:343].copy()]           # 128 x 8 = 1024; 340 x 3 = 1020
    qb = [_dna(rng, 100), r2[0:339].copy()]
    got, mn = mirror_sweep(qa, qb, [r1, r2], np.array([8, 3]), np.array([8, 3]), np.array([3, 2]), 340)
    assert got[0, 0].max() == 1024.0 and float(mn[0, 0]) == 0.5
    assert got[1, 0].max() == 1020.0
    _check(oracle, qa, qb, [r1, r2], np.array([8, 3]), np.array([8, 3]), np.array([3, 2]), 340)


def test_mirror_bit_pattern_is_linear_in_the_binade():
    # the premise of the integer gap term: in [0.5, 1] the float16 pattern of 1 - H / 2048 is 0x3C00 - H
    h = np.arange(0, 1025)
    pat = (1.0 - h / 2048.0).astype(np.float16).view(np.uint16).astype(np.int64)
    assert (pat == ZERO - h).all()
    # and 1 - N is exact there (what publish converts back to H / 2048)
    n = pat.astype(np.uint16).view(np.float16)
    assert ((np.float16(1.0) - n).astype(np.float64) * 2048.0 == h).all()


if __name__ == "__main__":
    pytest.main([__file__, "-q"])
