"""Mirrored float16 cells with the diagonal term as a 32-bit integer add (sw_score_kernel kSemF16M),
emulated on the CPU.

The profile entry of a register (query A in the low half, query B in the high half) is D = (-s_B) * 2^16 + (-s_A) mod 2^32,
with each -s capped at 1024 (padding and every score <= -1024 reach the zero floor from any cell anyway).  One step of a row:
    x = v_add_u32(D, N_nw)                              (32-bit integer add; a borrow of the low half is absorbed by -s_B * 2^16)
    N = v_pk_minimum3_f16(x, K_w, K_n) clamp            (minimum of both halves, clamped to [0, 1]: the zero floor)
    K = v_add_u32(N, g * 0x00010001)
Checked here: the halves of the add, the clamped minimum against the earlier clamped float16 add bit for bit, and the whole
recurrence against the oracle.  CPU only."""
import numpy as np
import pytest

from test_f16_mirror_cells import _cases, _dna, _halves, _pack

ZERO = 0x3C00                      # float16 1.0: H = 0
CELLS = np.arange(0x3800, 0x3C01, dtype=np.int64)   # every cell pattern: H = 1024 .. 0
PAD_ENTRY = 0xC800                 # the score table's padding entry: float16 -8 = -16384 / 2048
# scores of the exhaustive checks: the issue's [-8, 16], large mismatches, the cap and the padding entry's -16384
SCORES = list(range(-8, 17)) + [-20, -1023, -1024, -1025, -2048, -16384]


def neg_s(entry):
    """-s capped at 1024 from the float16 table entry s / 2048, as sw_score_kernel's build_profile decodes it."""
    s = (np.asarray(entry, dtype=np.uint16).view(np.float16).astype(np.float32) * np.float32(2048.0)).astype(np.int64)
    return np.minimum(-s, 1024)


def entry(s):
    return (np.asarray(s, dtype=np.float32) / np.float32(2048.0)).astype(np.float16).view(np.uint16)


def profile_word(sa, sb):
    """D for the scores sa (low half) and sb (high half), padding as -16384."""
    da = neg_s(PAD_ENTRY if sa == -16384 else entry(sa))
    db = neg_s(PAD_ENTRY if sb == -16384 else entry(sb))
    return np.uint32((int(da) + (int(db) << 16)) % (1 << 32))


def test_table_entries_decode_exactly():
    s = np.arange(-2048, 2049)
    assert (neg_s(entry(s)) == np.minimum(-s, 1024)).all()
    assert int(neg_s(np.uint16(PAD_ENTRY))) == 1024


def test_integer_add_halves_exhaustive():
    # every cell pattern in each half against every pair of scores; the high half's cells run in the other direction, so
    # that each pattern meets many others, and pairs with opposite signs exercise the borrow
    pa = CELLS
    pb = CELLS[::-1]
    n32 = (pa | (pb << 16)).astype(np.uint32)
    for sa in SCORES:
        for sb in SCORES:
            d = profile_word(sa, sb)
            x = (n32.astype(np.uint64) + np.uint64(d)) & np.uint64(0xFFFFFFFF)
            lo = (x & np.uint64(0xFFFF)).astype(np.int64)
            hi = (x >> np.uint64(16)).astype(np.int64)
            assert (lo == pa + min(-sa, 1024)).all(), (sa, sb)
            assert (hi == pb + min(-sb, 1024)).all(), (sa, sb)
            # every half stays a finite positive float16 (no infinity, no NaN): at most 1.0 + 1024 ulps = 2.0
            assert lo.max() <= 0x4000 and hi.max() <= 0x4000 and lo.min() >= 0x3800 - 16 and hi.min() >= 0x3800 - 16


def test_integer_add_halves_full_grid_opposite_signs():
    # the full 1025 x 1025 grid of cell pairs for a positive score in one half and a negative one in the other
    pa, pb = np.meshgrid(CELLS, CELLS, indexing="ij")
    n32 = (pa | (pb << 16)).astype(np.uint32).ravel()
    for sa, sb in ((16, -8), (-8, 16), (3, -16384), (-16384, 3)):
        x = (n32.astype(np.uint64) + np.uint64(profile_word(sa, sb))) & np.uint64(0xFFFFFFFF)
        assert ((x & np.uint64(0xFFFF)).astype(np.int64) == pa.ravel() + min(-sa, 1024)).all()
        assert ((x >> np.uint64(16)).astype(np.int64) == pb.ravel() + min(-sb, 1024)).all()


def test_clamped_minimum_equals_clamped_add():
    # min(x_int, K_w, K_n, 1.0) == min(clamp(N + (-s / 2048)), K_w, K_n) bit for bit, for every cell N, the scores above and
    # reachable gap terms K = N + g (above 1.0 where H < g)
    one = np.float16(1.0)
    kpat = np.unique(np.concatenate([np.arange(0x3800, 0x3C00 + 2041, 37), [0x3800, 0x3BFF, 0x3C00, 0x3C01, 0x3C00 + 2040]]))
    kw = kpat.astype(np.uint16).view(np.float16)[:, None, None]
    kn = kpat[::-1].astype(np.uint16).view(np.float16)[None, :, None]
    for s in SCORES:
        # the cells L14 admits for this score: H_nw + s <= 1024 (smax * maxlen + smax <= 1024), so x stays in the binade
        cells = CELLS[CELLS >= 0x3800 + max(s, 0)]
        n = cells.astype(np.uint16).view(np.float16)
        e = PAD_ENTRY if s == -16384 else int(entry(s))
        # today: float16 add of the sign-flipped entry (one rounding), clamped to [0, 1]
        addend = np.uint16(e ^ 0x8000).view(np.float16)
        x_f = np.clip((n.astype(np.float32) + np.float32(addend)).astype(np.float16), np.float16(0.0), one)
        old = np.minimum(np.minimum(x_f[None, None, :], kw), kn)
        # now: integer add on the pattern, the clamp on the minimum
        x_i = (cells + int(neg_s(np.uint16(e)))).astype(np.uint16).view(np.float16)
        new = np.minimum(np.minimum(np.minimum(x_i[None, None, :], kw), kn), one)
        assert (new.view(np.uint16) == old.view(np.uint16)).all(), s


def int_diag_sweep(qa, qb, ref, match, mismatch, gap, rows, pad_cols=0):
    """The mirrored recurrence with the integer diagonal term, op by op, both halves of a uint32 register at once.
    Returns H (pairs, 2, rows + 1, cols + 1) as float64 and the running minimum of N per half (pairs, 2)."""
    P = len(qa)
    cols = max(len(r) for r in ref) + pad_cols
    # -s per (pair, half, row, column) from the float16 table entries, padding -16384, capped at 1024
    negs = np.full((P, 2, rows, cols), 1024, dtype=np.int64)
    for k in range(P):
        for h, q in enumerate((qa[k], qb[k])):
            s = np.where(q[:, None] == ref[k][None, :], match[k], -mismatch[k])
            negs[k, h, :len(q), :len(ref[k])] = neg_s(entry(s))
    D = ((negs[:, 0] % (1 << 32)) + ((negs[:, 1] % (1 << 32)) << 16)) % (1 << 32)    # (pairs, rows, cols)
    g2 = (np.asarray(gap, dtype=np.uint64) * np.uint64(0x00010001))
    z2 = np.uint64(ZERO * 0x00010001)
    one = np.float16(1.0)
    Hc = np.full((rows, P), z2, dtype=np.uint64)
    Kc = Hc + g2[None, :]
    out = np.zeros((P, 2, rows + 1, cols + 1), dtype=np.float64)
    mn = np.full((P, 2), 1.0, dtype=np.float32)
    for j in range(cols):
        diag = np.full(P, z2, dtype=np.uint64)                # border row: H = 0
        ng = diag + g2
        Hn = np.empty_like(Hc)
        Kn = np.empty_like(Kc)
        for i in range(rows):
            x = (diag + D[:, i, j].astype(np.uint64)) & np.uint64(0xFFFFFFFF)                # v_add_u32
            xh = _halves(x.astype(np.uint32))
            assert np.isfinite(xh).all()
            n = np.minimum(np.minimum(np.minimum(xh, _halves(Kc[i].astype(np.uint32))), _halves(ng.astype(np.uint32))), one)
            nb = _pack(n).astype(np.uint64)
            k = nb + g2
            assert (k < (1 << 32)).all()
            diag = Hc[i]
            Hn[i] = nb
            Kn[i] = k
            ng = k
            mn = np.minimum(mn, n.astype(np.float32))
            out[:, :, i + 1, j + 1] = (1.0 - n.astype(np.float64)) * 2048.0
        Hc, Kc = Hn, Kn
    return out, mn


def _check(oracle, qa, qb, ref, match, mismatch, gap, rows, pad_cols=0):
    got, mn = int_diag_sweep(qa, qb, ref, match, mismatch, gap, rows, pad_cols)
    for k in range(len(qa)):
        for h, q in enumerate((qa[k], qb[k])):
            exp = oracle.fill(q.tobytes(), ref[k].tobytes(), oracle.F32, float(match[k]), -float(mismatch[k]), float(gap[k]))
            m, n = len(q), len(ref[k])
            sub = got[k, h, :m + 1, :n + 1]
            bad = np.argwhere(sub != exp)
            assert bad.size == 0, "pair %d half %d scoring (%r, %r, %r): first mismatch at %r: %r vs %r" % (
                k, h, match[k], mismatch[k], gap[k], bad[0], sub[tuple(bad[0])], exp[tuple(bad[0])])
            assert (1.0 - float(mn[k, h])) * 2048.0 == float(exp.max())
            assert 0.5 <= float(mn[k, h]) <= 1.0


def test_int_diag_matches_oracle_random_scorings(oracle):
    # random integer scorings (gaps above the match score, mismatches beyond the 1024 cap included), padding rows and columns
    rng = np.random.default_rng(20261017)
    scorings = [(int(rng.integers(1, 9)), int(rng.integers(0, 9)), int(rng.integers(1, 12))) for _ in range(10)]
    scorings += [(3, 3, 2), (1, 1, 1), (2, 1, 5), (4, 1100, 3), (1, 2000, 9)]
    qa, qb, ref, M, X, G = _cases(rng, scorings, 2, 10, 70, 110)
    rows = max(max(len(a) for a in qa), max(len(b) for b in qb)) + 3
    _check(oracle, qa, qb, ref, M, X, G, rows, pad_cols=4)


def test_int_diag_reaches_1024_exactly(oracle):
    # H = 1024 (N = 0.5, the bottom of the binade) and 1020 at 3 / -3 / 2 (340 bp), with a short unrelated read in the other half
    rng = np.random.default_rng(5)
    r1 = _dna(rng, 160)
    r2 = _dna(rng, 345)
    qa = [r1[10:138].copy(), r2[3:343].copy()]           # 128 x 8 = 1024; 340 x 3 = 1020
    qb = [_dna(rng, 100), _dna(rng, 60)]
    got, mn = int_diag_sweep(qa, qb, [r1, r2], np.array([8, 3]), np.array([8, 3]), np.array([3, 2]), 340)
    assert got[0, 0].max() == 1024.0 and float(mn[0, 0]) == 0.5
    assert got[1, 0].max() == 1020.0
    _check(oracle, qa, qb, [r1, r2], np.array([8, 3]), np.array([8, 3]), np.array([3, 2]), 340)


if __name__ == "__main__":
    pytest.main([__file__, "-q"])
