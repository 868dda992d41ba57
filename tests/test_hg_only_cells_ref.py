"""Mirrored float16 cells that keep only K = H - g (sw_score_kernel kSemF16M, Cell::kDiagFromHg), emulated
on the CPU lane by lane.

One DPP row of 16 lanes is emulated as the kernel runs it: 8 lanes x 19 rows (two tiles side by side, so that lane 8 receives the K
of ANOTHER tile's last lane) and 16 lanes x 10 rows; lane l of a tile is at column t - l at step t, columns outside the reference
score as padding.  A register is a uint32 word (query A in the low half, query B in the high half); the adds are 32-bit integer
adds, `v_pk_minimum3_f16 ... clamp` is taken on float16 views of the halves.  Two forms are run on the same inputs:

  today's H form     a row keeps H (pattern N) and K = N + g;  x = N_nw + D;            border row N = 1.0;  ng = up + g
  the K-only form    a row keeps K alone;                       x = K_nw + (D - g2);     border row K = 1.0 + g;  ng = up

and must agree word for word in every cell (x, the cell and K), and the H recovered from either must be the oracle's matrix.
CPU only."""
import numpy as np
import pytest

ZERO2 = 0x3C003C00                 # float16 1.0 in both halves: H = 0
PAD_NEG = 1024                     # -s of padding rows and columns (the cap)
LANES = 16                         # one DPP row
COLS = 300
M32 = np.uint64(0xFFFFFFFF)


def halves(w):
    """(..., 2) float16 view of uint32 words: [..., 0] the low half."""
    return np.ascontiguousarray(w.astype(np.uint32)).view(np.uint16).reshape(w.shape + (2,)).view(np.float16)


def min3_clamp(a, b, c):
    """v_pk_minimum3_f16 a, b, c clamp on uint32 words (every operand a positive finite float16: only the upper end 1.0 acts)."""
    m = np.minimum(np.minimum(np.minimum(halves(a), halves(b)), halves(c)), np.float16(1.0))
    assert np.isfinite(m).all() and (m > 0).all()
    return np.ascontiguousarray(m).view(np.uint16).reshape(a.shape + (2,)).view(np.uint32).reshape(a.shape).astype(np.uint64)


def row_shr1(v):
    """v_mov_b32_dpp row_shr:1 bound_ctrl:0 over the 16 lanes (axis 1): lane 0 reads 0."""
    out = np.zeros_like(v)
    out[:, 1:] = v[:, :-1]
    return out


class Scoring:
    def __init__(self, name, gap, match=None, mismatch=None, lut=None):
        self.name, self.gap, self.match, self.mismatch, self.lut = name, gap, match, mismatch, lut

    def score(self, q, ref):
        """s(query byte, reference byte) as the score table holds it: (len(q), len(ref)) integers."""
        if self.lut is None:
            return np.where(q[:, None] == ref[None, :], self.match, self.mismatch).astype(np.int64)
        return self.lut[q[:, None], ref[None, :]].astype(np.int64)

    def smax(self):
        return max(self.match, self.mismatch, 0) if self.lut is None else int(max(0, self.lut.max()))

    def oracle_kw(self):
        if self.lut is None:
            return dict(match=float(self.match), mismatch=float(self.mismatch), gap=float(self.gap))
        return dict(gap=float(self.gap), lut=self.lut)


def table(kind):
    """A 256 x 256 table over ACGT: 4 on the diagonal, small negatives off it, and the entries the issue asks for."""
    lut = np.full((256, 256), -3.0, dtype=np.float32)
    for k, c in enumerate(b"ACGT"):
        lut[c, c] = 4.0 + (k % 2)
    if kind == "cap":
        lut[ord("A"), ord("C")] = -1024.0          # exactly at the cap of the profile entry
        lut[ord("G"), ord("T")] = -1100.0          # beyond it: capped
        lut[ord("T"), ord("G")] = -1023.0          # just inside
    else:
        lut[ord("A"), ord("G")] = 2.0              # positive off the diagonal: with reads that differ in the two halves one half
        lut[ord("C"), ord("T")] = 1.0              # subtracts (positive score) while the other adds, and the low half borrows
        lut[ord("G"), ord("A")] = -8.0
    return lut


SCORINGS = [
    Scoring("3/-3/2", 2, 3, -3),
    Scoring("1/-1/1", 1, 1, -1),
    Scoring("5/-4/7", 7, 5, -4),
    Scoring("table, entries at the -1024 cap", 3, lut=table("cap")),
    Scoring("table, opposite signs in the two halves", 2, lut=table("signs")),
]


def dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]


def read_of(rng, ref, at, n):
    """n bases of ref from `at` with a few substitutions and one deleted base: a hit with a gap in it."""
    q = ref[at:at + n + 1].copy()
    q = np.delete(q, n // 2)
    for p in rng.integers(0, n, max(1, n // 25)):
        q[p] = dna(rng, 1)[0]
    return q[:n]


def make_tiles(rng, SL, R):
    """Per scoring the tiles of one DPP row: [(qa, qb, ref)] * (16 / SL).  Pairs of unequal length: the padding rows sit in one half
    only (the high half of the first tile, the low half of the second), and end inside a lane."""
    rows = SL * R
    out = []
    for k, _ in enumerate(SCORINGS):
        tiles = []
        for t in range(LANES // SL):
            ref = dna(rng, COLS)
            long_q = read_of(rng, ref, 40 + 17 * t, rows)                      # fills every row of every lane
            short_q = read_of(rng, ref, 120, rows - R - 3 - 7 * k)            # ends inside the last lane but one
            tiles.append((long_q, short_q, ref) if t == 0 else (short_q, long_q, ref))
        out.append(tiles)
    return out


def sweep(SL, R, tiles_per_case, k_only):
    """All cases at once (axis 0), 16 lanes (axis 1), R rows (axis 2).  Returns x, cell and K words of every (case, lane, row, step)."""
    C = len(SCORINGS)
    steps = COLS + SL
    g2 = np.array([sc.gap * 0x00010001 for sc in SCORINGS], dtype=np.uint64)
    # profile words per (case, lane, row, step): the lane's column at step t is t - (lane % SL)
    W = np.empty((C, LANES, R, steps), dtype=np.uint64)
    for c, (sc, tiles) in enumerate(zip(SCORINGS, tiles_per_case)):
        for ti, (qa, qb, ref) in enumerate(tiles):
            negs = np.full((2, SL * R, COLS + 2 * LANES), PAD_NEG, dtype=np.int64)
            for h, q in enumerate((qa, qb)):
                negs[h, :len(q), LANES:LANES + COLS] = np.minimum(-sc.score(q, ref), PAD_NEG)
            d = ((negs[0] % (1 << 32)) + ((negs[1] % (1 << 32)) << 16)) % (1 << 32)       # today's entry: -s_A + (-s_B << 16)
            if k_only:
                d = (d - int(g2[c])) % (1 << 32)                                         # ONE 32-bit subtraction of gap2
            for ls in range(SL):
                W[c, ti * SL + ls] = d[ls * R:(ls + 1) * R, LANES - ls:LANES - ls + steps]
    first = (np.arange(LANES) % SL == 0)[None, :]
    gcol = g2[:, None]
    zero_k = np.uint64(ZERO2) + gcol                                                     # K of H = 0
    flz = np.where(first, zero_k if k_only else np.uint64(ZERO2), np.uint64(0))          # first_lane_z
    K = np.broadcast_to(zero_k[:, :, None], (C, LANES, R)).copy()
    H = np.full((C, LANES, R), ZERO2, dtype=np.uint64)
    up_prev = np.broadcast_to(zero_k if k_only else np.uint64(ZERO2), (C, LANES)).copy()
    xs = np.empty((C, LANES, R, steps), dtype=np.uint64)
    hs = np.empty_like(xs)
    ks = np.empty_like(xs)
    for t in range(steps):
        last = K[:, :, R - 1] if k_only else H[:, :, R - 1]
        assert (last <= (zero_k if k_only else np.uint64(ZERO2))).all()                  # what the one-op border relies on
        up = np.maximum(row_shr1(last), flz)                                            # v_max_u32_dpp
        assert (up[:, np.arange(LANES) % SL == 0] == (zero_k if k_only else np.uint64(ZERO2))).all()
        diag = up_prev
        up_prev = up
        ng = up if k_only else (up + gcol) & M32
        for r in range(R):
            w = (K[:, :, r] if k_only else H[:, :, r]).copy()                            # next row's diagonal
            x = (diag + W[:, :, r, t]) & M32                                             # v_add_u32
            h = min3_clamp(x, K[:, :, r], ng)
            k = h + gcol                                                                # v_add_u32
            assert (k <= M32).all() and ((k & np.uint64(0xFFFF)) == (h & np.uint64(0xFFFF)) + (gcol & np.uint64(0xFFFF))).all()
            assert (k <= zero_k).all()                                                  # K <= kZero + gap2 as a word
            xs[:, :, r, t], hs[:, :, r, t], ks[:, :, r, t] = x, h, k
            diag = w
            if not k_only:
                H[:, :, r] = h
            K[:, :, r] = k
            ng = k
    return xs, hs, ks


def recovered(words, half):
    """H = 2048 (1 - N) of one half of cell words."""
    return (1.0 - halves(words)[..., half].astype(np.float64)) * 2048.0


@pytest.mark.parametrize("SL,R", [(8, 19), (16, 10)])
def test_k_only_form_is_word_for_word_todays(oracle, SL, R):
    rng = np.random.default_rng(1000 * SL + R)
    tiles_per_case = make_tiles(rng, SL, R)
    for sc in SCORINGS:
        assert sc.smax() * (SL * R) + sc.smax() <= 1024, sc.name                        # mirror_ok
    xh, hh, kh = sweep(SL, R, tiles_per_case, k_only=False)
    xk, hk, kk = sweep(SL, R, tiles_per_case, k_only=True)
    for c, sc in enumerate(SCORINGS):
        for name, a, b in (("x", xh, xk), ("cell", hh, hk), ("K", kh, kk)):
            bad = np.argwhere(a[c] != b[c])
            assert bad.size == 0, "%s: %s differs first at (lane, row, step) %r: %#x vs %#x" % (
                sc.name, name, tuple(bad[0]), int(a[c][tuple(bad[0])]), int(b[c][tuple(bad[0])]))
    # H recovered from either form (the cell itself; K - gap2 of the K-only form) against the oracle's matrix
    g2 = np.array([sc.gap * 0x00010001 for sc in SCORINGS], dtype=np.uint64)[:, None, None, None]
    from_k = (kk - g2) & M32
    cap_seen = 0
    for c, (sc, tiles) in enumerate(zip(SCORINGS, tiles_per_case)):
        for ti, (qa, qb, ref) in enumerate(tiles):
            for half, q in enumerate((qa, qb)):
                exp = oracle.fill(q.tobytes(), ref.tobytes(), oracle.F32, **sc.oracle_kw())
                cap_seen += int((sc.score(q, ref) <= -1024).sum())
                for words, what in ((hh, "H form"), (from_k, "K-only form")):
                    got = np.zeros((len(q), COLS))
                    for ls in range(SL):
                        rows = range(ls * R, min((ls + 1) * R, len(q)))
                        for i in rows:
                            got[i] = recovered(words[c, ti * SL + ls, i - ls * R, ls:ls + COLS], half)
                    bad = np.argwhere(got != exp[1:, 1:])
                    assert bad.size == 0, "%s, %s, tile %d half %d: first mismatch at %r: %r vs %r" % (
                        sc.name, what, ti, half, tuple(bad[0]), got[tuple(bad[0])], exp[1:, 1:][tuple(bad[0])])
    assert cap_seen > 0                                                                 # the capped entries were met


def test_inputs_cover_the_issue():
    # unequal pairs: padding rows in one half only, in either half; both table scorings hold their special entries
    rng = np.random.default_rng(7)
    for SL, R in ((8, 19), (16, 10)):
        for tiles in make_tiles(rng, SL, R):
            assert len(tiles) == LANES // SL
            assert len(tiles[0][0]) == SL * R and len(tiles[0][1]) < SL * R - R
            if len(tiles) > 1:
                assert len(tiles[1][1]) == SL * R and len(tiles[1][0]) < SL * R - R
    assert (table("cap") == -1024.0).any() and (table("cap") < -1024.0).any()
    t = table("signs")
    assert (t[list(b"ACGT")][:, list(b"ACGT")] > 0).sum() > 4 and (t < 0).any()


if __name__ == "__main__":
    pytest.main([__file__, "-q"])
