// sw_affine_kernel.h — affine-gap (Gotoh) Smith-Waterman for gfx950 (MI355X), hand-written HIP: score, end cell, traceback.
//
//   E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)        a gap of k columns (rows) costs o + (k - 1) e, o >= e > 0
//   F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)
//   H(i,j) = max(0, H(i-1,j-1) + s, E(i,j), F(i,j))  H = 0 on the borders; E, F = -inf there
//
// Three kernels:
//   * sw_affine_kernel<R, SL>: the anti-diagonal sweep, with the tile geometry of the two-query, one-strip instances of
//     sw_score_kernel (sw_score_kernel.h): tile = query pair x chunk + warm-up columns, SL lanes x R rows, the LDS query
//     profile read with ds_read_b128 at lane_stride, the code window refilled every 64 steps, per-sub-chunk maxima
//     published as (max << 32 | ~sub-chunk) keys.  Cells are packed float16 holding H / 2048 (Cell<kSemF16>), both queries
//     of a pair per register; per row the lane keeps H, E and Ho = H - o, and F runs down the lane's rows:
//         x     = v_pk_add_f16 clamp(NW, s)                     the [0, 1] clamp is the zero floor
//         E[r]  = pk_max(pk_add(E[r], -e), Ho[r])               Ho[r] still holds H(r, j-1) - o
//         H     = v_pk_maximum3_f16(x, E[r], F)
//         Ho[r] = pk_add(H, -o)
//         F     = pk_max(pk_add(F, -e), Ho[r])                  F of the row below
//     seven VOP3P ops per cell pair, and one maximum3 per two rows for the running maximum.  E and F never fall below -o
//     (each is a maximum with some H - o >= -o), so every value is an integer multiple of 1/2048 within +-2048/2048: exact.
//     Borders start at H = 0, E = F = -o, which gives the same cells as -inf.  Across lanes H and F each take one DPP
//     row_shr:1 per step; the tile's first lane gets 0 and -o.
//   * sw_affine_exact_kernel: float32 cells, one wavefront per (sub-)problem, three anti-diagonals of H and two each of E
//     and F in LDS (as sw_exact_kernel keeps H); tracks the first maximum in column-major order (order_key<0>) among the
//     window's own columns.  It finds the end cell inside the sub-chunk the sweep names, and computes whole problems that
//     are too small for the sweep (or all of them under option no_affine_sweep).
//   * sw_affine_trace_kernel: the same cells (affine_exact_fill) over the window behind an end cell (lemma L17), one decision
//     byte per cell, and the walk over them by the traceback rule of include/mi355_sw.h: pos and the reversed consensus strings.
// The anchored model of the extension calls (include/mi355_sw.h "anchored seed extension") is a third model of the same fill
// (affine_exact_fill_model): sw_affine_exact_ext_kernel and sw_affine_trace_ext_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_exact_kernel.h"
#include "sw_score_kernel.h"

namespace mi355sw {

// legal instances: 8- or 16-lane tiles
__host__ __device__ constexpr bool affine_instance_ok(int R, int SL) { return (SL == 8 || SL == 16) && R >= 1 && R <= 32; }

// a: as for sw_score_kernel (stab = float16 bits of s / 2048, [256][ncodes], pad column last; gap2, clamp2, pubmax, flag_*,
// submax_out, brow unused).  nopen2 / next2: float16 bits of -o / 2048 and -e / 2048 in both halves.
template <int R, int SL>
__global__ __launch_bounds__(256) void sw_affine_kernel(const ScoreArgs a, const uint32_t nopen2, const uint32_t next2) {
  static_assert(affine_instance_ok(R, SL), "no such sw_affine_kernel instance");
  typedef Cell<kSemF16> C;
  typedef uint32_t T;
  constexpr int LS = lane_stride(R);                               // dwords between the profile rows of adjacent lanes
  constexpr int NQ4 = (R + 3) / 4;
  constexpr int NSLOT = 256 / SL;                                  // tiles per workgroup
  constexpr int CPL = kSeg / SL;                                   // reference codes fetched per lane per segment (4 or 8)
  constexpr int PL = 16;                                           // lane positions of the profile
  constexpr int HIST = hist_bytes(SL);
  constexpr int CB = codebuf_bytes(SL);
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint32_t *prof = smem;                                           // [ncodes][PL lane positions][LS]
  uint8_t *codebuf = reinterpret_cast<uint8_t *>(smem + a.ncodes * PL * LS);

  const int tid = threadIdx.x;
  const int ls = tid & (SL - 1);                                   // lane within the tile
  const int slot = tid / SL;
  const int cgroups = (a.chunks_per_range + NSLOT - 1) / NSLOT;
  const int pair = blockIdx.x / cgroups;
  const int cg = blockIdx.x - pair * cgroups;
  const int range = blockIdx.y;
  const bool hasB = (2 * pair + 1) < a.qcount;
  const int qA = a.qsel[a.qfirst + 2 * pair];
  const int qB = hasB ? a.qsel[a.qfirst + 2 * pair + 1] : qA;
  const int mA = a.qlen[qA], mB = a.qlen[qB];

  // ---- query profile of this workgroup's pair: rows 0 .. SL*R - 1, padding rows score -8 (the clamp's floor) ------------
  {
    const uint8_t *xA = a.qbytes + a.qoff[qA];
    const uint8_t *xB = a.qbytes + a.qoff[qB];
    const int16_t *st = static_cast<const int16_t *>(a.stab);
    const int per_code = PL * R;
    for (int e = tid; e < a.ncodes * per_code; e += 256) {
      const int c = e / per_code;
      const int rem = e - c * per_code;
      const int ll = rem / R, r = rem - ll * R;
      const int i = (ll & (SL - 1)) * R + r;                       // (SL = 8: positions 8..15 repeat 0..7)
      const int sa = (i < mA) ? st[(int)xA[i] * a.ncodes + c] : C::kPad;
      const int sb = (i < mB) ? st[(int)xB[i] * a.ncodes + c] : C::kPad;
      prof[(c * PL + ll) * LS + r] = C::entry(sa, sb);
    }
  }

  // ---- this slot's tile ---------------------------------------------------------------------------------------------------
  const int64_t rlo = a.range_lo[range], rhi = a.range_hi[range];
  const int64_t nchunks = (rhi - rlo + a.chunk_len - 1) / a.chunk_len;
  const int64_t chunk = (int64_t)cg * NSLOT + slot;
  const bool active = chunk < nchunks;
  const int64_t own_lo = rlo + chunk * a.chunk_len;
  const int64_t own_hi = (own_lo + a.chunk_len < rhi) ? own_lo + a.chunk_len : rhi;
  const int64_t s0 = own_lo - a.warm;                              // reference index of stream position 0
  const uint32_t pad = (uint32_t)(a.ncodes - 1);
  const uint32_t pad4 = pad * 0x01010101u;

  // codes of stream positions seg*64 + CPL*ls .. +CPL-1 (pad outside [rlo, own_hi))
  struct Codes { uint32_t w[CPL / 4]; };
  auto stage_load = [&](int seg) -> Codes {
    Codes out;
    const int64_t c0 = s0 + (int64_t)seg * kSeg + CPL * ls;
#pragma unroll
    for (int d = 0; d < CPL / 4; ++d) {
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t col = c0 + 4 * d + b;
        const bool ok = active && col >= rlo && col < own_hi;
        const uint32_t code = ok ? (uint32_t)a.refcodes[col] : pad;
        w |= code << (8 * b);
      }
      out.w[d] = w;
    }
    return out;
  };
  uint8_t *buf = codebuf + slot * CB;
  uint32_t *buf32 = reinterpret_cast<uint32_t *>(buf);
  const uint8_t *buf_lane = buf + HIST - ls;                       // + k = code of step k
  const uint32_t *prof_lane = prof + (tid & (PL - 1)) * LS;
  auto window_put = [&](const Codes &c) {
#pragma unroll
    for (int d = 0; d < CPL / 4; ++d) buf32[HIST / 4 + (CPL / 4) * ls + d] = c.w[d];
  };

  const int64_t total_steps = a.warm + a.chunk_len + SL;           // + SL-1 skew, + 1 drain
  const int nseg = (int)((total_steps + kSeg - 1) / kSeg);
  const int code_stride = PL * LS;

  // border values of the tile's first lane: H(0, .) = 0 and F(1, .) = -o.  16 lanes: the DPP `old` operand; 8 lanes: lane 8 of
  // the DPP row starts another tile, one and-or per value
  uint32_t keep_mask = ls == 0 ? 0u : 0xFFFFFFFFu;
  uint32_t f_border = ls == 0 ? nopen2 : 0u;
  asm volatile("" : "+v"(keep_mask), "+v"(f_border));

  // per-sub-chunk maximum -> per-query key, as sw_score_kernel: lanes lag lane 0 by up to SL-1 columns, so up to SL-1 trailing
  // columns of a sub-chunk are reported with the next one; the host widens its search accordingly
  const int64_t subs_per_tile = a.chunk_len / a.sub_len;
  uint32_t best_a = 0u, best_b = 0u;                               // this tile's best published value per query
  T mx = 0u;
  auto publish = [&](int64_t sub) {
    uint32_t m32 = mx;
#pragma unroll
    for (int off = SL / 2; off >= 1; off >>= 1) m32 = C::vmax(m32, (uint32_t)__shfl_xor((int)m32, off, SL));
    // only a sub-chunk that strictly beats the tile's earlier ones can become the query's (max, first sub-chunk) key
    if (ls == 0 && active) {
      const unsigned long long tag = 0xFFFFFFFFull - (unsigned long long)(chunk * subs_per_tile + sub);
      unsigned long long *k = a.keys + (size_t)range * a.nq;
      const uint32_t va = m32 & 0xFFFFu, vb = m32 >> 16;           // (non-negative float16 values order like their bits)
      auto key_max = [&](unsigned long long *addr, unsigned long long v) {
        if (v > __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(addr, v);
      };
      if (va > best_a) { best_a = va; key_max(k + qA, ((unsigned long long)va << 32) | tag); }
      if (hasB && vb > best_b) { best_b = vb; key_max(k + qB, ((unsigned long long)vb << 32) | tag); }
    }
    mx = 0u;
  };
  const int segs_per_sub = (int)(a.sub_len / kSeg);
  const int warm_segs = (int)(a.warm / kSeg);
  int64_t sub = 0;

  Codes nextcodes = stage_load(0);
  if (ls < HIST / 4) buf32[ls] = pad4;                             // history in front of the first segment = padding
  window_put(nextcodes);
  nextcodes = stage_load(1);
  __syncthreads();                                                 // profile + first window ready

  T H[R], E[R], Ho[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { H[r] = 0u; E[r] = nopen2; Ho[r] = nopen2; }
  uint32_t up_prev = 0u;
  T fdown = nopen2;                                                // F of the row below this lane's last row, last step

  for (int seg = 0; seg < nseg; ++seg) {
#pragma unroll 2
    for (int k = 0; k < kSeg; ++k) {
      const uint32_t c = (uint32_t)buf_lane[k];
      const u32x4 *pp = static_cast<const u32x4 *>(__builtin_assume_aligned(prof_lane + c * code_stride, 16));
      uint32_t p[NQ4 * 4];
#pragma unroll
      for (int q = 0; q < NQ4; ++q) {
        const u32x4 v = pp[q];
        p[4 * q + 0] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
      }
      // last row of the lane above at this lane's column: H, and the F it hands down
      uint32_t up, f;
      if (SL == 16) {
        up = row_shr1(H[R - 1]);
        f = (uint32_t)__builtin_amdgcn_update_dpp((int)nopen2, (int)fdown, 0x111 /*row_shr:1*/, 0xf, 0xf, false);
      } else {
        up = row_shr1(H[R - 1]) & keep_mask;
        f = (row_shr1(fdown) & keep_mask) | f_border;
      }
      T diag = up_prev;                                            // H(i0-1, j-1)
      up_prev = up;
      T tpend = 0u;
      (void)tpend;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const T w = H[r];
        const T x = C::add(diag, p[r], 0u);
        E[r] = C::vmax(C::sub_gap(E[r], next2), Ho[r]);
        const T h = C::vmax3(x, E[r], f);
        if (r & 1) mx = C::vmax3(mx, tpend, h);
        else if (r + 1 < R) tpend = h;
        else mx = C::vmax(mx, h);
        diag = w;
        H[r] = h;
        Ho[r] = C::sub_gap(h, nopen2);
        f = C::vmax(C::sub_gap(f, next2), Ho[r]);
      }
      fdown = f;
    }
    // slide the code window: keep the last HIST bytes as history, append the prefetched segment
    {
      const uint32_t h = buf32[kSeg / 4 + (ls & 3)];
      if (ls < HIST / 4) buf32[ls] = h;
    }
    window_put(nextcodes);
    nextcodes = stage_load(seg + 2);
    // lane 0 has just finished a sub-chunk (and it is not the tile's last): report and restart the maximum
    const int done = seg + 1 - warm_segs;
    if (done > 0 && done % segs_per_sub == 0 && done / segs_per_sub < subs_per_tile) publish(sub++);
  }
  publish(sub);                                                    // the tile's last (or only) sub-chunk
}

struct AffineScoring {
  const float *lut;       // device 256x256 or null
  float match, mismatch, gap_open, gap_extend;
};

// Decision byte of one cell of sw_affine_trace_kernel (diagonal-major, as ExactProblem::dirs): where H came from, in the priority
// of the traceback rule (include/mi355_sw.h), and whether E / F continued a gap instead of opening one.
enum : int { kAffStop = 0, kAffDiag = 1, kAffE = 2, kAffF = 3, kAffEExt = 4, kAffFExt = 8 };

// One wavefront per problem (ExactProblem of sw_exact_kernel.h; hout, full_n and square_quirk unused).  The diagonals are
// indexed by the row: cell (i, jl) of diagonal d = i + jl sits at index i.  A wavefront executes its LDS operations in order,
// so no barrier is needed between diagonals.  TRACE: every cell also stores its decision byte to P.dirs and nothing competes
// for the maximum; the value of the corner cell (m, nw) comes back in `best` of every lane.
// E2E: the end-to-end model of include/mi355_sw.h — no floor, column 0 holds H = F = -(o + (i-1) e) and E = -inf (row 0 stays 0),
// only row m competes and the first column wins (own_lo as before); a decision byte never holds kAffStop.
// BAND (local model only): the banded model of include/mi355_sw.h in the window's LOCAL coordinates — only cells with
// blo <= jl - i <= bhi are part of the matrix.  An out-of-band cell is written as H = 0, E = F = -inf (the header's second statement of
// the model) wherever a later diagonal can read it: on diagonal d the in-band rows are ceil((d - bhi) / 2) .. floor((d - blo) / 2), the
// two later diagonals read at most one row beyond them on either side, and the three rotating buffers hold nothing older; so the loop
// runs over the in-band rows and one more on each side, work in proportion to the band.  Such a cell competes for nothing and gets no
// decision byte: the walk never reaches it (its E and F never equal a positive H).  The layout of dirs is the unbanded one.
// EXT (kAffineModelExt): the anchored model of include/mi355_sw.h — the end-to-end model with row 0 a gap as well: H(0,j) = E(0,j) =
// -(o + (j-1) e), F(0,j) = -inf, H(0,0) = 0.  Two winners: the first column-major maximum over all cells — the local model's key
// order; only a positive cell can beat cell (0,0) = 0, and the border cells are negative, so the cells of the loop are all that
// compete — and the maximum of row m with its smallest column (end, end_j; column 0 is the caller's to fold in).  TRACE: as E2E.
// EXT with BAND: the anchored model inside blo <= jl - i <= bhi, blo <= 0 <= bhi (include/mi355_sw.h).  An out-of-band cell is written as
// H = E = F = -inf, not 0: the model has no floor, so a 0 outside would win.  A border cell of row 0 or column 0 keeps its value only
// where it lies in the band, else it is -inf as well.  The loop is the banded one, so both folds see in-band cells only, all finite;
// a row m without an in-band cell leaves end = -inf (the host reports the pair as unreachable).  TRACE: an equality with -inf never
// holds, so the walk stays in the band; it meets row 0 or column 0 on an in-band cell, and the rest of that border towards (0,0) is.
// ROWS (EXT with BAND, score pass): the rows instance of the z-drop stop rule (include/mi355_sw.h "z-drop").  Beside
// the two winners it keeps, per row i = 1..m, the maximum of H(i, jl) over the in-band real columns 0 <= jl <= nw and its smallest
// column, in two more LDS arrays behind the letters of x: the border cell (i, 0) initialises them where it lies in the band (else -inf),
// and the one cell of row i on a diagonal replaces them where it is greater — a row meets its columns in rising order, so '>' keeps the
// smallest.  They are stored at the end: P.hout[i-1] = the maximum, P.hout[m + i-1] = the column's bits.  The host runs the rule.
// GLOB (kAffineModelGlob): the anchored model again — EXT's borders, EXT's cells, with or without BAND — whose answer is the corner:
// nothing competes, `best` is the value of cell (m, nw) (the lane that computes it; -inf in the others, and where the band misses the
// corner, which the host never sends).  It has no TRACE instance of its own: the traceback of a corner is EXT's walk from (m, nw).
struct AffineBest { float best; int64_t i, j; float end; int64_t end_j; };
enum : int { kAffineModelLocal = 0, kAffineModelE2E = 1, kAffineModelExt = 2, kAffineModelGlob = 3 };
template <bool TRACE, int MODEL, bool BAND, bool ROWS = false>
__device__ __forceinline__ AffineBest affine_exact_fill_model(const ExactProblem P, const AffineScoring sc, uint8_t *smem_raw, const int blo,
                                                              const int bhi) {
  constexpr bool GLOB = MODEL == kAffineModelGlob;                 // EXT's matrix, the corner for an answer
  static_assert(!(GLOB && TRACE), "the corner is traced by the anchored model's walk");
  constexpr bool EXT = MODEL == kAffineModelExt || GLOB;
  constexpr bool E2E = MODEL != kAffineModelLocal;                 // no floor and the column-0 border: every floor-free model
  static_assert(!(BAND && MODEL == kAffineModelE2E), "the banded end-to-end model is not defined");
  constexpr bool XB = EXT && BAND;                                 // the anchored model under a band: outside is -inf, borders only in the band
  static_assert(!ROWS || (MODEL == kAffineModelExt && BAND && !TRACE), "the rows instance is the banded anchored score pass");
  const int lane = threadIdx.x;
  const int m = P.m, nw = P.nw;
  const int plen = m + 2;
  float *Hb = reinterpret_cast<float *>(smem_raw);                 // 3 x H, 2 x E, 2 x F
  float *H0 = Hb, *H1 = Hb + plen, *H2 = Hb + 2 * plen;
  float *E0 = Hb + 3 * plen, *E1 = Hb + 4 * plen, *F0 = Hb + 5 * plen, *F1 = Hb + 6 * plen;
  uint8_t *xs = reinterpret_cast<uint8_t *>(Hb + 7 * plen);
  [[maybe_unused]] float *rmax = reinterpret_cast<float *>(xs + ((m + 3) & ~3));   // ROWS: [m + 1] the row's maximum ...
  [[maybe_unused]] int *rcol = reinterpret_cast<int *>(rmax + (m + 1));            // ... and [m + 1] its smallest column
  const float ninf = -__builtin_inff();
  for (int k = lane; k < 3 * plen; k += 64) Hb[k] = 0.0f;
  for (int k = lane; k < 4 * plen; k += 64) E0[k] = ninf;
  for (int k = lane; k < m; k += 64) xs[k] = P.x[k];
  if constexpr (ROWS)
    for (int i = 1 + lane; i <= m; i += 64) { rmax[i] = -i >= blo ? -(sc.gap_open + (float)(i - 1) * sc.gap_extend) : -__builtin_inff(); rcol[i] = 0; }
  if (E2E && lane == 0 && m >= 1) { H0[1] = -sc.gap_open; F0[1] = -sc.gap_open; }   // diagonal 1: cell (1, 0)
  if (EXT && lane == 0) { H0[0] = -sc.gap_open; E0[0] = -sc.gap_open; }             // and cell (0, 1)
  if (XB && lane == 0) {                                           // the two border cells of diagonal 1 where they miss the band
    if (m >= 1 && blo > -1) { H0[1] = ninf; F0[1] = ninf; }
    if (bhi < 1) { H0[0] = ninf; E0[0] = ninf; }
  }

  float best = (E2E && (TRACE || !EXT || GLOB)) ? ninf : -1.0f;    // (EXT, score pass: only a positive cell beats cell (0,0))
  float end = ninf;                                                // EXT: the greatest H(m, jl) and its first column
  int64_t end_j = 0;
  unsigned long long bkey = ~0ull;
  int64_t bi = 0, bj = 0;
  const float go = sc.gap_open, ge = sc.gap_extend;
  const int dstride = m < nw ? m : nw;

  float *Hc = H0, *Hp = H1, *Hpp = H2, *Ec = E0, *Ep = E1, *Fc = F0, *Fp = F1;
  // diagonals d = i + jl; d = 0 and 1 are all border (already initialised)
  for (int d = 2; d <= m + nw; ++d) {
    { float *t = Hpp; Hpp = Hp; Hp = Hc; Hc = t; }
    { float *t = Ep; Ep = Ec; Ec = t; }
    { float *t = Fp; Fp = Fc; Fc = t; }
    // border cells of this diagonal: row 0 (index 0) and column 0 (index d)
    if (lane == 0) {
      Hc[0] = 0.0f; Fc[0] = ninf; Ec[0] = ninf;
      if (EXT) { const float r0 = -(sc.gap_open + (float)(d - 1) * sc.gap_extend); Hc[0] = r0; Ec[0] = r0; }   // cell (0, d)
      if (d <= m) {
        const float b0 = E2E ? -(sc.gap_open + (float)(d - 1) * sc.gap_extend) : 0.0f;   // (integers below 2^24: exact)
        Hc[d] = b0; Ec[d] = ninf; Fc[d] = E2E ? b0 : ninf;
      }
      if (XB) {                                                    // cells (0, d) and (d, 0) outside the band
        if (d > bhi) { Hc[0] = ninf; Ec[0] = ninf; }
        if (d <= m && -d < blo) { Hc[d] = ninf; Fc[d] = ninf; }
      }
    }
    const int ilo = d - nw > 1 ? d - nw : 1;
    const int ihi = d - 1 < m ? d - 1 : m;
    int i0 = ilo, i1 = ihi;
    if (BAND) {                                                    // (floor division of possibly negative numbers: shifts)
      const int b0 = ((d - bhi + 1) >> 1) - 1, b1 = ((d - blo) >> 1) + 1;
      i0 = b0 > ilo ? b0 : ilo;
      i1 = b1 < ihi ? b1 : ihi;
    }
    for (int i = i0 + lane; i <= i1; i += 64) {
      const int jl = d - i;
      if (BAND && (jl - i < blo || jl - i > bhi)) { Hc[i] = XB ? ninf : 0.0f; Ec[i] = ninf; Fc[i] = ninf; continue; }
      const uint8_t xa = xs[i - 1], yb = P.y[jl - 1];
      const float s = sc.lut ? sc.lut[(int)xa * 256 + yb] : (xa == yb ? sc.match : sc.mismatch);
      const float eo = Hp[i] - go, fo = Hp[i - 1] - go;            // a gap opened from (i, jl-1) / (i-1, jl) on d-1
      const float e = fmaxf(Ep[i] - ge, eo);
      const float f = fmaxf(Fp[i - 1] - ge, fo);
      const float x = Hpp[i - 1] + s;
      const float h = E2E ? fmaxf(x, fmaxf(e, f)) : fmaxf(fmaxf(x, 0.0f), fmaxf(e, f));
      Hc[i] = h; Ec[i] = e; Fc[i] = f;
      // (row i is another lane's on the next diagonal, and the store loop behind reads it from yet another: one wavefront executes its
      // LDS operations in order, as for Hc / Hp above — no barrier)
      if constexpr (ROWS) { if (h > rmax[i]) { rmax[i] = h; rcol[i] = jl; } }
      if (TRACE) {
        const int src = (!E2E && h == 0.0f) ? kAffStop : h == x ? kAffDiag : h == e ? kAffE : kAffF;
        P.dirs[(size_t)d * (size_t)dstride + (size_t)(i - ilo)] = (uint8_t)(src | (e != eo ? kAffEExt : 0) | (f != fo ? kAffFExt : 0));
        if (d == m + nw) best = h;                                 // (one cell, one lane)
      } else if (GLOB) {
        if (d == m + nw) best = h;                                 // (one cell, one lane)
      } else if (EXT) {
        if (i == m && h > end) { end = h; end_j = jl; }            // (a lane meets its columns in rising order)
        if (h > 0.0f && h >= best) {
          const unsigned long long key = order_key<0>(i, jl, m, 0);
          if (h > best || key < bkey) { best = h; bkey = key; bi = i; bj = jl; }
        }
      } else if (E2E) {
        // row m, own columns; a lane meets its columns in rising order, so '>' keeps its first, and the key orders the lanes
        if (i == m && jl >= P.own_lo && h > best) { best = h; bkey = (unsigned long long)(P.col_offset + jl); bi = i; bj = P.col_offset + jl; }
      } else if (jl >= P.own_lo && h > 0.0f) {
        const bool cand = (P.target >= 0.0f) ? (h == P.target) : (h >= best);
        if (cand) {
          const int64_t jt = P.col_offset + jl;
          const unsigned long long key = order_key<0>(i, jt, m, 0);
          if (h > best || key < bkey) { best = h; bkey = key; bi = i; bj = jt; }
        }
      }
    }
  }
  // wave reduction: larger value first, then smaller key
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const unsigned long long ok = __shfl_xor(bkey, off);
    const long long oi = __shfl_xor((long long)bi, off);
    const long long oj = __shfl_xor((long long)bj, off);
    if (ob > best || (ob == best && ok < bkey)) { best = ob; bkey = ok; bi = oi; bj = oj; }
    if (EXT) {
      const float oe = __shfl_xor(end, off);
      const long long oej = __shfl_xor((long long)end_j, off);
      if (oe > end || (oe == end && oej < end_j)) { end = oe; end_j = oej; }
    }
  }
  if constexpr (ROWS)
    for (int i = 1 + lane; i <= m; i += 64) { P.hout[i - 1] = rmax[i]; P.hout[m + i - 1] = __int_as_float(rcol[i]); }
  return AffineBest{best, bi, bj, end, end_j};
}

// the fill by its two switches, as the local, end-to-end and banded instances name it
template <bool TRACE, bool E2E = false, bool BAND = false>
__device__ __forceinline__ AffineBest affine_exact_fill(const ExactProblem P, const AffineScoring sc, uint8_t *smem_raw, const int blo = 0,
                                                        const int bhi = 0) {
  return affine_exact_fill_model<TRACE, E2E ? kAffineModelE2E : kAffineModelLocal, BAND>(P, sc, smem_raw, blo, bhi);
}

// BAND: the problems carry their band (ExactBandProblem), in the window's local coordinates
struct ExactBandProblem { ExactProblem e; int32_t blo, bhi; };
template <bool BAND> struct AffineExactProblemOf { typedef ExactProblem type; };
template <> struct AffineExactProblemOf<true> { typedef ExactBandProblem type; };
__device__ __forceinline__ const ExactProblem &affine_problem(const ExactProblem &p) { return p; }
__device__ __forceinline__ const ExactProblem &affine_problem(const ExactBandProblem &p) { return p.e; }
__device__ __forceinline__ int affine_band_lo(const ExactProblem &) { return 0; }
__device__ __forceinline__ int affine_band_hi(const ExactProblem &) { return 0; }
__device__ __forceinline__ int affine_band_lo(const ExactBandProblem &p) { return p.blo; }
__device__ __forceinline__ int affine_band_hi(const ExactBandProblem &p) { return p.bhi; }

template <bool E2E = false, bool BAND = false>
__global__ __launch_bounds__(64) void sw_affine_exact_kernel(const typename AffineExactProblemOf<BAND>::type *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const ExactProblem P = affine_problem(probs[blockIdx.x]);
  const AffineBest r = affine_exact_fill<false, E2E, BAND>(P, sc, smem_raw, affine_band_lo(probs[blockIdx.x]), affine_band_hi(probs[blockIdx.x]));
  const float best = r.best;
  const int64_t bi = r.i, bj = r.j;
  if (threadIdx.x == 0) {
    if (P.best) *P.best = best;
    if (P.cell) { P.cell[0] = (E2E || best > 0.0f) ? bi : 0; P.cell[1] = (E2E || best > 0.0f) ? bj : 0; }
  }
}

// The anchored model (EXT of affine_exact_fill_model) on whole problems: P.best[0] / P.cell[0..1] = the best extension (0 / 0 / 0
// when no cell is positive), P.best[1] / P.cell[2..3] = the maximum of row m over columns 0..nw — H(m,0) = -(o + (m-1) e) folded in
// here, column 0 winning a tie — as (m, column).  own_lo, col_offset and target are unused.
__global__ __launch_bounds__(64) void sw_affine_exact_ext_kernel(const ExactProblem *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const ExactProblem P = probs[blockIdx.x];
  const AffineBest r = affine_exact_fill_model<false, kAffineModelExt, false>(P, sc, smem_raw, 0, 0);
  if (threadIdx.x == 0) {
    const bool pos = r.best > 0.0f;
    const float col0 = -(sc.gap_open + (float)(P.m - 1) * sc.gap_extend);
    const bool at0 = col0 >= r.end;
    P.best[0] = pos ? r.best : 0.0f;
    P.best[1] = at0 ? col0 : r.end;
    P.cell[0] = pos ? r.i : 0; P.cell[1] = pos ? r.j : 0;
    P.cell[2] = P.m; P.cell[3] = at0 ? 0 : r.end_j;
  }
}

// The same under a band (ExactBandProblem: blo <= 0 <= bhi, in the pair's own coordinates — the anchor is the window's corner).  Column
// 0 of row m competes only where it lies in the band; a row m that the band misses: P.best[1] = -inf, P.cell[3] = -1.
__global__ __launch_bounds__(64) void sw_affine_exact_ext_band_kernel(const ExactBandProblem *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const ExactProblem P = probs[blockIdx.x].e;
  const int blo = probs[blockIdx.x].blo, bhi = probs[blockIdx.x].bhi;
  const AffineBest r = affine_exact_fill_model<false, kAffineModelExt, true>(P, sc, smem_raw, blo, bhi);
  if (threadIdx.x == 0) {
    const bool pos = r.best > 0.0f;
    const float col0 = blo <= -P.m ? -(sc.gap_open + (float)(P.m - 1) * sc.gap_extend) : -__builtin_inff();
    const bool at0 = col0 >= r.end && blo <= -P.m;
    const float end = at0 ? col0 : r.end;
    P.best[0] = pos ? r.best : 0.0f;
    P.best[1] = end;
    P.cell[0] = pos ? r.i : 0; P.cell[1] = pos ? r.j : 0;
    P.cell[2] = P.m; P.cell[3] = at0 ? 0 : (end == -__builtin_inff() ? -1 : r.end_j);
  }
}

// The rows instance under a band (ROWS of affine_exact_fill_model): P.hout[0 .. 2 m) = the rows' maxima and, as bits, their smallest
// columns; P.best and P.cell are not written — the pair's results come from sw_affine_exact_ext_band_kernel on its first rows_done rows.
__global__ __launch_bounds__(64) void sw_affine_exact_rows_band_kernel(const ExactBandProblem *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const ExactProblem P = probs[blockIdx.x].e;
  (void)affine_exact_fill_model<false, kAffineModelExt, true, true>(P, sc, smem_raw, probs[blockIdx.x].blo, probs[blockIdx.x].bhi);
}

// The anchored model's corner (GLOB of affine_exact_fill_model) on whole problems of at least one row and one column, with or without a
// band that holds the corner: P.best[0] = H(m, nw), P.cell[0..1] = m, nw.  own_lo, col_offset and target are unused.
template <bool BAND>
__global__ __launch_bounds__(64) void sw_affine_exact_glob_kernel(const typename AffineExactProblemOf<BAND>::type *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const ExactProblem P = affine_problem(probs[blockIdx.x]);
  const AffineBest r = affine_exact_fill_model<false, kAffineModelGlob, BAND>(P, sc, smem_raw, affine_band_lo(probs[blockIdx.x]), affine_band_hi(probs[blockIdx.x]));
  if (threadIdx.x == 0) { P.best[0] = r.best; P.cell[0] = P.m; P.cell[1] = P.nw; }
}

// Traceback under affine gaps: the window [end_y - nw, end_y] x [end_x - m, end_x] of one alignment (lemmas L17 and L18, DESIGN.md
// §3.8: e.x is the first row of the window), so the end cell is the window's corner (e.m, e.nw).  e.target = the score, e.dirs = dirs_bytes(m, nw) bytes; e.best, e.cell,
// e.own_lo unused.
struct AffineTraceProblem {
  ExactProblem e;
  char *cons_x;           // capacity cap each: reversed, '-' for gaps, not terminated
  char *cons_y;
  int32_t cap;
  int32_t clamped;        // the window starts at the range's first column: its left border is the problem's own
  int32_t row_clamped;    // the window starts at the query's first row (e.x = x): its top border is the problem's own (lemma L18)
  // outputs: [0] consensus length, [1] pos (true column of the last letter pair), [2] status: 0 ok, 1 the walk left an
  // unclamped window (by its left or its top border), 2 capacity exceeded, 3 the corner cell does not hold the score
  int64_t *out;
};

// Fills the window as sw_affine_exact_kernel does (the same cells: affine_exact_fill), one decision byte per cell, then lane 0
// walks them from the corner by the rule of include/mi355_sw.h: state M follows bits 0-1, states E / F emit one gap letter and
// close the gap unless their extension bit is set (the opening wins a tie: the shortest gap).
// E2E: the walk ends in row 0 and nowhere else.  Local column 0 of a clamped window is the model's column 0: the rest of x is one run
// of F moves (x[i], '-') up to row 0; of an unclamped window it is status 1 as before (lemma L19).  There is no row window.
// BAND: the window's band in its local coordinates (AffineTraceBandProblem); the walk is the same one, it never reaches a cell
// outside the band (affine_exact_fill), and status 3 stays the guard of the window (L17 / L18 under a band: DESIGN.md §3.8).
struct AffineTraceBandProblem { AffineTraceProblem t; int32_t blo, bhi; };
template <bool BAND> struct AffineTraceProblemOf { typedef AffineTraceProblem type; };
template <> struct AffineTraceProblemOf<true> { typedef AffineTraceBandProblem type; };
__device__ __forceinline__ const AffineTraceProblem &affine_problem(const AffineTraceProblem &p) { return p; }
__device__ __forceinline__ const AffineTraceProblem &affine_problem(const AffineTraceBandProblem &p) { return p.t; }
__device__ __forceinline__ int affine_band_lo(const AffineTraceProblem &) { return 0; }
__device__ __forceinline__ int affine_band_hi(const AffineTraceProblem &) { return 0; }
__device__ __forceinline__ int affine_band_lo(const AffineTraceBandProblem &p) { return p.blo; }
__device__ __forceinline__ int affine_band_hi(const AffineTraceBandProblem &p) { return p.bhi; }

// EXT: the window is the whole rectangle from the anchor to the traced cell, so both clamps hold by construction.  The walk ends at
// (0,0) and nowhere else; in row 0 only E moves ('-', y[j]) happen, in column 0 only F moves (x[i], '-').
template <int MODEL, bool BAND, class Problem>
__device__ __forceinline__ void affine_trace_body(const Problem *probs, const AffineScoring sc, uint8_t *smem_raw) {
  constexpr bool EXT = MODEL == kAffineModelExt;
  constexpr bool E2E = MODEL == kAffineModelE2E;
  const AffineTraceProblem T = affine_problem(probs[blockIdx.x]);
  const ExactProblem &P = T.e;
  const float corner = affine_exact_fill_model<true, MODEL, BAND>(P, sc, smem_raw, affine_band_lo(probs[blockIdx.x]), affine_band_hi(probs[blockIdx.x])).best;
  // the walk reads what other lanes of this wavefront stored: wait for the stores, then keep the loads behind the barrier
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int m = P.m, nw = P.nw;
  const int dstride = m < nw ? m : nw;
  int i = m, jl = nw, len = 0, state = kAffDiag;                   // kAffDiag stands for state M
  int64_t status = corner == P.target ? 0 : 3, pos = 0;
  while (status == 0) {
    if (EXT) {
      if (i <= 0 && jl <= 0) break;
      if (i <= 0 || jl <= 0) {
        if (len >= T.cap) { status = 2; break; }
        if (i <= 0) { T.cons_x[len] = '-'; T.cons_y[len] = (char)P.y[jl - 1]; ++len; pos = P.col_offset + jl; --jl; }
        else { T.cons_x[len] = (char)P.x[i - 1]; T.cons_y[len] = '-'; ++len; --i; }
        continue;
      }
    } else if (E2E) {
      if (i <= 0) break;
      if (jl <= 0) {
        if (!T.clamped) { status = 1; break; }
        if (len >= T.cap) { status = 2; break; }
        T.cons_x[len] = (char)P.x[i - 1]; T.cons_y[len] = '-'; ++len;
        --i;
        continue;
      }
    } else if (i <= 0 || jl <= 0) {                                       // border: H = 0, stop
      if ((jl <= 0 && !T.clamped) || (i <= 0 && !T.row_clamped)) status = 1;
      break;
    }
    const int d = i + jl;
    const int ilo = d - nw > 1 ? d - nw : 1;
    const int dir = P.dirs[(size_t)d * (size_t)dstride + (size_t)(i - ilo)];
    if (state == kAffDiag) {
      const int src = dir & 3;
      if (src == kAffStop) break;
      if (src != kAffDiag) { state = src; continue; }
    }
    if (len >= T.cap) { status = 2; break; }
    if (state == kAffDiag) {
      T.cons_x[len] = (char)P.x[i - 1]; T.cons_y[len] = (char)P.y[jl - 1]; ++len;
      pos = P.col_offset + jl; --i; --jl;
    } else if (state == kAffE) {
      T.cons_x[len] = '-'; T.cons_y[len] = (char)P.y[jl - 1]; ++len;
      pos = P.col_offset + jl;
      if (!(dir & kAffEExt)) state = kAffDiag;
      --jl;
    } else {
      T.cons_x[len] = (char)P.x[i - 1]; T.cons_y[len] = '-'; ++len;
      if (!(dir & kAffFExt)) state = kAffDiag;
      --i;
    }
  }
  T.out[0] = len; T.out[1] = pos; T.out[2] = status;
}

template <bool E2E = false, bool BAND = false>
__global__ __launch_bounds__(64) void sw_affine_trace_kernel(const typename AffineTraceProblemOf<BAND>::type *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  affine_trace_body<E2E ? kAffineModelE2E : kAffineModelLocal, BAND>(probs, sc, smem_raw);
}

__global__ __launch_bounds__(64) void sw_affine_trace_ext_kernel(const AffineTraceProblem *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  affine_trace_body<kAffineModelExt, false>(probs, sc, smem_raw);
}

// under a band, in the pair's own coordinates: the rectangle runs from the anchor to the traced cell, so the band needs no shift
__global__ __launch_bounds__(64) void sw_affine_trace_ext_band_kernel(const AffineTraceBandProblem *probs, const AffineScoring sc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  affine_trace_body<kAffineModelExt, true>(probs, sc, smem_raw);
}

}  // namespace mi355sw
