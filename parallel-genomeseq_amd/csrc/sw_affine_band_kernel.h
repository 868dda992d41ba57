// sw_affine_band_kernel.h — affine-gap (Gotoh) score and end cell of a LIST OF PAIRS inside a DIAGONAL BAND per pair, hand-written
// HIP for gfx950.
//
// The banded sibling of sw_affine_pair_kernel (sw_affine_pair_kernel.h): pair k is a query x (m rows) against a
// window of y (n columns) restricted to the cells lo <= j - i <= hi (include/mi355_sw.h, "banded pairs").  Work must be proportional
// to rows x band width, so the geometry is the other one: the 16 lanes of a slot lie ACROSS the diagonals of the band and the ROWS
// are the time axis.  With lo_e the band's first diagonal inside the matrix and W its width (the host clips the band to the matrix),
// lane l, register r holds diagonal D = l R + r, i.e. delta = lo_e + D; step i computes the cells (i, i + delta) of row i:
//
//   diagonal   H(i-1,j-1) is the same register one row earlier: no move.  x = v_add_f32 clamp(Ho, s + o) = max(0, H(i-1,j-1) + s),
//              Ho = H - o and a table of s + o as in the pair kernel: the [0, 1] clamp is the zero floor
//   F          F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o) reads diagonal D + 1 of the previous row: the next register of the lane, or
//              register 0 of the next lane through one DPP row_shl:1 (two moves per step: Ho and F); the slot's last lane keeps
//              `old`, the value of a cell outside the band
//   E          runs along the row, a serial chain across all lanes.  It is broken up: first Ht = max(x, F) for every cell, then
//                  E(i,j) = max over the row's cells k < j of (Ht(i,k) - o - (j-1-k) e),          H = max(Ht, E)
//              — the scan runs over Ht and not over H, which is exact because o >= e: re-opening out of an E never beats extending
//              it.  A max-plus prefix scan with decay e: R serial sub / max pairs in the lane (q), then the lanes' totals through
//              four DPP steps row_shr:1/2/4/8 with decays R e, 2R e, 4R e, 8R e, and one row_shr:1 for the exclusive carry C;
//              E of register r is max(q[r-1], C - r e).  DPP rows are the 16-lane slots: no move crosses a slot.
//
// What lies outside.  A cell outside the band holds H = 0, E = F = -inf — here -o for E and F, which gives the same cells (L15 (d)):
// it contributes at most -o < 0 to a neighbour and never wins (the header's second statement of the model).  Three kinds:
//   * columns j < 1 and j > n (the band sticks out of the matrix in later or earlier rows) and rows beyond m (the slots of a
//     wavefront run to the longest query of the four): the `outside` code of y and the last class of x, kPadScoreF, as in the pair
//     kernel.  Left of column 1 and above row 1 nothing positive ever arrives, so those cells stay 0; right of column n and below row m
//     a cell holds max(0, E, F), strictly below a real cell, feeds only cells of its own kind (F runs down a column, the diagonal
//     stays on its diagonal, E runs to the right) and never leads the slot;
//   * registers D >= W of a band narrower than the instance's 16 R diagonals: real cells of the matrix to the right of the band.  E
//     flows into them and the diagonal term can score there, and their F would flow back into diagonal W - 1.  One v_min_f32 per cell
//     against cap[r] (1 in the band, 0 beyond) makes their H 0 — the model's value — before it is stored, folded or handed on;
//   * beyond the slot's last lane: the `old` operand of the two row_shl moves, Ho = F = -o.
//
// y reaches the cells through LDS: the slot stages the codes of columns lo_e + 1 .. lo_e + steps + 16 R once, and the class offsets
// of its rows of x; cell (i, D) reads entry i - 1 + D — per cell one ds_read_u8 at an immediate offset, one v_mad_u32_u24 (code *
// bytes of a table row + the row's class offset) and the ds_read_b32 of the table.  Static LDS: 16 x (512 + 16 R) + 16 KiB, at most
// 28 KiB, so that a 32 KiB table keeps the workgroup within 64 KiB.  The table is that kernel's: tab[code of y][class of x] = (s + o) 2^-k.
//
// Winner: the first maximum in column-major order.  The sweep is by ROWS, so "a later step only wins with a greater value" is wrong
// here: a later row can hold the same value in a smaller column.  Per step the lane's greatest key bits(H) | (31 - r) is the
// greatest value at its smallest column (columns rise with r); the lane replaces its best where the step's value is greater, or
// equal in a smaller column (equal in the same column: the earlier row stays).  Across lanes slot_first_max: value, then smaller
// column, then smaller row.  Exactness (float32 scaled by 2^-k, five mantissa bits free, decayed carries): DESIGN.md §3.8, L20.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_affine_pair_kernel.h"

namespace mi355sw {

// registers per lane of the compiled instances: a band of at most 16 R diagonals each.  A step costs all 16 R diagonals whatever W is, so
// the list is dense where a mapper's bands lie: half widths 8, 16, 32, 64 are 17, 33, 65, 129 diagonals, on R = 2, 3, 5, 9
constexpr int kBandR[] = {1, 2, 3, 5, 7, 9, 12, 16};
constexpr int kBandRowsMax = 512;                                  // rows of a pair: what a slot's windows in LDS hold

struct AffineBandProblem {
  const uint8_t *x;          // bytes of the query
  const uint8_t *y;          // CODES of the window of the reference
  int32_t m, n;              // rows (1..kBandRowsMax), columns (>= 1)
  int32_t lo, W;             // first diagonal j - i of the band inside the matrix, and its width (1..16 R)
};

template <int CTRL>
__device__ __forceinline__ float band_dpp(float old, float v) {
  return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp((int)__float_as_uint(old), (int)__float_as_uint(v), CTRL, 0xf, 0xf, false));
}

// sa: as for sw_affine_pair_kernel
template <int R>
__global__ __launch_bounds__(256) void sw_affine_band_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  static_assert(R >= 1 && R <= 32, "the key holds the register within the lane in five bits");
  constexpr int YW = kBandRowsMax + 16 * R;                        // entries of a slot's window of y: cell (i, D) reads i - 1 + D
  extern __shared__ __attribute__((aligned(16))) uint32_t bandsmem[];
  __shared__ uint8_t ywin[16 * YW];                                // codes of y
  __shared__ uint16_t xwin[16 * kBandRowsMax];                     // 4 * class of x[i]
  float *tab = reinterpret_cast<float *>(bandsmem);                // [nrows][ncls]
  const int tid = threadIdx.x;
  const int l = tid & 15;
  const int slot = tid >> 4;
  const int pid = blockIdx.x * 16 + slot;
  const bool active = pid < nprob;
  const uint8_t *xb = nullptr, *yc = nullptr;
  int m = 0, n = 0, lo = 0, W = 0;
  if (active) { xb = probs[pid].x; yc = probs[pid].y; m = probs[pid].m; n = probs[pid].n; lo = probs[pid].lo; W = probs[pid].W; }
  m = min(m, kBandRowsMax);                                        // (the host admits no more: the windows below hold no more)
  for (int e = tid; e < sa.nrows * sa.ncls; e += 256) tab[e] = sa.tab[e];
  // rows the wavefront runs: the longest query of its four slots
  int steps = m;
  steps = max(steps, __shfl_xor(steps, 16));
  steps = max(steps, __shfl_xor(steps, 32));
  const uint32_t row_bytes = 4u * (uint32_t)sa.ncls;
  const uint32_t outside = (uint32_t)(sa.nrows - 1);
  uint8_t *yw = ywin + slot * YW;
  uint16_t *xw = xwin + slot * kBandRowsMax;
  for (int p = l; p < steps + 16 * R; p += 16) {                   // entry p: column lo + 1 + p
    const long long j = (long long)lo + 1 + p;
    const uint32_t c = (j >= 1 && j <= (long long)n) ? (uint32_t)yc[j - 1] : outside;
    yw[p] = (uint8_t)c;
  }
  for (int i = l; i < steps; i += 16) xw[i] = (uint16_t)(4u * (i < m ? (uint32_t)sa.cls[xb[i]] : (uint32_t)(sa.ncls - 1)));
  __syncthreads();

  const float ov = sa.open_s, ev = sa.ext_s;
  const float nopen = -sa.open_s;                                  // outside the band: H = 0 is Ho = -o, and F = -o
  const float ninf = -__builtin_inff();                            // in front of the slot's first lane: no carry
  const float dec1 = (float)R * sa.ext_s, dec2 = 2.0f * dec1, dec4 = 4.0f * dec1, dec8 = 8.0f * dec1;
  float Ho[R], F[R], cap[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { Ho[r] = nopen; F[r] = nopen; cap[r] = (l * R + r < W) ? 1.0f : 0.0f; }
  float bval = 0.0f;                                               // the lane's best value, first seen at (brow, bcol)
  int brow = 0, bcol = 0x7fffffff;
  const char *tab_b = reinterpret_cast<const char *>(tab);
  const uint8_t *yl = yw + l * R;
  const int col0 = lo + l * R + 1;                                 // column of register 0 in row 0 (it = 0 is row 1: + it)

  for (int it = 0; it < steps; ++it) {
    const uint32_t xo = xw[it];
    const uint8_t *yp = yl + it;
    // diagonal D + 1 of the previous row for the lane's last register: register 0 of the next lane
    const float hnext = band_dpp<0x101>(nopen, Ho[0]);
    const float fnext = band_dpp<0x101>(nopen, F[0]);
    float Ht[R], q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float hon = r + 1 < R ? Ho[r + 1] : hnext;             // H(i-1, j) - o
      const float fpn = r + 1 < R ? F[r + 1] : fnext;              // F(i-1, j)
      const float s = *reinterpret_cast<const float *>(tab_b + (__umul24((uint32_t)yp[r], row_bytes) + xo));
      // plain C++ (an inline-asm definition costs a wait state in front of the VALU op that reads it on gfx950): the median with 0
      // and 1 folds into the add's clamp, the maxima of results of arithmetic need no canonicalisation
      const float x = __builtin_amdgcn_fmed3f(Ho[r] + s, 0.0f, 1.0f);
      const float f = fmaxf(fpn - ev, hon);
      const float ht = fmaxf(x, f);
      const float a = ht - ov;
      F[r] = f;
      Ht[r] = ht;
      q[r] = r == 0 ? a : fmaxf(q[r - 1] - ev, a);
    }
    // the lanes' totals: inclusive max-plus scan with decay R e per lane, then the exclusive carry
    float G = q[R - 1];
    G = fmaxf(G, band_dpp<0x111>(ninf, G) - dec1);
    G = fmaxf(G, band_dpp<0x112>(ninf, G) - dec2);
    G = fmaxf(G, band_dpp<0x114>(ninf, G) - dec4);
    G = fmaxf(G, band_dpp<0x118>(ninf, G) - dec8);
    float ce = band_dpp<0x111>(ninf, G);                           // E of register 0: everything left of the lane
    float mx = 0.0f, tpend = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float h = r == 0 ? fmaxf(Ht[0], ce) : fmaxf(fmaxf(Ht[r], q[r - 1]), ce);
      h = fminf(h, cap[r]);
      WaveKeyFold::cell<R>(r, h, mx, tpend);
      Ho[r] = h - ov;
      if (r + 1 < R) ce = ce - ev;
    }
    // the step's best against the lane's: greater value, or the same value in a smaller column (header: Winner)
    const uint32_t kb = __float_as_uint(mx);
    const float v = __uint_as_float(kb & ~31u);
    const int col = col0 + it + (31 - (int)(kb & 31u));
    const bool take = v > bval || (v == bval && col < bcol);
    bval = take ? v : bval;
    bcol = take ? col : bcol;
    brow = take ? it + 1 : brow;
  }

  float bv = bval * sa.unscale;
  long long bi = brow, bj = bcol;
  if (!(bv > 0.0f)) { bv = 0.0f; bi = 0; bj = 0; }
  slot_first_max(bv, bi, bj);
  if (l == 0 && active) {
    sa.best[pid] = bv;
    sa.cell[2 * (size_t)pid] = bv > 0.0f ? bi : 0;
    sa.cell[2 * (size_t)pid + 1] = bv > 0.0f ? bj : 0;
  }
}

// sw_affine_band_ext_kernel — the ANCHORED sibling (include/mi355_sw.h "anchored seed extension inside a diagonal band", DESIGN.md
// §3.8 lemma L22): the model of sw_affine_pair_ext_kernel restricted to the cells lo <= j - i <= hi, lo <= 0 <= hi, i and j counted
// from the anchor (0,0).  A sibling and not a flag, so that the local instances above stay the code they were; geometry, the two
// row_shl:1 moves for F, the max-plus scan for E, the windows of y and of x's classes in LDS and the (value, column) fold of the
// best are copies of the kernel above, which a change of the scaffold must visit as well.  What differs:
//   * no floor: the diagonal term is a plain add of Ho = H - o and the table's s + o;
//   * outside the band is -inf, not 0: the `old` operand of the two row_shl moves, the cap beyond diagonal W - 1 (one v_min_f32
//     against cap[r]: +inf in the band, -inf beyond) and the initial registers.  -inf only ever meets finite operands of add, sub,
//     min and max: no NaN arises, and F of a capped register stays -inf (both its sources are capped registers or `old`);
//   * row 0 is the initial state: Ho = H(0,delta) - o on the diagonals 0 <= delta <= hi_e (hi_e <= n: all real columns), H(0,0) = 0
//     and H(0,delta) = -(o + (delta-1) e); every other register and every F is -inf.  Column 0 has no code of its own: column j < 1
//     is an `outside` column like j > n, whose diagonal term is lost in kPadScoreF, the cells of columns j < 0 stay -inf (all three
//     sources are), so in column 0 E = -inf and H(i,0) = F(i,0) = max(F(i-1,0) - e, H(i-1,0) - o) = -(o + (i-1) e): the border;
//   * two results: the best extension is the fold above over max(H, 0) — cell (0,0) = 0 competes, a negative cell never wins, the
//     final "no positive cell: 0 / 0 / 0" stands; to the end is the unfloored maximum of row m over the real columns 0 <= j <= n at
//     the smallest column.  The slots of a wavefront have different m and the loop runs to the longest: row m is folded only at the
//     step where a slot of the wavefront stands on its row m, behind one compare of the step's row with the slot's m per step.  As
//     compiled that is an exec-mask branch (s_and_saveexec, s_cbranch_execz): the wavefront jumps over the fold unless one of its
//     slots stands on its row m, so it runs the fold at most four times; no second fold per cell.  A lane's columns rise with r, so
//     a strict '>' keeps its smallest column; the lanes' (value, column) meet after the loop.  A pair whose band misses row m (lo_e > n - m) yields -inf
//     here: the host fills in "unreachable".
// Padding (L22): a padding row (> m) or column (> n) has E and F only, each derived by opening or extending a gap from a real cell
// of the same row or column — strictly below it, and that cell lies in no later column — or from another padding cell; it wins
// neither fold (value first, and row m folds real columns at a step where the slot stands on a real row).  Padding never feeds a
// real cell: F runs down a column, E to the right, the diagonal stays on its diagonal.
// Exactness: every value of a real cell is an integer of magnitude below 2^24 and every positive H is below 2^18, the key's five
// mantissa bits free (host_affine.h: affine_band_ext_exact); a decayed carry of the scan below -2^24 is rounded, stays below every
// real value (rounding is monotone) and never wins a maximum.  The scale 2^-k moves no mantissa bit.
// best[2 pid] = the best extension, cell[4 pid ..] = end_x, end_y (lengths; 0 / 0 at score 0); best[2 pid + 1] = max over the in-band
// 0 <= j <= n of H(m, j), cell[4 pid + 2 ..] = m and the smallest such column.
template <int R>
__global__ __launch_bounds__(256) void sw_affine_band_ext_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  static_assert(R >= 1 && R <= 32, "the key holds the register within the lane in five bits");
  constexpr int YW = kBandRowsMax + 16 * R;
  extern __shared__ __attribute__((aligned(16))) uint32_t bandsmem[];
  __shared__ uint8_t ywin[16 * YW];
  __shared__ uint16_t xwin[16 * kBandRowsMax];
  float *tab = reinterpret_cast<float *>(bandsmem);
  const int tid = threadIdx.x;
  const int l = tid & 15;
  const int slot = tid >> 4;
  const int pid = blockIdx.x * 16 + slot;
  const bool active = pid < nprob;
  const uint8_t *xb = nullptr, *yc = nullptr;
  int m = 0, n = 0, lo = 0, W = 0;
  if (active) { xb = probs[pid].x; yc = probs[pid].y; m = probs[pid].m; n = probs[pid].n; lo = probs[pid].lo; W = probs[pid].W; }
  m = min(m, kBandRowsMax);
  for (int e = tid; e < sa.nrows * sa.ncls; e += 256) tab[e] = sa.tab[e];
  int steps = m;
  steps = max(steps, __shfl_xor(steps, 16));
  steps = max(steps, __shfl_xor(steps, 32));
  const uint32_t row_bytes = 4u * (uint32_t)sa.ncls;
  const uint32_t outside = (uint32_t)(sa.nrows - 1);
  uint8_t *yw = ywin + slot * YW;
  uint16_t *xw = xwin + slot * kBandRowsMax;
  for (int p = l; p < steps + 16 * R; p += 16) {                   // entry p: column lo + 1 + p; column 0 is `outside` too
    const long long j = (long long)lo + 1 + p;
    const uint32_t c = (j >= 1 && j <= (long long)n) ? (uint32_t)yc[j - 1] : outside;
    yw[p] = (uint8_t)c;
  }
  for (int i = l; i < steps; i += 16) xw[i] = (uint16_t)(4u * (i < m ? (uint32_t)sa.cls[xb[i]] : (uint32_t)(sa.ncls - 1)));
  __syncthreads();

  const float ov = sa.open_s, ev = sa.ext_s;
  const float ninf = -__builtin_inff(), pinf = __builtin_inff();   // outside the band, and the cap of a register inside it
  const float dec1 = (float)R * sa.ext_s, dec2 = 2.0f * dec1, dec4 = 4.0f * dec1, dec8 = 8.0f * dec1;
  float Ho[R], F[R], cap[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int D = l * R + r, delta = lo + D;                       // row 0: cell (0, delta), in the band for D < W (delta <= hi_e <= n)
    const float h0 = delta == 0 ? 0.0f : -(sa.open_s + (float)(delta - 1) * sa.ext_s);
    Ho[r] = (D < W && delta >= 0) ? h0 - sa.open_s : ninf;
    F[r] = ninf;
    cap[r] = D < W ? pinf : ninf;
    asm volatile("" : "+v"(cap[r]));                               // (a register, so that the cap stays one v_min_f32 and not a min and a select)
  }
  float bval = 0.0f;                                               // best extension: the lane's best value, first seen at (brow, bcol)
  int brow = 0, bcol = 0x7fffffff;
  float eval = ninf;                                               // to the end: the lane's greatest H(m, j) at its smallest column
  int ecol = 0x7fffffff;
  const char *tab_b = reinterpret_cast<const char *>(tab);
  const uint8_t *yl = yw + l * R;
  const int col0 = lo + l * R + 1;                                 // column of register 0 in row 0 (it = 0 is row 1: + it)

  for (int it = 0; it < steps; ++it) {
    const uint32_t xo = xw[it];
    const uint8_t *yp = yl + it;
    const float hnext = band_dpp<0x101>(ninf, Ho[0]);
    const float fnext = band_dpp<0x101>(ninf, F[0]);
    float Ht[R], q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float hon = r + 1 < R ? Ho[r + 1] : hnext;             // H(i-1, j) - o
      const float fpn = r + 1 < R ? F[r + 1] : fnext;              // F(i-1, j)
      const float s = *reinterpret_cast<const float *>(tab_b + (__umul24((uint32_t)yp[r], row_bytes) + xo));
      const float x = Ho[r] + s;                                   // no clamp: no floor
      const float f = fmaxf(fpn - ev, hon);
      const float ht = fmaxf(x, f);
      const float a = ht - ov;
      F[r] = f;
      Ht[r] = ht;
      q[r] = r == 0 ? a : fmaxf(q[r - 1] - ev, a);
    }
    float G = q[R - 1];
    G = fmaxf(G, band_dpp<0x111>(ninf, G) - dec1);
    G = fmaxf(G, band_dpp<0x112>(ninf, G) - dec2);
    G = fmaxf(G, band_dpp<0x114>(ninf, G) - dec4);
    G = fmaxf(G, band_dpp<0x118>(ninf, G) - dec8);
    float ce = band_dpp<0x111>(ninf, G);                           // E of register 0: everything left of the lane
    float mx = 0.0f, tpend = 0.0f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float h = r == 0 ? fmaxf(Ht[0], ce) : fmaxf(fmaxf(Ht[r], q[r - 1]), ce);
      h = fminf(h, cap[r]);
      WaveKeyFold::cell<R>(r, fmaxf(h, 0.0f), mx, tpend);          // the floor on the answer: cell (0,0) competes
      Ho[r] = h - ov;
      if (r + 1 < R) ce = ce - ev;
    }
    const uint32_t kb = __float_as_uint(mx);
    const float v = __uint_as_float(kb & ~31u);
    const int col = col0 + it + (31 - (int)(kb & 31u));
    const bool take = v > bval || (v == bval && col < bcol);
    bval = take ? v : bval;
    bcol = take ? col : bcol;
    brow = take ? it + 1 : brow;
    // to the end: only at the step where the slot stands on its row m (an idle slot: m = 0, which no step matches); the wavefront
    // skips the block unless one of its four slots does
    if (it + 1 == m) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = col0 + it + r;
        const float h = Ho[r] + ov;                                // H(m, j): exact, both are integers below 2^24 units
        const bool in = j >= 0 && j <= n && h > eval;              // (a capped register holds -inf and never passes)
        eval = in ? h : eval;
        ecol = in ? j : ecol;
      }
    }
  }

  float bv = bval * sa.unscale;
  long long bi = brow, bj = bcol;
  if (!(bv > 0.0f)) { bv = 0.0f; bi = 0; bj = 0; }
  slot_first_max(bv, bi, bj);
  // to the end: the lanes' (value, column) -> the slot's: value, then smaller column
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const float oe = __shfl_xor(eval, off, 16);
    const int oc = __shfl_xor(ecol, off, 16);
    if (oe > eval || (oe == eval && oc < ecol)) { eval = oe; ecol = oc; }
  }
  if (l == 0 && active) {
    sa.best[2 * (size_t)pid] = bv;
    sa.best[2 * (size_t)pid + 1] = eval * sa.unscale;
    sa.cell[4 * (size_t)pid] = bv > 0.0f ? bi : 0;
    sa.cell[4 * (size_t)pid + 1] = bv > 0.0f ? bj : 0;
    sa.cell[4 * (size_t)pid + 2] = m;
    sa.cell[4 * (size_t)pid + 3] = ecol == 0x7fffffff ? -1 : ecol;
  }
}

// sw_affine_band_glob_kernel — the sibling ANCHORED AT BOTH ENDS (include/mi355_sw.h "global alignment between two anchors", DESIGN.md
// §3.8 lemma L23): the banded anchored model of the kernel above, whose answer is the one cell H(m, n).  A sibling and not a flag;
// geometry, the two row_shl:1 moves for F, the max-plus scan for E, the windows in LDS, -inf outside the band, the cap, the initial
// row-0 registers are copies of the kernel above, which a change of the scaffold must visit as well.  What differs: less.
//   * nothing competes: no max(H, 0), no key, no per-step fold and no (bval, bcol, brow) state;
//   * the answer is READ, not folded: in row m the cell of column n lies on diagonal n - m, register D = n - m - lo.  At the step
//     it + 1 == m — the branch of the kernel above, which a wavefront skips unless one of its slots stands on its row m — the lane
//     that holds D takes Ho + o of that one register.  The host sends only pairs with lo <= n - m <= lo + W - 1 (the corner lies in
//     the band), so D is one of the 16 R registers and holds a finite value.  The four slots of a wavefront have different m and run
//     to the longest: a slot reads at its own step, once; steps behind row m write nothing.
// Padding and exactness: as the kernel above, without its key — every value of a real cell is an integer below 2^24 in magnitude
// (host_affine.h: affine_band_glob_exact), no mantissa bit is reserved.
// best[pid] = H(m, n), of any sign; cell[2 pid ..] = m, n.
template <int R>
__global__ __launch_bounds__(256) void sw_affine_band_glob_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  static_assert(R >= 1 && R <= 32, "instances of kBandR");
  constexpr int YW = kBandRowsMax + 16 * R;
  extern __shared__ __attribute__((aligned(16))) uint32_t bandsmem[];
  __shared__ uint8_t ywin[16 * YW];
  __shared__ uint16_t xwin[16 * kBandRowsMax];
  float *tab = reinterpret_cast<float *>(bandsmem);
  const int tid = threadIdx.x;
  const int l = tid & 15;
  const int slot = tid >> 4;
  const int pid = blockIdx.x * 16 + slot;
  const bool active = pid < nprob;
  const uint8_t *xb = nullptr, *yc = nullptr;
  int m = 0, n = 0, lo = 0, W = 0;
  if (active) { xb = probs[pid].x; yc = probs[pid].y; m = probs[pid].m; n = probs[pid].n; lo = probs[pid].lo; W = probs[pid].W; }
  m = min(m, kBandRowsMax);
  for (int e = tid; e < sa.nrows * sa.ncls; e += 256) tab[e] = sa.tab[e];
  int steps = m;
  steps = max(steps, __shfl_xor(steps, 16));
  steps = max(steps, __shfl_xor(steps, 32));
  const uint32_t row_bytes = 4u * (uint32_t)sa.ncls;
  const uint32_t outside = (uint32_t)(sa.nrows - 1);
  uint8_t *yw = ywin + slot * YW;
  uint16_t *xw = xwin + slot * kBandRowsMax;
  for (int p = l; p < steps + 16 * R; p += 16) {                   // entry p: column lo + 1 + p; column 0 is `outside` too
    const long long j = (long long)lo + 1 + p;
    const uint32_t c = (j >= 1 && j <= (long long)n) ? (uint32_t)yc[j - 1] : outside;
    yw[p] = (uint8_t)c;
  }
  for (int i = l; i < steps; i += 16) xw[i] = (uint16_t)(4u * (i < m ? (uint32_t)sa.cls[xb[i]] : (uint32_t)(sa.ncls - 1)));
  __syncthreads();

  const float ov = sa.open_s, ev = sa.ext_s;
  const float ninf = -__builtin_inff(), pinf = __builtin_inff();   // outside the band, and the cap of a register inside it
  const float dec1 = (float)R * sa.ext_s, dec2 = 2.0f * dec1, dec4 = 4.0f * dec1, dec8 = 8.0f * dec1;
  float Ho[R], F[R], cap[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int D = l * R + r, delta = lo + D;                       // row 0: cell (0, delta), in the band for D < W (delta <= hi_e <= n)
    const float h0 = delta == 0 ? 0.0f : -(sa.open_s + (float)(delta - 1) * sa.ext_s);
    Ho[r] = (D < W && delta >= 0) ? h0 - sa.open_s : ninf;
    F[r] = ninf;
    cap[r] = D < W ? pinf : ninf;
    asm volatile("" : "+v"(cap[r]));                               // (a register, so that the cap stays one v_min_f32 and not a min and a select)
  }
  float corner = ninf;                                             // H(m, n), in the lane that holds diagonal n - m
  const int dsel = n - m - lo - l * R;                             // that diagonal's register within this lane (0..R-1: this lane holds it)
  const char *tab_b = reinterpret_cast<const char *>(tab);
  const uint8_t *yl = yw + l * R;

  for (int it = 0; it < steps; ++it) {
    const uint32_t xo = xw[it];
    const uint8_t *yp = yl + it;
    const float hnext = band_dpp<0x101>(ninf, Ho[0]);
    const float fnext = band_dpp<0x101>(ninf, F[0]);
    float Ht[R], q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float hon = r + 1 < R ? Ho[r + 1] : hnext;             // H(i-1, j) - o
      const float fpn = r + 1 < R ? F[r + 1] : fnext;              // F(i-1, j)
      const float s = *reinterpret_cast<const float *>(tab_b + (__umul24((uint32_t)yp[r], row_bytes) + xo));
      const float x = Ho[r] + s;                                   // no clamp: no floor
      const float f = fmaxf(fpn - ev, hon);
      const float ht = fmaxf(x, f);
      const float a = ht - ov;
      F[r] = f;
      Ht[r] = ht;
      q[r] = r == 0 ? a : fmaxf(q[r - 1] - ev, a);
    }
    float G = q[R - 1];
    G = fmaxf(G, band_dpp<0x111>(ninf, G) - dec1);
    G = fmaxf(G, band_dpp<0x112>(ninf, G) - dec2);
    G = fmaxf(G, band_dpp<0x114>(ninf, G) - dec4);
    G = fmaxf(G, band_dpp<0x118>(ninf, G) - dec8);
    float ce = band_dpp<0x111>(ninf, G);                           // E of register 0: everything left of the lane
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float h = r == 0 ? fmaxf(Ht[0], ce) : fmaxf(fmaxf(Ht[r], q[r - 1]), ce);
      h = fminf(h, cap[r]);
      Ho[r] = h - ov;
      if (r + 1 < R) ce = ce - ev;
    }
    // the corner: only at the step where the slot stands on its row m (an idle slot: m = 0, which no step matches); the wavefront
    // skips the block unless one of its four slots does
    if (it + 1 == m) {
#pragma unroll
      for (int r = 0; r < R; ++r) corner = dsel == r ? Ho[r] + ov : corner;   // H(m, n): exact, both are integers below 2^24 units
    }
  }

  // the slot's result: the value of the lane that holds diagonal n - m
  const int wd = n - m - lo;
  const int wl = (active && wd >= 0 && wd < 16 * R) ? wd / R : 0;
  const float bv = __shfl(corner, wl, 16) * sa.unscale;
  if (l == 0 && active) {
    sa.best[pid] = bv;
    sa.cell[2 * (size_t)pid] = m;
    sa.cell[2 * (size_t)pid + 1] = n;
  }
}

}  // namespace mi355sw
