// sw_affine_pair_kernel.h — affine-gap (Gotoh) score and end cell of a LIST OF PAIRS (query, window of the resident reference),
// hand-written HIP for gfx950.
//
// The fourth score kernel of the affine path (sw_affine_kernel.h): the extension stage of a seed-and-extend mapper,
// where read k meets its own candidate window and nothing else.  Slot geometry, stream window and the slot's winner:
// sw_wave_common.h — but the slots of a workgroup share neither sequence, and the orientation is the other one: lane l holds ROWS
// l R .. l R + R - 1 of the query x (1..512 rows), the COLUMNS of the window of y stream, so nothing is kept per column and the
// window may be long.  sw_affine_prof_kernel (sw_affine_prof_kernel.h) with the roles of E and F exchanged:
//
//   E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)     runs along the columns of y: one register per row
//   F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)     runs along the rows of x: down the lane's R rows within a step (Frun), handed to
//                                                the next lane by one DPP row_shr:1
//   H(i,j) = max(0, H(i-1,j-1) + s, E, F)
//
// Cells are float32 scaled by 2^-k (2^k above every value: the host admits integer scores with smax (rows + 1) < 2^18 and
// gap_open < 2^18: exact, five mantissa bits free).  Per row the lane keeps E[r] and Ho[r] = H - o; the table holds s + o:
//     x     = v_add_f32 clamp(Ho(i-1,j-1), s + o)         = max(0, H(i-1,j-1) + s): the [0, 1] clamp is the zero floor
//     E[r]  = max(E[r] - e, Ho[r])                        Ho[r] still holds H(i,j-1) - o
//     H     = max3(x, E[r], Frun)
//     Ho[r] = H - o
//     Frun  = max(Frun - e, Ho[r])                        F of the next row
// seven float32 ops per cell.  Borders: H = 0, i.e. Ho = -o, and E = F = -o (lemma L15 (d)); the slot's first lane takes both
// border values from the `old` operand of its two DPP moves.
//
// Substitution scores: there is no per-workgroup profile, since every slot has its own query and its own window.  One small table
// in LDS serves the workgroup: tab[code of y][class of x] = (s + o) 2^-k, classes as affine_prof_plan groups the bytes of x (5 x 5
// entries for DNA, 25 x 21 for a 20-letter table); the last row ("outside": steps in front of and beyond the window) and the last
// class (padding rows beyond the query) hold kPadScoreF.  A lane computes the byte offset of its R rows' classes once; per cell one
// v_add_u32 (the step's row pointer + that offset) and one ds_read_b32.  Equal addresses broadcast; a table of at most 32 entries
// lies in as many banks.
//
// Winner: the first maximum in column-major order.  Per lane one key bits(H) | (31 - row in the lane); within a step (one column) the
// greatest key is the greatest value at its smallest row.  ACROSS steps a later column replaces the lane's key only where its VALUE
// is greater — the compare is against the stored key with its five low bits set — so the smallest column stays, whatever its row
// (a plain '>' on keys would let an equal value at a smaller row of a later column in).  Across the 16 lanes slot_first_max: value,
// then smaller column, then smaller row.  Padding rows and outside positions hold max(0, neighbours - penalty), strictly below some
// real cell: they never lead the slot.
//
// A slot writes only best[pid] / cell[2 pid ..]; no slot communicates with another, no workgroup waits, no atomics.  A slot whose
// window ends early idles on `outside` codes until the longest window of its wavefront is done (wave_steps).
//
// The file holds the local kernel, described above, and behind it ONE BODY for the three other modes of the same geometry — end to
// end, anchored extension, global — whose entry points only name their mode (the comment in front of them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sw_wave_common.h"

namespace mi355sw {

// rows per lane of the compiled instances: 16 R rows each, 150 rows on R = 10
constexpr int kPairR[] = {2, 5, 10, 16, 24, 32};

struct AffinePairProblem {
  const uint8_t *x;          // bytes of the query
  const uint8_t *y;          // CODES of the window of the reference
  int32_t m, n;              // rows (1..16 R), columns (>= 1)
};

struct AffinePairArgs {
  const float *tab;          // [nrows][ncls]: (s + o) * 2^-k; last row and last class: kPadScoreF
  const uint8_t *cls;        // [256] byte of x -> class
  int32_t nrows, ncls;       // letters of the reference + 1, classes of x's bytes + 1
  float open_s, ext_s;       // o and e * 2^-k
  float unscale;             // 2^k
  float zdrop_s;             // sw_affine_band_extz_kernel only: floor(zdrop) * 2^-k, below 2^24 units; in what was padding
  float *best;               // [nprob] maximum (0 when no positive cell)
  int64_t *cell;             // [nprob][2] = row (into x), column (into the window), 1-based, of the first maximum
  unsigned long long *zrows; // sw_affine_band_extz_kernel only: the word its wavefronts add the rows of their loops to (null for every other kernel)
};

template <int R>
__global__ __launch_bounds__(256) void sw_affine_pair_kernel(const AffinePairProblem *probs, int nprob, const AffinePairArgs sa) {
  static_assert(R >= 1 && R <= 32, "the key holds the row within the lane in five bits");
  extern __shared__ __attribute__((aligned(16))) uint32_t pairsmem[];
  __shared__ __attribute__((aligned(16))) uint8_t win[16 * kWaveBuf];
  float *tab = reinterpret_cast<float *>(pairsmem);                // [nrows][ncls]
  const int tid = threadIdx.x;
  const int l = tid & 15;
  const int slot = tid >> 4;
  const int pid = blockIdx.x * 16 + slot;
  const bool active = pid < nprob;
  const uint8_t *xb = nullptr, *yc = nullptr;
  int m = 0, n = 0;
  if (active) { xb = probs[pid].x; yc = probs[pid].y; m = probs[pid].m; n = probs[pid].n; }
  for (int e = tid; e < sa.nrows * sa.ncls; e += 256) tab[e] = sa.tab[e];
  // byte offset of each row's class within a table row (padding rows: the last class)
  uint32_t boff[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = l * R + r;
    boff[r] = 4u * (i < m ? (uint32_t)sa.cls[xb[i]] : (uint32_t)(sa.ncls - 1));
  }
  __syncthreads();

  // stream window of CODES (in front of the first column and beyond the last: `outside`)
  const uint32_t outside = (uint32_t)(sa.nrows - 1);
  auto stage_load = [&](int seg) -> uint32_t {
    return wave_stage_word(yc, n, seg * kWaveSeg + 4 * l, [&](bool in, uint32_t byte) { return in ? byte : outside; });
  };
  int nseg, steps4;
  wave_steps(n, 16, nseg, steps4);
  uint8_t *buf = win + slot * kWaveBuf;
  uint32_t *buf32 = reinterpret_cast<uint32_t *>(buf);
  const uint8_t *buf_lane = buf + 16 - l;
  uint32_t nextc = stage_load(0);
  if (l < 4) buf32[l] = outside * 0x01010101u;                     // history in front of the first column
  buf32[4 + l] = nextc;
  nextc = stage_load(1);

  float ov = sa.open_s, ev = sa.ext_s;
  asm volatile("" : "+v"(ov), "+v"(ev));                           // (VGPR operands: v_sub_f32 then issues at the double rate)
  const int nopen = (int)__float_as_uint(-sa.open_s);              // both border values: H = 0 is Ho = -o, and F = -o
  float E[R], Ho[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { E[r] = -ov; Ho[r] = -ov; }
  float up_prev = -ov;                                             // Ho of the previous lane's last row, one column to the left
  float fout = -ov;                                                // F this lane hands to the next one
  float blk = 0.0f, blk31 = __uint_as_float(31u);                  // the lane's best key, and the same with its row bits set
  int tl = 0;                                                      // the column (0-based) blk was first seen at
  const uint32_t row_bytes = 4u * (uint32_t)sa.ncls;
  const char *tab_b = reinterpret_cast<const char *>(tab);

  for (int seg = 0; seg < nseg; ++seg) {
    const int kq = min(kWaveSeg, steps4 - seg * kWaveSeg) >> 2;
    for (int k4 = 0; k4 < kq; ++k4) {
#pragma unroll
      for (int ku = 0; ku < 4; ++ku) {
        const int k = 4 * k4 + ku;
        const int t = seg * kWaveSeg + k - l;                      // this lane's column of the window (0-based)
        const uint32_t c = (uint32_t)buf_lane[k];
        const char *rowp = tab_b + c * row_bytes;
        // the previous lane's last row in this column: Ho and the F it hands on; the slot's first lane keeps `old`, the border
        const float up = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(nopen, (int)__float_as_uint(Ho[R - 1]), 0x111, 0xf, 0xf, false));
        float frun = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(nopen, (int)__float_as_uint(fout), 0x111, 0xf, 0xf, false));
        float diag = up_prev;                                      // H(i-1, j-1) - o
        up_prev = up;
        float mx = 0.0f, tpend = 0.0f;
        (void)tpend;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float w = Ho[r];                                   // H(i, j-1) - o
          const float s = *reinterpret_cast<const float *>(rowp + boff[r]);
          float x, g, h, ho, fs;
          asm("v_add_f32_e64 %0, %1, %2 clamp" : "=v"(x) : "v"(diag), "v"(s));
          asm("v_sub_f32 %0, %1, %2" : "=v"(g) : "v"(E[r]), "v"(ev));
          asm("v_max_f32 %0, %1, %2" : "=v"(g) : "v"(g), "v"(w));
          asm("v_max3_f32 %0, %1, %2, %3" : "=v"(h) : "v"(x), "v"(g), "v"(frun));
          WaveKeyFold::cell<R>(r, h, mx, tpend);
          asm("v_sub_f32 %0, %1, %2" : "=v"(ho) : "v"(h), "v"(ov));
          asm("v_sub_f32 %0, %1, %2" : "=v"(fs) : "v"(frun), "v"(ev));
          asm("v_max_f32 %0, %1, %2" : "=v"(frun) : "v"(fs), "v"(ho));
          E[r] = g;
          Ho[r] = ho;
          diag = w;
        }
        fout = frun;
        // a later column wins only with a greater VALUE (header: Winner)
        const bool take = mx > blk31;
        tl = take ? t : tl;
        blk = take ? mx : blk;
        blk31 = __uint_as_float(__float_as_uint(blk) | 31u);
      }
    }
    const uint32_t hist = buf32[kWaveSeg / 4 + (l & 3)];
    if (l < 4) buf32[l] = hist;
    buf32[4 + l] = nextc;
    nextc = stage_load(seg + 2);
  }

  // the lane's winner: value, row of x, column of the window (1-based), then the slot's
  const uint32_t kb = __float_as_uint(blk);
  float bv = __uint_as_float(kb & ~31u) * sa.unscale;
  long long bi = (long long)l * R + (31 - (int)(kb & 31u)) + 1;
  long long bj = (long long)tl + 1;
  if (!(bv > 0.0f)) { bv = 0.0f; bi = 0; bj = 0; }
  slot_first_max(bv, bi, bj);
  if (l == 0 && active) {
    sa.best[pid] = bv;
    sa.cell[2 * (size_t)pid] = bv > 0.0f ? bi : 0;
    sa.cell[2 * (size_t)pid + 1] = bv > 0.0f ? bj : 0;
  }
}

// ---- The non-local modes: ONE BODY (sw_affine_pair_body.inc), a mode is a set of traits, an entry point only names its mode ----
// End to end, anchored extension and global alignment share slots, stream window, table, the per-cell chain and the row loop of the
// kernel above; what a mode adds is written once, under the trait that asks for it.  Every one of them has no zero floor — the
// diagonal term is a plain v_add_f32, scores may be negative — and the column-0 border:
//   column 0   H(i,0) = F(i,0) = -(o + (i-1) e), E(i,0) = -inf.  Lane l stands on column 0 at its step with t == -1 (step l - 1;
//              lane 0: in front of the loop).  There its rows take Ho[r] = E[r] = H(i,0) - o: E(i,1) = max(E[r] - e, Ho[r]) = H(i,0) - o,
//              the value -inf gives.  What the lane computed on `outside` codes before that step is overwritten.  At the same step the
//              lane's DPP move reads the previous lane's Ho[R - 1] as that lane left it at ITS border step, one step earlier:
//              Ho(i0 - 1, 0), which becomes up_prev; one step later it reads Ho(i0 - 1, 1) and the real F(i0, 1).  The chain needs no
//              further change.  The selects live in a prologue of the first 16 steps (every border step is one of steps 0..14); the
//              steady-state loop has none of them.  Every fold restarts at the border step: nothing computed left of column 1
//              competes.  The step's R table values are all requested in front of the row loop (sv[]): left to itself the scheduler
//              issued each ds_read_b32 next to its use and waited for it (lgkmcnt(0) after nearly every load at R >= 16: twice the
//              local instance's time at R = 32).
// The traits:
//   kRow0      the row-0 border H(0,j) = E(0,j) = -(o + (j-1) e), F(0,j) = -inf.  The slot's first lane takes Ho(0,j) = H(0,j) - o and
//              F(1,j) = H(0,j) - o — the same number, -(2 o + (j-1) e) — from the `old` operand of its two DPP moves: `rowo`, -2 o at
//              step 0 (lane 0 stands on column 1 there) and e lower every step: one subtract per step, not per cell.  Cell (1,1) takes
//              its diagonal from up_prev = -o: H(0,0) = 0.  Beyond the window the value stays at that of column n (`rowmin`, one max
//              per step), so that no register leaves the admitted range while the slot idles behind a longer window of its wavefront.
//              Off: row 0 is free, `old` = -o (H(0,j) = 0, F(1,j) = -o), as in the kernel above.
//   kKey       the best over all cells: the kernel's key fold (WaveKeyFold: value bits | 31 - row, a later column only with a greater
//              VALUE, then slot_first_max) over max(H, 0) — one more max per cell, the floor on the answer, since H has none.
//   kRowM      the strict row-m fold: only row m competes — lane (m-1)/R, row (m-1)%R: one select per cell (`hm`) under masks fixed
//              before the loop — and only a strictly greater value replaces the lane's best, so the smallest column stays.  At the
//              end the slot takes value and column from that one lane.
//   kCorner    the corner capture: the row-m select again, and the step's value replaces the lane's result at the one step with
//              t == n - 1, the lane's column n — one integer compare and one select per step.  The four slots of a wavefront have
//              different n and run to the longest: the compare is with the slot's own n, so a slot takes its value once, at its own
//              step, and no padding step behind column n can overwrite it (t only rises; it equals n - 1 once).  "The last value
//              seen" would be wrong for every slot but the longest.
//   kOuts      results (best, cell) a problem writes: one per fold or capture.
// The modes:
// AffinePairE2E — sw_affine_pair_e2e_kernel, END TO END (include/mi355_sw.h "end-to-end mode", DESIGN.md §3.8 lemma L19): every row of
//   x is aligned, the window's flanks are free, the score may be negative: the row-m fold and nothing else; no key, no WaveKeyFold.
//   Columns beyond n and rows beyond m keep the `outside` code and the last class.  A padding row never feeds a real one (F and the
//   diagonal run downwards).  A padding column has E and F only: H(m, j > n) <= max over j <= n of H(m, j), with equality only for
//   the all-F path from the free row 0, and the strict compare keeps the real column (L19 (c)).  kPadScoreF enters one sum per cell,
//   whose other operand is an Ho = max(.., E, F) - o, and E and F never hold such a sum alone: every register stays finite (L19 (d)).
//   Exactness: nothing is floored and no mantissa bit is reserved; the host admits integer scores whose every value is below 2^24
//   in magnitude (host_affine.h: affine_e2e_exact); the scale 2^-k moves no mantissa bit.
//   best[pid] = max over j of H(m, j), of any sign; cell[2 pid ..] = m and the smallest such column (1-based).
// AffinePairExt — sw_affine_pair_ext_kernel, ANCHORED (include/mi355_sw.h "anchored seed extension", lemma L21): the alignment starts
//   at cell (0,0), in front of x[1] and y[1], both flanks are gaps, and it ends where the score peaks (the best extension, over all
//   cells: kKey) or in row m (to the end: kRowM), under the row-0 border.  Cell (0,0) = 0 always competes and every border cell is
//   negative, so the winner of the key fold is a positive cell or 0 / 0 / 0, and a negative cell never wins.  To the end: after the
//   slot's result H(m,0) = -(o + (m-1) e) is folded in, and column 0 wins a tie.  Padding (L21 (c), restating L19 (c) / (d) for the
//   row-0 border): a padding row (> m) or column (> n) has E and F only, since kPadScoreF enters its diagonal term.  Its E and F
//   derive, by opening or extending a gap, from a real cell in the same row or column — strictly below that cell, which lies in no
//   later column — or from a border cell, which is negative; inductively every padding cell is negative or strictly below a real
//   cell of no later column: it wins neither fold (max(H, 0) and the value-only compare; the strict compare of row m, where the
//   frozen row 0 repeats the all-F value of column n at most).  A padding row never feeds a real one.  Every register stays finite:
//   kPadScoreF enters one sum per cell, whose other operand is an Ho.  Exactness: every value of a real cell is an integer of
//   magnitude below 2^24 and every positive H is below 2^19, so that the key's five mantissa bits are free (host_affine.h:
//   affine_ext_exact); the scale 2^-k moves no mantissa bit.
//   best[2 pid] = the best extension, cell[4 pid ..] = end_x, end_y (lengths; 0 / 0 at score 0); best[2 pid + 1] = max over
//   0 <= j <= n of H(m, j), cell[4 pid + 2 ..] = m and the smallest such column (0: the whole of x as one insertion).
// AffinePairGlob — sw_affine_pair_glob_kernel, ANCHORED AT BOTH ENDS (include/mi355_sw.h "global alignment between two anchors", lemma
//   L23): the anchored model, whose answer is the one cell H(m, n): the row-0 border and the corner capture.  Nothing competes: kKey
//   and kRowM are off — no max(H, 0), no key, no WaveKeyFold, no (blk, tl), no (best, te) and no compare of values.  Padding: a
//   padding row (> m) or column (> n) never feeds a real cell (F and the diagonal run downwards, E to the right), and the capture
//   reads a real cell by construction; every register stays finite as in the extension (kPadScoreF enters one sum per cell, whose
//   other operand is an Ho; row 0 is frozen at column n's value).  Exactness: every value of a real cell is an integer below 2^24 in
//   magnitude (host_affine.h: affine_glob_exact).  No key is formed, so no mantissa bit is reserved: the extension's
//   smax (rows + 1) < 2^18 has no counterpart here.  The scale 2^-k moves no bit.
//   best[pid] = H(m, n), of any sign; cell[2 pid ..] = m, n.
// A further mode is a trait set, its paragraph here and its entry point.
//
// Why the body is a file that an entry point includes, and why the local kernel above is not one of its modes: the compiled kernels
// are to stay what they are (profiles/affine_list_merge_isa_identity.txt).  Behind a call — a __forceinline__ function, by reference or
// by value — the optimiser meets the kernel's arguments and loops in another order, and local R = 24 went from 127 to 129 VGPRs, a
// wave per SIMD, global R = 5 from 60 to 68; included, the 18 instances below are the parent's instruction for instruction.  The
// local kernel's row loop through the body's `step` lambda schedules differently at R >= 24 (the same two VGPRs) whatever else is
// done, so it keeps its own text; a change of the scaffold visits the kernel above and the body, no longer four kernels.
struct AffinePairE2E {
  static constexpr bool kRow0 = false, kKey = false, kRowM = true, kCorner = false;
  static constexpr int kOuts = 1;
};
struct AffinePairExt {
  static constexpr bool kRow0 = true, kKey = true, kRowM = true, kCorner = false;
  static constexpr int kOuts = 2;
};
struct AffinePairGlob {
  static constexpr bool kRow0 = true, kKey = false, kRowM = false, kCorner = true;
  static constexpr int kOuts = 1;
};

// The entry points: a name per mode (public: include/mi355_sw.h documents them, mi355_sw_last_kernel reports them).
template <int R> __global__ __launch_bounds__(256) void sw_affine_pair_e2e_kernel(const AffinePairProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffinePairE2E;
#include "sw_affine_pair_body.inc"
}
template <int R> __global__ __launch_bounds__(256) void sw_affine_pair_ext_kernel(const AffinePairProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffinePairExt;
#include "sw_affine_pair_body.inc"
}
template <int R> __global__ __launch_bounds__(256) void sw_affine_pair_glob_kernel(const AffinePairProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffinePairGlob;
#include "sw_affine_pair_body.inc"
}

// dst[k] = src[n - 1 - k]: the reversed copies behind the backward pairs of the extension calls (no kernel above knows a direction)
__global__ __launch_bounds__(256) void reverse_bytes_kernel(const uint8_t *src, uint8_t *dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += stride) dst[k] = src[n - 1 - k];
}

}  // namespace mi355sw
