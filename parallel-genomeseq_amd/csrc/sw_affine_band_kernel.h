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
// a permutation of the slot's lanes (quad_perm, row_half_mirror, row_mirror: every lane has a source, no `old`)
template <int CTRL>
__device__ __forceinline__ int band_dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }

// ---- ONE BODY (sw_affine_band_body.inc), a mode is a set of traits, an entry point only names its mode ----
// Everything above is the scaffold of every mode: geometry, the two row_shl:1 moves for F, the max-plus scan for E, the windows of y
// and of x's classes in LDS, the cap, the (value, column) fold of the best and the branch at the slot's row m.  The traits:
//   kFloor     the LOCAL model, as the file's head states it: the zero floor in the cell (the clamped add), 0 outside the band (`old`
//              of the two row_shl moves and the initial registers: Ho = F = -o; cap 1 in the band, 0 beyond) and a free row 0.
//              Off, the ANCHORED model (the pair kernel's extension restricted to the cells lo <= j - i <= hi, lo <= 0 <= hi, i and j
//              counted from the anchor (0,0)), which has none of the three:
//                * no floor: the diagonal term is a plain add of Ho = H - o and the table's s + o;
//                * outside the band is -inf, not 0: the `old` operand of the two row_shl moves, the cap beyond diagonal W - 1 (one
//                  v_min_f32 against cap[r]: +inf in the band, -inf beyond, kept in a register) and the initial registers.  -inf only
//                  ever meets finite operands of add, sub, min and max: no NaN arises, and F of a capped register stays -inf (both
//                  its sources are capped registers or `old`);
//                * row 0 is the initial state: Ho = H(0,delta) - o on the diagonals 0 <= delta <= hi_e (hi_e <= n: all real columns),
//                  H(0,0) = 0 and H(0,delta) = -(o + (delta-1) e); every other register and every F is -inf.  Column 0 has no code of
//                  its own: column j < 1 is an `outside` column like j > n, whose diagonal term is lost in kPadScoreF, the cells of
//                  columns j < 0 stay -inf (all three sources are), so in column 0 E = -inf and H(i,0) = F(i,0) = max(F(i-1,0) - e,
//                  H(i-1,0) - o) = -(o + (i-1) e): the border.
//   kKey       the key fold of the best cell (head: Winner).  Without the floor over max(H, 0) — one more max per register: cell
//              (0,0) = 0 competes, a negative cell never wins, the final "no positive cell: 0 / 0 / 0" stands.
//   kRowM      the unfloored maximum of row m over the real columns 0 <= j <= n at the smallest column.  The slots of a wavefront
//              have different m and the loop runs to the longest: row m is folded only at the step where a slot of the wavefront
//              stands on its row m, behind one compare of the step's row with the slot's m per step (`it + 1 == m`).  As compiled that
//              is an exec-mask branch (s_and_saveexec, s_cbranch_execz): the wavefront jumps over the fold unless one of its slots
//              stands on its row m, so it runs the fold at most four times; no second fold per cell.  A lane's columns rise with r,
//              so a strict '>' keeps its smallest column; the lanes' (value, column) meet after the loop.  A pair whose band misses
//              row m (lo_e > n - m) yields -inf here: the host fills in "unreachable".
//   kCorner    the one cell H(m, n), READ, not folded: in row m the cell of column n lies on diagonal n - m, register D = n - m - lo.
//              Behind the same branch the lane that holds D takes Ho + o of that one register.  The host sends only pairs with
//              lo <= n - m <= lo + W - 1 (the corner lies in the band), so D is one of the 16 R registers and holds a finite value.
//              A slot reads at its own step, once; steps behind row m write nothing.
//   kZdrop     the stop rule over the rows and the early exit (AffineBandExtZ below); off, nothing of it is compiled.
//   kOuts      results (best, cell) a problem writes: one per fold or read.
// The modes:
// AffineBandLocal — sw_affine_band_kernel: the floor and the key (the file's head; exactness: DESIGN.md §3.8, L20).
//   best[pid] = the maximum (0 when no positive cell); cell[2 pid ..] = row, column (1-based) of the first maximum.
// AffineBandExt — sw_affine_band_ext_kernel, ANCHORED (include/mi355_sw.h "anchored seed extension inside a diagonal band", lemma L22):
//   two results, the best extension (kKey) and to the end (kRowM).  Padding (L22): a padding row (> m) or column (> n) has E and F
//   only, each derived by opening or extending a gap from a real cell of the same row or column — strictly below it, and that cell
//   lies in no later column — or from another padding cell; it wins neither fold (value first, and row m folds real columns at a
//   step where the slot stands on a real row).  Padding never feeds a real cell: F runs down a column, E to the right, the diagonal
//   stays on its diagonal.  Exactness: every value of a real cell is an integer of magnitude below 2^24 and every positive H is below
//   2^18, the key's five mantissa bits free (host_affine.h: affine_band_ext_exact); a decayed carry of the scan below -2^24 is
//   rounded, stays below every real value (rounding is monotone) and never wins a maximum.  The scale 2^-k moves no mantissa bit.
//   best[2 pid] = the best extension, cell[4 pid ..] = end_x, end_y (lengths; 0 / 0 at score 0); best[2 pid + 1] = max over the
//   in-band 0 <= j <= n of H(m, j), cell[4 pid + 2 ..] = m and the smallest such column.
// AffineBandGlob — sw_affine_band_glob_kernel, ANCHORED AT BOTH ENDS (include/mi355_sw.h "global alignment between two anchors", lemma
//   L23): the banded anchored model, whose answer is the one cell H(m, n): kCorner alone.  Nothing competes: no max(H, 0), no key,
//   no per-step fold and no (bval, bcol, brow) state.  Padding and exactness: as the extension, without its key — every value of a
//   real cell is an integer below 2^24 in magnitude (host_affine.h: affine_band_glob_exact), no mantissa bit is reserved.
//   best[pid] = H(m, n), of any sign; cell[2 pid ..] = m, n.
// AffineBandExtZ — sw_affine_band_extz_kernel, AffineBandExt under the Z-DROP STOP RULE (include/mi355_sw.h "z-drop", lemma L24): the
//   traits of AffineBandExt and kZdrop.  Per row i (step it = i - 1) every lane folds the unfloored maximum of its registers over the
//   REAL columns 0 <= j <= n at its smallest column (a capped register holds -inf; a padding column j > n can hold more than the
//   row's real cells — an F chain runs down column n + 1 — and is masked as the row-m fold masks it).  Four DPP permutations inside
//   the slot (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) leave the slot's maximum r_i in all 16 lanes, four more the
//   smallest column c_i among the lanes that hold it.  Every lane of the slot keeps the rule's state redundantly: B, the diagonal
//   bj - bi of the cell that set it (d = |(i - bi) - (c_i - bj)| is the distance of two diagonals) and the stop row.  The test is
//   r_i + d e < B - z: r_i + d e is an integer within (-2^24, smax m + (W - 1) e) units and B - z within (-2^24, 2^18) for z < 2^24, so
//   no intermediate needs a 25th bit (L24); r_i = -inf (no real in-band column) stops.  Row m is not tested.  A stopped slot keeps
//   executing: the step's key is replaced by -inf so that (bval, bcol, brow) freeze, the row-m fold is taken back (to the end: -inf /
//   -1) and the stop row goes where AffineBandExt writes m.  The wavefront leaves the row loop by a `break` under a ballot: none of
//   its four slots is alive (not stopped, row below m).  The loop stays `for (it < steps)`, so it ends whatever the data hold, and
//   there is no barrier in or behind it: the four wavefronts of a workgroup leave at different steps.  At its exit a wavefront adds
//   the rows its loop ran to *sa.zrows, one vector atomic.
//   best / cell: as AffineBandExt, with cell[4 pid + 2] = rows_done (the stop row, or m).
// A further mode is a trait set, its paragraph here and its entry point.  The compiled instances are the ones the three kernels were
// before they shared a body (profiles/affine_list_merge_isa_identity.txt).
struct AffineBandLocal {
  static constexpr bool kFloor = true, kKey = true, kRowM = false, kCorner = false;
  static constexpr bool kZdrop = false;
  static constexpr int kOuts = 1;
};
struct AffineBandExt {
  static constexpr bool kFloor = false, kKey = true, kRowM = true, kCorner = false;
  static constexpr bool kZdrop = false;
  static constexpr int kOuts = 2;
};
struct AffineBandGlob {
  static constexpr bool kFloor = false, kKey = false, kRowM = false, kCorner = true;
  static constexpr bool kZdrop = false;
  static constexpr int kOuts = 1;
};
struct AffineBandExtZ : AffineBandExt {
  static constexpr bool kZdrop = true;
};

// The entry points: a name per mode (public: include/mi355_sw.h documents them, mi355_sw_last_kernel reports them).  sa: as for
// sw_affine_pair_kernel
template <int R> __global__ __launch_bounds__(256) void sw_affine_band_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffineBandLocal;
#include "sw_affine_band_body.inc"
}
template <int R> __global__ __launch_bounds__(256) void sw_affine_band_ext_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffineBandExt;
#include "sw_affine_band_body.inc"
}
template <int R> __global__ __launch_bounds__(256) void sw_affine_band_glob_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffineBandGlob;
#include "sw_affine_band_body.inc"
}
template <int R> __global__ __launch_bounds__(256) void sw_affine_band_extz_kernel(const AffineBandProblem *probs, int nprob, const AffinePairArgs sa) {
  using MODE = AffineBandExtZ;
#include "sw_affine_band_body.inc"
}

}  // namespace mi355sw
