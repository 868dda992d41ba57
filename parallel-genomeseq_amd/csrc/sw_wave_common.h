// sw_wave_common.h — the scaffold of the 16-lane slot kernels: sw_wave_kernel, sw_wave_prof_kernel, sw_wave_prof16_kernel
// (sw_wave_kernel.h) and sw_affine_prof_kernel (sw_affine_prof_kernel.h).  The scheme is described here once.  A helper is used in a
// kernel only where the instance compiles as it did with the piece written out, so copies remain that a scaffold change must visit:
// window (prime, rotate) and profile row fetch in all four kernels; step count and 16-lane reduction in sw_wave_kernel and
// sw_wave_prof_kernel; sw_wave_kernel's stage load of raw bytes; sw_affine_prof_kernel's profile fill.
//
// Geometry.  256 threads = 16 slots of 16 lanes, one problem per slot (two on packed float16 cells).  Lane l holds R consecutive
// cells of the short ("lane") side; the long side streams past.  At step k lane l works on stream position k - l, so a lane sees
// its left neighbour's last cell of the same position one step later, through one DPP row_shr:1: a skew of 15 steps, hence
// nb + 16 steps for a stream of nb positions (rounded up to a multiple of four by the kernels that stop inside a segment).
//
// Stream window.  Per slot 16 B of history + one 64 B segment in LDS.  Each lane stages four positions of a segment as one word,
// a segment ahead of its use; after the segment's 64 steps the last 16 bytes become the history (lane l then still reads positions
// up to 15 behind the segment's start) and the staged word goes in.  In front of the first step the history holds what matches
// nothing — or, where a problem resumes at step k0 > 0, the sixteen positions in front of k0.
//
// Winner.  The end cell is the FIRST maximum in column-major order (columns of the second sequence outer, rows of the first inner,
// strict '>').  The profile kernels keep one orderable key per lane, bits(H) | (31 - column in the lane): the host admits only
// scorings whose cells have their five lowest mantissa bits clear, so the key is still a positive float ordered by (value, smaller
// column first); per step a strict '>' keeps the first row.  Across the sixteen lanes: value, then smaller column, then smaller row.
// Padding columns (beyond the lane side) and positions outside the stream score kPadScoreF, which the cell's clamp turns into 0:
// such a cell holds max(0, neighbours - penalty), strictly below some real cell, so it can lead a lane for a while, never the slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_score_kernel.h"   // lane_stride, u32x4, kPadScoreF

namespace mi355sw {

struct WaveProblem {
  const uint8_t *a;      // sequence held on lanes: x (ORIENT 0) or y (ORIENT 1); na <= 16*R
  const uint8_t *b;      // streamed sequence: window of y (ORIENT 0) or window of x (ORIENT 1)
  int32_t na, nb;
  int64_t b_offset;      // true (1-based) stream index = b_offset + t + 1 for stream position t
  uint32_t *dirs;        // DIRS: [nb + 15][16][W] packed decisions (2 bits per cell, cell r of a lane at bit 2*(r%16)); lane l's
                         // decisions for stream position t are in row t + l (the step they were made at); or null
  float *best;           // TRACK: maximum (0 when no positive cell)
  int64_t *cell;         // TRACK: [2] = row (into x), column (into y), 1-based, of the first maximum
  // KEYED tracking (ORIENT 0): the first cell in the engine's storage order (order_key<>, sw_exact_kernel.h) among
  // the cells equal to `target` at stream positions >= own_lo; best = target when found, else -1
  float target;
  int32_t own_lo;
  int64_t full_n;        // |y| of the full problem (uint8 storage order)
  // sw_wave_prof_kernel only (checkpointed whole problems, host_batch.h).  TRACK without DIRS: where the state of the slot's
  // wavefront is saved after every kCkptEvery-th step (null: nowhere).  DIRS without TRACK: k0 > 0 resumes the problem at step k0
  // (a multiple of kCkptEvery) from the state saved there; nb is then the END of the rows to run, dirs rows count from step k0.
  float *ckpt;
  int32_t k0;
  // DIRS resumed from a state sw_wave_prof16_kernel saved: that kernel stores its packed registers as they are, one row of
  // 16 x (R + 1) dwords per saved state for the PAIR of problems a slot runs (ckpt of the pair's first problem); 1 / 2 = this
  // problem was the low / high half (0: float32 states of its own, sw_wave_prof_kernel<TRACK>)
  int32_t ck_half;
  // DIRS of a window that ENDS at the argmax (host_batch.h): the walk only moves up and to the left, so decisions are wanted of
  // the lanes up to the argmax column's; the launch then runs nb - k0 + lanes_used steps instead of nb - k0 + 16 (0: all lanes)
  int32_t lanes_used;
};

constexpr int kWaveSeg = 64;
constexpr int kWaveBuf = 16 + kWaveSeg;
constexpr int kCkptEvery = 32;           // steps between two saved states of a checkpointed pass (sw_wave_prof_kernel / sw_wave_prof16_kernel);
                                         // 16 was measured: decision pass 1.51 -> 1.32 ms, first pass 2.81 -> 2.93 ms, twice the states: not taken
constexpr int kCkptPerSeg = kWaveSeg / kCkptEvery;
static_assert(kWaveSeg % kCkptEvery == 0 && kCkptEvery % 4 == 0, "states are saved inside and at the end of every 64-step segment");

// the slot's problem, or one without rows, columns and outputs for a slot beyond the launch's last problem
__device__ __forceinline__ WaveProblem wave_problem_or_idle(const WaveProblem *probs, int pid, int nprob) {
  WaveProblem P;
  if (pid < nprob) P = probs[pid];
  else { P.a = nullptr; P.b = nullptr; P.na = 0; P.nb = 0; P.b_offset = 0; P.dirs = nullptr; P.best = nullptr; P.cell = nullptr;
         P.target = -1.0f; P.own_lo = 0; P.full_n = 0; P.ckpt = nullptr; P.k0 = 0; P.ck_half = 0; P.lanes_used = 0; }
  return P;
}

// stream positions c0 .. c0 + 3 as one word of window bytes; translate(in_range, byte) makes the window byte of a position (byte is
// read only inside the stream, else 0)
template <class T>
__device__ __forceinline__ uint32_t wave_stage_word(const uint8_t *b, int nb, int c0, T translate) {
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = c0 + k;
    const bool in = (uint32_t)t < (uint32_t)nb;
    w |= (uint32_t)translate(in, in ? (uint32_t)b[t] : 0u) << (8 * k);
  }
  return w;
}

// Steps a wavefront runs: the most of its four slots' stream positions + skew (wave-uniform); the segments that takes, and the count
// in fours for a last segment that stops at the last step.  (A sum handed in would carry its value range into the loop bounds.)
__device__ __forceinline__ void wave_steps(int positions, int skew, int &nseg, int &steps4) {
  int steps = positions + skew;
  steps = max(steps, __shfl_xor(steps, 16));
  steps = max(steps, __shfl_xor(steps, 32));
  nseg = (steps + kWaveSeg - 1) / kWaveSeg;
  steps4 = (steps + 3) & ~3;
}

// Profile fill by the whole workgroup: put(at, c, j) stores the entry of profile row c (a code or class of the stream's letters)
// and column j of the lane side, at dword `at` of a table [nrows][16][lane_stride(R)].  j runs over all 16 R columns: the caller
// stores the pad score where j is beyond the lane side.
template <int R, class P>
__device__ __forceinline__ void wave_fill_profile(int nrows, P put) {
  for (int e = threadIdx.x; e < nrows * 16 * R; e += 256) {
    const int c = e / (16 * R);
    const int rem = e - c * 16 * R;
    const int ll = rem / R, r = rem - ll * R;
    put((c * 16 + ll) * lane_stride(R) + r, c, ll * R + r);
  }
}

// The float32 key fold of a lane (header: Winner).  Per step: m = tpend = 0, cell<R>(r, h, m, tpend) for r = 0 .. R - 1, end(t, m).
struct WaveKeyFold {
  float blk = 0.0f;      // the lane's best key so far ...
  int tl = 0;            // ... and the stream position it was first seen at
  template <int R>
  __device__ __forceinline__ static void cell(int r, float h, float &m, float &tpend) {
    const float hk = __uint_as_float(__float_as_uint(h) | (uint32_t)(31 - r));     // (value, smaller column first)
    if (r & 1) asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(m), "v"(tpend), "v"(hk));   // one maximum3 per two cells
    else if (r + 1 < R) tpend = hk;
    else m = fmaxf(m, hk);
  }
  // strict '>': an equal key (same value, same column) at a later row does not replace the first
  __device__ __forceinline__ void end(int t, float m) {
    tl = m > blk ? t : tl;
    blk = fmaxf(blk, m);
  }
  // the lane's winner: value, row of x, column of y (1-based; zeros when no cell is positive)
  template <int R>
  __device__ __forceinline__ void winner(int l, float unscale, long long b_offset, float &bv, long long &bi, long long &bj) const {
    const uint32_t kb = __float_as_uint(blk);
    bv = __uint_as_float(kb & ~31u) * unscale;
    bj = (long long)l * R + (31 - (int)(kb & 31u)) + 1;
    bi = b_offset + tl + 1;
    if (!(bv > 0.0f)) { bv = 0.0f; bi = 0; bj = 0; }
  }
};

// the lanes' winners (value, row bi, column bj) -> the slot's: value, then smaller column, then smaller row; in every lane
__device__ __forceinline__ void slot_first_max(float &bv, long long &bi, long long &bj) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 16);
    const long long oi = __shfl_xor(bi, off, 16);
    const long long oj = __shfl_xor(bj, off, 16);
    if (ov > bv || (ov == bv && ov > 0.0f && (oj < bj || (oj == bj && oi < bi)))) { bv = ov; bi = oi; bj = oj; }
  }
}

// the slot's winner to the problem's outputs (P: the slot's problem, a copy or where it lies; read only in an active slot)
__device__ __forceinline__ void wave_store_winner(const WaveProblem *P, bool active, int l, float bv, long long bi, long long bj) {
  if (l == 0 && active) {
    *P->best = bv;
    P->cell[0] = bv > 0.0f ? bi : 0;
    P->cell[1] = bv > 0.0f ? bj : 0;
  }
}

}  // namespace mi355sw
