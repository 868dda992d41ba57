// sw_affine_prof_kernel.h — affine-gap (Gotoh) database search against ONE SHORT second sequence, hand-written HIP for gfx950.
//
// The third score kernel of the affine path (sw_affine_kernel.h): many database sequences x, each against the same
// y of at most 512 letters (a range of the resident reference).  Slot geometry, stream window and winner: sw_wave_common.h; lane l
// holds columns l R .. l R + R - 1 of y, the rows of x stream.  The affine, table-scoring counterpart of sw_wave_prof_kernel<R,
// TRACK = true, DIRS = false> (sw_wave_kernel.h).
//
//   E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)     runs along the columns of y: down the lane's R columns within a step (Erun),
//                                                handed to the next lane by one DPP row_shr:1
//   F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)     runs along the rows of x: one register per column
//   H(i,j) = max(0, H(i-1,j-1) + s, E, F)
//
// Cells are float32 scaled by 2^-k (2^k above every value: the host admits integer scores with smax (|y| + 1) < 2^18 and
// gap_open < 2^18, so every value is an integer multiple of 2^-k with fewer than 19 significant bits: exact).  Per column the lane
// keeps F[r] and Ho[r] = H - o only; the profile holds s + o, so that the diagonal term needs no H register:
//     x     = v_add_f32 clamp(Ho(i-1,j-1), s + o)         = max(0, H(i-1,j-1) + s): the [0, 1] clamp is the zero floor
//     F[r]  = max(F[r] - e, Ho[r])                        Ho[r] still holds H(i-1,j) - o
//     H     = max3(x, F[r], Erun)
//     Ho[r] = H - o
//     Erun  = max(Erun - e, Ho[r])                        E of the next column
// seven float32 ops per cell.  Borders: H = 0, i.e. Ho = -o, and E = F = -o, which gives the same cells as -infinity (lemma L15 (d));
// the slot's first lane takes both border values from the `old` operand of its two DPP moves.
//
// Profile: prof[class][lane][r] at lane_stride(R), read with ds_read_b128.  The class of a letter of x is the set of bytes with the
// same row of scores against the reference's letters (identity scoring: one per letter of y and one for all others; a 20-letter
// table: 21); one more class, "outside", for the steps in front of and beyond the stream.  Padding columns (j >= |y|) and the
// outside class score kPadScoreF: their H is max(0, E, F), strictly below a real cell (L15 (e)), so they never win.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_wave_common.h"

namespace mi355sw {

struct AffineProfArgs {
  const float *ctab;         // [nclass][nletters]: (s + o) * 2^-k of a class of x's bytes against a letter (code) of the reference;
                             // the last class is "outside": kPadScoreF
  const uint8_t *cls;        // [256] byte of x -> class
  int32_t nclass, nletters;
  float open_s, ext_s;       // o and e * 2^-k
  float unscale;             // 2^k
};

// probs: WaveProblem as batch_wave_setup writes them for orient 1 without decisions, with a = the CODES of the range of the
// reference (the same for every problem of the launch), b = the bytes of x.
template <int R>
__global__ __launch_bounds__(256) void sw_affine_prof_kernel(const WaveProblem *probs, int nprob, const AffineProfArgs sa) {
  static_assert(R >= 1 && R <= 32, "the key holds the column within the lane in five bits");
  extern __shared__ __attribute__((aligned(16))) uint32_t apsmem[];
  __shared__ __attribute__((aligned(16))) uint8_t win[16 * kWaveBuf];
  __shared__ uint8_t cls_s[256];
  float *prof = reinterpret_cast<float *>(apsmem);                 // [nclass][16][lane_stride(R)]
  const int tid = threadIdx.x;
  const int l = tid & 15;
  const int slot = tid >> 4;
  const int pid = blockIdx.x * 16 + slot;
  const bool active = pid < nprob;
  const uint8_t *xb = nullptr;
  int nb = 0;
  if (active) { xb = probs[pid].b; nb = probs[pid].nb; }
  // the lane side is the same for every problem of the launch (the range of the resident reference)
  const uint8_t *ycodes = probs[blockIdx.x * 16].a;
  const int na = probs[blockIdx.x * 16].na;
  const uint32_t outside = (uint32_t)(sa.nclass - 1);
  cls_s[tid] = sa.cls[tid];
  for (int e = tid; e < sa.nclass * 16 * R; e += 256) {
    const int c = e / (16 * R);
    const int rem = e - c * 16 * R;
    const int ll = rem / R, r = rem - ll * R;
    const int j = ll * R + r;
    float v = kPadScoreF;                                          // padding columns: the clamp makes 0 of them
    if (j < na) v = sa.ctab[c * sa.nletters + (int)ycodes[j]];
    prof[(c * 16 + ll) * lane_stride(R) + r] = v;
  }
  __syncthreads();

  // stream window of CLASSES (in front of the first row and beyond the last: `outside`)
  auto stage_load = [&](int seg) -> uint32_t {
    return wave_stage_word(xb, nb, seg * kWaveSeg + 4 * l, [&](bool in, uint32_t byte) { return in ? (uint32_t)cls_s[byte] : outside; });
  };
  int nseg, steps4;
  wave_steps(nb, 16, nseg, steps4);
  uint8_t *buf = win + slot * kWaveBuf;
  uint32_t *buf32 = reinterpret_cast<uint32_t *>(buf);
  const uint8_t *buf_lane = buf + 16 - l;
  uint32_t nextc = stage_load(0);
  if (l < 4) buf32[l] = outside * 0x01010101u;                     // history in front of the first row
  buf32[4 + l] = nextc;
  nextc = stage_load(1);

  float ov = sa.open_s, ev = sa.ext_s;
  asm volatile("" : "+v"(ov), "+v"(ev));                           // (VGPR operands: v_sub_f32 then issues at the double rate)
  const int nopen = (int)__float_as_uint(-sa.open_s);              // both border values: H = 0 is Ho = -o, and E = -o
  float F[R], Ho[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { F[r] = -ov; Ho[r] = -ov; }
  float up_prev = -ov;                                             // Ho of the previous lane's last column, one row up
  float eout = -ov;                                                // E this lane hands to the next one
  WaveKeyFold key;
  const float *prof_lane = prof + l * lane_stride(R);

  for (int seg = 0; seg < nseg; ++seg) {
    const int kq = min(kWaveSeg, steps4 - seg * kWaveSeg) >> 2;
    for (int k4 = 0; k4 < kq; ++k4) {
#pragma unroll
      for (int ku = 0; ku < 4; ++ku) {
        const int k = 4 * k4 + ku;
        const int t = seg * kWaveSeg + k - l;                      // this lane's row of x (0-based)
        const uint32_t c = (uint32_t)buf_lane[k];
        const u32x4 *pp = static_cast<const u32x4 *>(__builtin_assume_aligned(prof_lane + c * (16 * lane_stride(R)), 16));
        uint32_t p[(R + 3) / 4 * 4];
#pragma unroll
        for (int q = 0; q < (R + 3) / 4; ++q) {
          const u32x4 v = pp[q];
          p[4 * q + 0] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
        }
        // the previous lane's last column in this row: Ho and the E it hands on; the slot's first lane keeps `old`, the border
        const float up = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(nopen, (int)__float_as_uint(Ho[R - 1]), 0x111, 0xf, 0xf, false));
        float erun = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(nopen, (int)__float_as_uint(eout), 0x111, 0xf, 0xf, false));
        float diag = up_prev;                                      // H(i-1, j-1) - o
        up_prev = up;
        float m = 0.0f, tpend = 0.0f;
        (void)tpend;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float w = Ho[r];                                   // H(i-1, j) - o
          float x, f, h, ho, es;
          asm("v_add_f32_e64 %0, %1, %2 clamp" : "=v"(x) : "v"(diag), "v"(__uint_as_float(p[r])));
          asm("v_sub_f32 %0, %1, %2" : "=v"(f) : "v"(F[r]), "v"(ev));
          asm("v_max_f32 %0, %1, %2" : "=v"(f) : "v"(f), "v"(w));
          asm("v_max3_f32 %0, %1, %2, %3" : "=v"(h) : "v"(x), "v"(f), "v"(erun));
          WaveKeyFold::cell<R>(r, h, m, tpend);
          asm("v_sub_f32 %0, %1, %2" : "=v"(ho) : "v"(h), "v"(ov));
          asm("v_sub_f32 %0, %1, %2" : "=v"(es) : "v"(erun), "v"(ev));
          asm("v_max_f32 %0, %1, %2" : "=v"(erun) : "v"(es), "v"(ho));
          F[r] = f;
          Ho[r] = ho;
          diag = w;
        }
        eout = erun;
        key.end(t, m);
      }
    }
    const uint32_t hist = buf32[kWaveSeg / 4 + (l & 3)];
    if (l < 4) buf32[l] = hist;
    buf32[4 + l] = nextc;
    nextc = stage_load(seg + 2);
  }

  float bv;
  long long bi, bj;
  key.template winner<R>(l, sa.unscale, 0, bv, bi, bj);
  slot_first_max(bv, bi, bj);
  wave_store_winner(probs + pid, active, l, bv, bi, bj);
}

}  // namespace mi355sw
