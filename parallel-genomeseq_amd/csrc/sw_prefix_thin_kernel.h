// sw_prefix_thin_kernel.h — the thin stage of the prefix filter (DESIGN.md §3.3 lemma L20, host_pipeline.h prefix_bucket round 2).
//
// A row-P pass flags sub-chunk s of read q when row P of the read's first P rows reaches the read's threshold there.  Lemma L20: an
// optimal alignment that crosses row P in the columns of sub-chunk s crosses the taller row P2 at most W12 columns further right, with
// H_P2(P2, c2) >= thr2[q].  So a flag need not go to the locate stage when row P2 of the read's first P2 rows stays below thr2 on
// [s E - 63, (s + 1) E + W12), and what survives is the sub-chunk(s) that hold such a cell.
//
// One item {query id, sub-chunk} per LANE: the lane sweeps the P2-row matrix of x[0:P2] column by column over
//   [s E - 64 - warm2, (s + 1) E + W12), clipped to the range [0, n),
// from a zero border, with the oracle's float32 cell rule (similaritymatrix.cpp:49-54; integer-valued scores: exact).  warm2 columns in
// front make every value that reaches thr2 > 0 exact on the own columns [s E - 63, ...) (the margin rule of Bucket::warm for P2 rows);
// whatever the border cuts off only lowers a value, never raises one.  The lanes of a wavefront hold different reads, so there is no
// profile per lane: the score table [256][ncodes] of the call sits in LDS and a lane keeps the byte offset of each of its P2 rows.
// State: P2 cells and P2 row offsets in registers, the row loop fully unrolled.
//
// Output: for every sub-chunk t that the own columns touch — t = s - 1 .. s + 1 + (W12 - 1) / E, 0-based column j lies in sub-chunk
// j / E — the maximum of row P2 over the own columns in t.  A maximum that reaches thr2[q] appends {q, t} to the survivor list (the
// list holds nitems * nout entries: it cannot overflow).  Test hook: every maximum also goes to vals[item * nout + (t - (s - 1))],
// -1 where the clipped window holds no column of t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi355sw {

struct ThinArgs {
  const uint2 *items;        // [nitems] {query id, sub-chunk of the range}, sorted by query id
  uint32_t nitems;
  const float *thr2;         // [nq] by query id, > 0 for every listed query
  const uint8_t *codes;      // reference codes of the RANGE's first column
  int64_t n;                 // columns of the range
  const uint8_t *qbytes;     // the batch's concatenated query bytes
  const int64_t *qoff;       // [nq]
  const float *ftab;         // [256][ncodes] score(query byte, reference code), unscaled
  int ncodes;
  float gap;
  int32_t E;                 // sub-chunk length (>= 64)
  int32_t warm2;             // warm-up columns in front of the own columns
  int32_t W12;               // columns a crossing of row P2 may lie right of the crossing of row P
  int32_t nout;              // sub-chunks per item: 3 + (W12 - 1) / E
  unsigned int *count;       // survivors appended
  uint2 *list;               // [nitems * nout]
  float *vals;               // test hook: [nitems][nout], or null
};

template <int P2>
__global__ __launch_bounds__(64) void sw_prefix_thin_kernel(const ThinArgs a) {
  extern __shared__ __attribute__((aligned(16))) float thin_tab[];
  for (int k = threadIdx.x; k < 256 * a.ncodes; k += 64) thin_tab[k] = a.ftab[k];
  __syncthreads();
  const uint32_t it = blockIdx.x * 64u + threadIdx.x;
  if (it >= a.nitems) return;                                        // (the last wavefront's idle lanes: before any item load)
  const uint2 item = a.items[it];
  const int q = (int)item.x;
  const int64_t s = (int64_t)item.y, E = a.E;
  const float thr = a.thr2[q], g = a.gap;
  const uint8_t *x = a.qbytes + a.qoff[q];
  int xo[P2];
  float h[P2];
#pragma unroll
  for (int i = 0; i < P2; ++i) { xo[i] = (int)x[i] * a.ncodes; h[i] = 0.0f; }
  const int64_t own_lo = s * E - 63 > 0 ? s * E - 63 : 0;
  const int64_t w_hi = (s + 1) * E + a.W12 < a.n ? (s + 1) * E + a.W12 : a.n;
  const int64_t w_lo = own_lo - 1 - a.warm2 > 0 ? own_lo - 1 - a.warm2 : 0;
  const int64_t t0 = s > 0 ? s - 1 : 0;                              // sub-chunk of own_lo (E >= 64 > 63)
  float *vrow = a.vals ? a.vals + (size_t)it * (size_t)a.nout : nullptr;
  if (vrow) for (int k = 0; k < a.nout; ++k) vrow[k] = -1.0f;
  int64_t t = t0, next = (t0 + 1) * E;                               // current sub-chunk and its end
  float mx = -1.0f;
  auto flush = [&]() {
    if (vrow) vrow[t - (s - 1)] = mx;
    if (mx >= thr) { const unsigned int at = atomicAdd(a.count, 1u); a.list[at] = make_uint2((unsigned int)q, (unsigned int)t); }
  };
  int c = w_lo < w_hi ? (int)a.codes[w_lo] : 0;
  for (int64_t j = w_lo; j < w_hi; ++j) {
    const int cn = j + 1 < w_hi ? (int)a.codes[j + 1] : 0;           // (the next column's code, loaded ahead of the row loop)
    float diag = 0.0f, up = 0.0f;
#pragma unroll
    for (int i = 0; i < P2; ++i) {
      const float left = h[i];
      const float xx = diag + thin_tab[xo[i] + c], yy = left - g, zz = up - g;
      const float v = fmaxf(fmaxf(xx, yy), fmaxf(zz, 0.0f));
      diag = left; up = v; h[i] = v;
    }
    if (j >= own_lo) {
      if (j == next) { flush(); ++t; next += E; mx = -1.0f; }
      mx = fmaxf(mx, up);
    }
    c = cn;
  }
  if (w_lo < w_hi && w_hi > own_lo) flush();
}

}  // namespace mi355sw
