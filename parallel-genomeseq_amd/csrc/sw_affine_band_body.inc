// sw_affine_band_body.inc — the body of the band kernels (sw_affine_band_kernel.h: the geometry, the traits, the modes; why a body is a
// file to include: sw_affine_pair_kernel.h).  Stands inside `template <int R> __global__ void name(const AffineBandProblem *probs,
// int nprob, const AffinePairArgs sa)` behind `using MODE = ...;`.
  static_assert(R >= 1 && R <= 32, "the key holds the register within the lane in five bits");
  static_assert(MODE::kOuts == (MODE::kKey ? 1 : 0) + (MODE::kRowM ? 1 : 0) + (MODE::kCorner ? 1 : 0), "one result per fold or read");
  static_assert(MODE::kFloor ? !MODE::kRowM && !MODE::kCorner : true, "row m is an answer of the anchored model");
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
  for (int p = l; p < steps + 16 * R; p += 16) {                   // entry p: column lo + 1 + p; without the floor column 0 is `outside` too
    const long long j = (long long)lo + 1 + p;
    const uint32_t c = (j >= 1 && j <= (long long)n) ? (uint32_t)yc[j - 1] : outside;
    yw[p] = (uint8_t)c;
  }
  for (int i = l; i < steps; i += 16) xw[i] = (uint16_t)(4u * (i < m ? (uint32_t)sa.cls[xb[i]] : (uint32_t)(sa.ncls - 1)));
  __syncthreads();

  const float ov = sa.open_s, ev = sa.ext_s;
  [[maybe_unused]] const float nopen = -sa.open_s;                 // kFloor, outside the band: H = 0 is Ho = -o, and F = -o
  // ninf: in front of the slot's first lane, no carry; without the floor also outside the band; pinf: the cap of a register inside it
  [[maybe_unused]] const float ninf = -__builtin_inff(), pinf = __builtin_inff();
  const float dec1 = (float)R * sa.ext_s, dec2 = 2.0f * dec1, dec4 = 4.0f * dec1, dec8 = 8.0f * dec1;
  float Ho[R], F[R], cap[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if constexpr (MODE::kFloor) { Ho[r] = nopen; F[r] = nopen; cap[r] = (l * R + r < W) ? 1.0f : 0.0f; }
    else {
      const int D = l * R + r, delta = lo + D;                     // row 0: cell (0, delta), in the band for D < W (delta <= hi_e <= n)
      const float h0 = delta == 0 ? 0.0f : -(sa.open_s + (float)(delta - 1) * sa.ext_s);
      Ho[r] = (D < W && delta >= 0) ? h0 - sa.open_s : ninf;
      F[r] = ninf;
      cap[r] = D < W ? pinf : ninf;
      asm volatile("" : "+v"(cap[r]));                             // (a register, so that the cap stays one v_min_f32 and not a min and a select)
    }
  }
  [[maybe_unused]] float bval = 0.0f;                              // kKey: the lane's best value, first seen at (brow, bcol)
  [[maybe_unused]] int brow = 0, bcol = 0x7fffffff;
  [[maybe_unused]] float eval = ninf;                              // kRowM: the lane's greatest H(m, j) at its smallest column
  [[maybe_unused]] int ecol = 0x7fffffff;
  [[maybe_unused]] float corner = ninf;                            // kCorner: H(m, n), in the lane that holds diagonal n - m
  [[maybe_unused]] const int dsel = n - m - lo - l * R;            // that diagonal's register within this lane (0..R-1: this lane holds it)
  const char *tab_b = reinterpret_cast<const char *>(tab);
  const uint8_t *yl = yw + l * R;
  [[maybe_unused]] const int col0 = lo + l * R + 1;                // column of register 0 in row 0 (it = 0 is row 1: + it)
  // kZdrop: the rule's running best B and the diagonal bj - bi of its cell, the stop row (0: none yet) — the same in every lane of the
  // slot — and the rows the wavefront's loop ran
  [[maybe_unused]] float zB = 0.0f;
  [[maybe_unused]] int zdiag = 0, zstop = 0, zrun = steps;

  for (int it = 0; it < steps; ++it) {
    const uint32_t xo = xw[it];
    const uint8_t *yp = yl + it;
    // diagonal D + 1 of the previous row for the lane's last register: register 0 of the next lane; the slot's last lane keeps `old`
    const float hnext = band_dpp<0x101>(MODE::kFloor ? nopen : ninf, Ho[0]);
    const float fnext = band_dpp<0x101>(MODE::kFloor ? nopen : ninf, F[0]);
    float Ht[R], q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float hon = r + 1 < R ? Ho[r + 1] : hnext;             // H(i-1, j) - o
      const float fpn = r + 1 < R ? F[r + 1] : fnext;              // F(i-1, j)
      const float s = *reinterpret_cast<const float *>(tab_b + (__umul24((uint32_t)yp[r], row_bytes) + xo));
      // plain C++ (an inline-asm definition costs a wait state in front of the VALU op that reads it on gfx950).  kFloor: the median
      // with 0 and 1 folds into the add's clamp, the maxima of results of arithmetic need no canonicalisation
      const float x = MODE::kFloor ? __builtin_amdgcn_fmed3f(Ho[r] + s, 0.0f, 1.0f) : Ho[r] + s;
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
    [[maybe_unused]] float mx = 0.0f, tpend = 0.0f;
    [[maybe_unused]] float zr = ninf;                              // kZdrop: the lane's greatest real cell of this row at its smallest column
    [[maybe_unused]] int zc = 0x3fffffff;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float h = r == 0 ? fmaxf(Ht[0], ce) : fmaxf(fmaxf(Ht[r], q[r - 1]), ce);
      h = fminf(h, cap[r]);
      if constexpr (MODE::kKey) WaveKeyFold::cell<R>(r, MODE::kFloor ? h : fmaxf(h, 0.0f), mx, tpend);   // no floor in the cell: the floor on the answer, cell (0,0) competes
      if constexpr (MODE::kZdrop) {
        const int j = col0 + it + r;                               // 0 <= j <= n in one unsigned compare; columns rise with r: '>' keeps the smallest
        const bool in = (uint32_t)j <= (uint32_t)n && h > zr;      // (a capped register holds -inf and never passes)
        zr = in ? h : zr;
        zc = in ? j : zc;
      }
      Ho[r] = h - ov;
      if (r + 1 < R) ce = ce - ev;
    }
    if constexpr (MODE::kZdrop) mx = zstop != 0 ? ninf : mx;       // a stopped slot: the key of -inf wins nothing, (bval, bcol, brow) freeze
    if constexpr (MODE::kKey) {
      // the step's best against the lane's: greater value, or the same value in a smaller column (header: Winner)
      const uint32_t kb = __float_as_uint(mx);
      const float v = __uint_as_float(kb & ~31u);
      const int col = col0 + it + (31 - (int)(kb & 31u));
      const bool take = v > bval || (v == bval && col < bcol);
      bval = take ? v : bval;
      bcol = take ? col : bcol;
      brow = take ? it + 1 : brow;
    }
    // row m: only at the step where the slot stands on its row m (an idle slot: m = 0, which no step matches); the wavefront skips
    // the block unless one of its four slots does
    if constexpr (MODE::kRowM || MODE::kCorner) {
      if (it + 1 == m) {
        if constexpr (MODE::kRowM) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int j = col0 + it + r;
            const float h = Ho[r] + ov;                            // H(m, j): exact, both are integers below 2^24 units
            const bool in = j >= 0 && j <= n && h > eval;          // (a capped register holds -inf and never passes)
            eval = in ? h : eval;
            ecol = in ? j : ecol;
          }
          if constexpr (MODE::kZdrop) {                            // a stopped slot never reached its row m: the fold is taken back
            eval = zstop != 0 ? ninf : eval;
            ecol = zstop != 0 ? 0x7fffffff : ecol;
          }
        }
        if constexpr (MODE::kCorner) {
#pragma unroll
          for (int r = 0; r < R; ++r) corner = dsel == r ? Ho[r] + ov : corner;   // H(m, n): exact, both are integers below 2^24 units
        }
      }
    }
    // the stop rule on row it + 1 (header: AffineBandExtZ; DESIGN.md §3.8, L24)
    if constexpr (MODE::kZdrop) {
      float rs = zr;                                               // the slot's r_i in every lane ...
      rs = fmaxf(rs, band_dpp<0xB1>(rs, rs));
      rs = fmaxf(rs, band_dpp<0x4E>(rs, rs));
      rs = fmaxf(rs, band_dpp<0x141>(rs, rs));
      rs = fmaxf(rs, band_dpp<0x140>(rs, rs));
      int rc = zr == rs ? zc : 0x3fffffff;                         // ... and c_i, the smallest column among the lanes that hold it
      rc = min(rc, band_dpp_i<0xB1>(rc));
      rc = min(rc, band_dpp_i<0x4E>(rc));
      rc = min(rc, band_dpp_i<0x141>(rc));
      rc = min(rc, band_dpp_i<0x140>(rc));
      const int row = it + 1, cdiag = rc - row;
      const bool live = zstop == 0 && row < m;                     // row m is never tested; an idle slot has m = 0
      const bool up = rs > zB;
      const int dd = zdiag > cdiag ? zdiag - cdiag : cdiag - zdiag;
      const bool drop = !up && rs + (float)dd * ev < zB - sa.zdrop_s;   // r_i = -inf: drops for every z
      zB = live && up ? rs : zB;
      zdiag = live && up ? cdiag : zdiag;
      zstop = live && drop ? row : zstop;
      if (__builtin_amdgcn_ballot_w64(zstop == 0 && row < m) == 0) { zrun = row; break; }   // wave-uniform: no slot of the wavefront is alive
    }
  }
  if constexpr (MODE::kZdrop) {
    if ((tid & 63) == 0) atomicAdd(sa.zrows, (unsigned long long)zrun);
  }

  // kKey: the lanes' winners -> the slot's
  float bv = 0.0f;
  long long bi = 0, bj = 0;
  if constexpr (MODE::kKey) {
    bv = bval * sa.unscale;
    bi = brow; bj = bcol;
    if (!(bv > 0.0f)) { bv = 0.0f; bi = 0; bj = 0; }
    slot_first_max(bv, bi, bj);
  }
  // kRowM: the lanes' (value, column) -> the slot's: value, then smaller column
  if constexpr (MODE::kRowM) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
      const float oe = __shfl_xor(eval, off, 16);
      const int oc = __shfl_xor(ecol, off, 16);
      if (oe > eval || (oe == eval && oc < ecol)) { eval = oe; ecol = oc; }
    }
  }
  // kCorner: the value of the lane that holds diagonal n - m, scaled here (kRowM's `eval` is scaled at its store)
  [[maybe_unused]] float cval = 0.0f;
  if constexpr (MODE::kCorner) {
    const int wd = n - m - lo;
    const int wl = (active && wd >= 0 && wd < 16 * R) ? wd / R : 0;
    cval = __shfl(corner, wl, 16) * sa.unscale;
  }
  if (l == 0 && active) {
    constexpr size_t NO = MODE::kOuts;
    if constexpr (MODE::kKey) sa.best[NO * (size_t)pid] = bv;
    if constexpr (MODE::kRowM) sa.best[NO * (size_t)pid + NO - 1] = eval * sa.unscale;
    if constexpr (MODE::kCorner) sa.best[NO * (size_t)pid + NO - 1] = cval;
    if constexpr (MODE::kKey) {
      sa.cell[2 * NO * (size_t)pid] = bv > 0.0f ? bi : 0;
      sa.cell[2 * NO * (size_t)pid + 1] = bv > 0.0f ? bj : 0;
    }
    if constexpr (MODE::kRowM || MODE::kCorner) {
      sa.cell[2 * NO * (size_t)pid + 2 * NO - 2] = MODE::kZdrop && zstop != 0 ? zstop : m;   // kZdrop: rows_done
      sa.cell[2 * NO * (size_t)pid + 2 * NO - 1] = MODE::kCorner ? n : ecol == 0x7fffffff ? -1 : ecol;
    }
  }
