// sw_affine_pair_body.inc — the body of the non-local pair kernels (sw_affine_pair_kernel.h: the traits, the modes, and why this is a
// file to include).  Stands inside `template <int R> __global__ void name(const AffinePairProblem *probs, int nprob, const
// AffinePairArgs sa)` behind `using MODE = ...;`.  A test on MODE alone discards at once; one that also depends on the step lambda's
// BORDER would still capture what it names, and the lambda's captures are part of the compiled code: nest it inside the MODE test.
  static_assert(R >= 1 && R <= 32, "the key holds the row within the lane in five bits");
  static_assert(MODE::kOuts == (MODE::kKey ? 1 : 0) + (MODE::kRowM ? 1 : 0) + (MODE::kCorner ? 1 : 0), "one result per fold or capture");
  constexpr bool kSelM = MODE::kRowM || MODE::kCorner;             // the row-m select
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
  // row 0 as the slot's first lane sees it.  kRow0: Ho(0, j) = F(1, j) = -(2 o + (j - 1) e), column j = step + 1; never below column
  // n's.  Else both are the one value -o: H = 0 is Ho = -o, and F = -o
  [[maybe_unused]] const int nopen = (int)__float_as_uint(-sa.open_s);
  [[maybe_unused]] float rowo = -2.0f * sa.open_s;
  [[maybe_unused]] const float rowmin = -(2.0f * sa.open_s + (float)max(n - 1, 0) * sa.ext_s);
  // column 0: Ho = E = H(i,0) - o = -(2 o + (i - 1) e) of the lane's first row, i - 1 = l R (integers below 2^24 units: exact)
  const float bord0 = -(2.0f * sa.open_s + (float)(l * R) * sa.ext_s);
  float E[R], Ho[R];
#pragma unroll
  for (int r = 0; r < R; ++r) { E[r] = bord0 - (float)r * sa.ext_s; Ho[r] = E[r]; }   // lane 0 stands on column 0 here
  float up_prev = -ov;                                             // Ho of the previous lane's last row, one column to the left; lane 0: Ho(0, 0)
  float fout = -ov;                                                // F this lane hands to the next one
  const float ninf = -__builtin_inff();
  [[maybe_unused]] float blk = 0.0f, blk31 = __uint_as_float(31u); // kKey: the lane's best key, and the same with its row bits set
  [[maybe_unused]] int tl = 0;                                     // kKey: the column (0-based) blk was first seen at
  [[maybe_unused]] float best = ninf;                              // kRowM: the greatest H(m, j) so far, first seen at column te (0-based)
  [[maybe_unused]] int te = 0;
  [[maybe_unused]] float corner = ninf;                            // kCorner: H(m, n), in the lane that holds row m
  [[maybe_unused]] const int tcap = n - 1;                         // kCorner: the lane's column n (0-based): the one step that is captured
  const uint32_t row_bytes = 4u * (uint32_t)sa.ncls;
  const char *tab_b = reinterpret_cast<const char *>(tab);
  // the one cell of a column that row m has: lane (m - 1) / R, row (m - 1) % R (no lane of an idle slot)
  const int wrow = (m > 0 && (m - 1) / R == l) ? (m - 1) % R : -1;
  bool wsel[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wsel[r] = wrow == r;

  // one step of the lane: column t = gstep - l of the window, code at buf_lane[k].  BORDER (the first 16 steps): the lane whose
  // t is -1 stands on column 0 and takes the border instead of what it computed
  auto step = [&](auto border, const int gstep, const int k) {
    constexpr bool BORDER = decltype(border)::value;
    const int t = gstep - l;                                       // this lane's column of the window (0-based)
    const uint32_t c = (uint32_t)buf_lane[k];
    const char *rowp = tab_b + c * row_bytes;
    // the previous lane's last row in this column: Ho and the F it hands on; the slot's first lane keeps `old`, row 0
    const int old = MODE::kRow0 ? (int)__float_as_uint(rowo) : nopen;
    const float up = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(old, (int)__float_as_uint(Ho[R - 1]), 0x111, 0xf, 0xf, false));
    float frun = __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(old, (int)__float_as_uint(fout), 0x111, 0xf, 0xf, false));
    if constexpr (MODE::kRow0) rowo = fmaxf(rowo - ev, rowmin);
    float diag = up_prev;                                          // H(i-1, j-1) - o
    up_prev = up;
    [[maybe_unused]] float hm = ninf;                              // kRowM, kCorner: H(m, t + 1) in the lane that holds row m
    [[maybe_unused]] float mx = 0.0f, tpend = 0.0f;                // kKey: the step's key fold
    const bool on_border = BORDER && t == -1;
    float bord = bord0;
    float sv[R];                                                   // the step's R table values, all requested in front of the row loop
#pragma unroll
    for (int r = 0; r < R; ++r) sv[r] = *reinterpret_cast<const float *>(rowp + boff[r]);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float w = Ho[r];                                       // H(i, j-1) - o
      const float s = sv[r];
      float x, g, h, ho, fs;
      [[maybe_unused]] float hp;                                   // kKey: max(H, 0)
      asm("v_add_f32 %0, %1, %2" : "=v"(x) : "v"(diag), "v"(s));   // no clamp: no floor
      asm("v_sub_f32 %0, %1, %2" : "=v"(g) : "v"(E[r]), "v"(ev));
      asm("v_max_f32 %0, %1, %2" : "=v"(g) : "v"(g), "v"(w));
      asm("v_max3_f32 %0, %1, %2, %3" : "=v"(h) : "v"(x), "v"(g), "v"(frun));
      if constexpr (kSelM) hm = wsel[r] ? h : hm;
      if constexpr (MODE::kKey) {
        asm("v_max_f32 %0, 0, %1" : "=v"(hp) : "v"(h));            // the floor on the answer: cell (0,0) competes
        WaveKeyFold::cell<R>(r, hp, mx, tpend);
      }
      asm("v_sub_f32 %0, %1, %2" : "=v"(ho) : "v"(h), "v"(ov));
      asm("v_sub_f32 %0, %1, %2" : "=v"(fs) : "v"(frun), "v"(ev));
      asm("v_max_f32 %0, %1, %2" : "=v"(frun) : "v"(fs), "v"(ho));
      if constexpr (BORDER) { g = on_border ? bord : g; ho = on_border ? bord : ho; bord -= ev; }
      E[r] = g;
      Ho[r] = ho;
      diag = w;
    }
    fout = frun;
    if constexpr (MODE::kKey) {                                    // a later column wins only with a greater VALUE
      const bool take = mx > blk31;
      tl = take ? t : tl;
      blk = take ? mx : blk;
    }
    if constexpr (MODE::kRowM) {                                   // only a strictly greater value: the smallest column stays
      const bool take_e = hm > best;
      te = take_e ? t : te;
      best = take_e ? hm : best;
    }
    // at the border step every fold restarts (the mode's test outside: what a dependent test discards, the lambda still captures)
    if constexpr (MODE::kKey) { if constexpr (BORDER) blk = on_border ? 0.0f : blk; }
    if constexpr (MODE::kRowM) { if constexpr (BORDER) best = on_border ? ninf : best; }
    if constexpr (MODE::kKey) blk31 = __uint_as_float(__float_as_uint(blk) | 31u);
    if constexpr (MODE::kCorner) corner = t == tcap ? hm : corner; // the capture: the slot's own column n, once
  };

  for (int seg = 0; seg < nseg; ++seg) {
    const int kq = min(kWaveSeg, steps4 - seg * kWaveSeg) >> 2;
    int k4 = 0;
    if (seg == 0) {                                                // the 16 steps that hold every lane's border step (steps4 >= 16)
#pragma unroll 1
      for (int k = 0; k < 16; ++k) step(std::true_type(), k, k);
      k4 = 4;
    }
    for (; k4 < kq; ++k4) {
#pragma unroll
      for (int ku = 0; ku < 4; ++ku) step(std::false_type(), seg * kWaveSeg + 4 * k4 + ku, 4 * k4 + ku);
    }
    const uint32_t hist = buf32[kWaveSeg / 4 + (l & 3)];
    if (l < 4) buf32[l] = hist;
    buf32[4 + l] = nextc;
    nextc = stage_load(seg + 2);
  }

  // kKey: the lane's winner — value, row of x, column of the window (1-based) — then the slot's
  float bv = 0.0f;
  long long bi = 0, bj = 0;
  if constexpr (MODE::kKey) {
    const uint32_t kb = __float_as_uint(blk);
    bv = __uint_as_float(kb & ~31u) * sa.unscale;
    bi = (long long)l * R + (31 - (int)(kb & 31u)) + 1;
    bj = (long long)tl + 1;
    if (!(bv > 0.0f)) { bv = 0.0f; bi = 0; bj = 0; }
    slot_first_max(bv, bi, bj);
  }
  // kRowM, kCorner: value and column of the lane that holds row m.  kRowM under kRow0: then column 0, H(m,0) = -(o + (m-1) e), which
  // wins a tie — value and column stay unscaled and 1-based until that is decided; without it they are final here (where each form
  // stands is the entry points' compiled code, as every statement order of this body)
  constexpr bool kTie = MODE::kRowM && MODE::kRow0;
  const int wl = m > 0 ? (m - 1) / R : 0;
  float ev_best = 0.0f;
  [[maybe_unused]] long long ej = 0;                               // kTie: the column, 1-based (0: column 0)
  [[maybe_unused]] int et = 0;                                     // kRowM without kTie: the column, 0-based
  if constexpr (kTie) {
    ev_best = __shfl(best, wl, 16);
    ej = (long long)__shfl(te, wl, 16) + 1;
    const float col0 = -(sa.open_s + (float)max(m - 1, 0) * sa.ext_s);
    if (col0 >= ev_best) { ev_best = col0; ej = 0; }
  } else if constexpr (MODE::kRowM) {
    ev_best = __shfl(best, wl, 16) * sa.unscale;
    et = __shfl(te, wl, 16);
  } else if constexpr (MODE::kCorner) {
    ev_best = __shfl(corner, wl, 16) * sa.unscale;
  }
  if (l == 0 && active) {
    constexpr size_t NO = MODE::kOuts;
    if constexpr (MODE::kKey) sa.best[NO * (size_t)pid] = bv;
    if constexpr (kSelM) sa.best[NO * (size_t)pid + NO - 1] = kTie ? ev_best * sa.unscale : ev_best;
    if constexpr (MODE::kKey) {
      sa.cell[2 * NO * (size_t)pid] = bv > 0.0f ? bi : 0;
      sa.cell[2 * NO * (size_t)pid + 1] = bv > 0.0f ? bj : 0;
    }
    if constexpr (kSelM) {
      sa.cell[2 * NO * (size_t)pid + 2 * NO - 2] = m;
      sa.cell[2 * NO * (size_t)pid + 2 * NO - 1] = kTie ? ej : MODE::kCorner ? (long long)n : (long long)et + 1;
    }
  }
