// mirror_cell_rate.hip — can the third op of the packed float16 score cell issue at the double rate?
// The cell of sw_score_kernel<R, kSemF16> is three VOP3P ops per register (two cells):
//     x = v_pk_add_f16 clamp(H_nw, s);  H = v_pk_maximum3_f16(x, Hg_w, Hg_n);  Hg = v_pk_add_f16(H, -g)
// In the mirrored cell (N = 1 - H/2048, one float16 binade, DESIGN.md §3.3 lemma L14) the last op is an integer add on the
// bit pattern of both halves at once:
//     x = v_pk_add_f16 clamp(N_nw, -s);  N = v_pk_minimum3_f16(x, K_w, K_n);  K = v_add_u32(N, g * 0x00010001)
// (1) issue rate of the single instructions (8 independent chains per wave, like valu_rate.hip);
// (2) the R = 19 cell loop of the bench instance (8-lane tiles: DPP row_shr:1 plus one border op per step, the running maximum
//     every 4th step, one maximum3 per two rows) in three forms — today's, mirrored with the gap in an SGPR, mirrored with the
//     gap in a VGPR — at 2 / 4 / 6 wavefronts per SIMD, in cycles per cell PAIR (one register) and lane.
#include <hip/hip_runtime.h>
#include <cstdio>
#define ITERS 4096
#define BODY(INSTR) \
  for (int it = 0; it < ITERS; ++it) { \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) { \
      asm volatile(INSTR(0) INSTR(1) INSTR(2) INSTR(3) INSTR(4) INSTR(5) INSTR(6) INSTR(7) \
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) : "v"(b), "v"(c), "s"(sg)); } }
#define K(name, INSTR) __global__ __launch_bounds__(256) void name(unsigned* out, unsigned b, unsigned c, unsigned sg) { \
  unsigned a[8]; for (int i=0;i<8;++i) a[i]=0x3a003a00u+threadIdx.x*i; BODY(INSTR) unsigned s=0; for(int i=0;i<8;++i) s^=a[i]; out[blockIdx.x*256+threadIdx.x]=s; }

#define I_ADDU32V(n) "v_add_u32 %" #n ", %" #n ", %8\n"
#define I_ADDU32S(n) "v_add_u32 %" #n ", %10, %" #n "\n"
#define I_PKADDF16S(n) "v_pk_add_f16 %" #n ", %" #n ", %10\n"
#define I_PKADDF16C(n) "v_pk_add_f16 %" #n ", %" #n ", %8 clamp\n"
#define I_PKMAX3(n) "v_pk_maximum3_f16 %" #n ", %" #n ", %8, %9\n"
#define I_PKMIN3(n) "v_pk_minimum3_f16 %" #n ", %" #n ", %8, %9\n"
#define I_BFI(n) "v_bfi_b32 %" #n ", %" #n ", %8, %10\n"
K(k_addu32v, I_ADDU32V) K(k_addu32s, I_ADDU32S) K(k_pkaddf16s, I_PKADDF16S) K(k_pkaddf16c, I_PKADDF16C) K(k_pkmax3, I_PKMAX3)
K(k_pkmin3, I_PKMIN3) K(k_bfi, I_BFI)

// ---- the cell loop ---------------------------------------------------------------------------
// FORM 0: today's kSemF16 cell (v_pk_add_f16 clamp, v_pk_maximum3_f16, v_pk_add_f16 with -g in an SGPR); border v_and_b32
// FORM 1: mirrored (v_pk_add_f16 clamp, v_pk_minimum3_f16, v_add_u32 with g * 0x00010001 in an SGPR); border bit-select
// FORM 2: FORM 1 with the gap constant in a VGPR
template <int R, int FORM>
__global__ __launch_bounds__(256) void k_cell(unsigned* out, const unsigned* pin, unsigned gap2, int steps) {
  constexpr bool M = FORM != 0;
  constexpr unsigned Z = M ? 0x3C003C00u : 0u;                      // H = 0
  unsigned H[R], Hg[R], p[4];                                       // (the kernel reads p from LDS every step: 4 registers here)
  unsigned gv = gap2;
  if (FORM == 2) asm volatile("" : "+v"(gv));
  auto sub_gap = [&](unsigned t) -> unsigned {
    unsigned r;
    if (FORM == 0) asm volatile("v_pk_add_f16 %0, %1, %2" : "=v"(r) : "v"(t), "s"(gap2));
    else if (FORM == 1) asm volatile("v_add_u32 %0, %1, %2" : "=v"(r) : "s"(gap2), "v"(t));
    else asm volatile("v_add_u32 %0, %1, %2" : "=v"(r) : "v"(gv), "v"(t));
    return r;
  };
  for (int r = 0; r < R; ++r) { H[r] = Z; Hg[r] = sub_gap(Z); }
  for (int r = 0; r < 4; ++r) p[r] = pin[(threadIdx.x * 4 + r) & 1023];
  unsigned up_prev = Z, mx = Z;
  unsigned first = (threadIdx.x & 7) == 0 ? 0u : 0xFFFFFFFFu;
  asm volatile("" : "+v"(first));
  for (int t = 0; t < steps; t += 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned up;
      if (!M) {
        up = (unsigned)__builtin_amdgcn_update_dpp(0, (int)H[R - 1], 0x111, 0xf, 0xf, true);
        up &= first;
      } else {
        up = (unsigned)__builtin_amdgcn_update_dpp((int)Z, (int)H[R - 1], 0x111, 0xf, 0xf, false);
        up = (up & first) | (Z & ~first);
      }
      unsigned diag = up_prev;
      up_prev = up;
      unsigned ng = sub_gap(up);
      unsigned tp = Z;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const unsigned w = H[r];
        unsigned x, h;
        asm volatile("v_pk_add_f16 %0, %1, %2 clamp" : "=v"(x) : "v"(diag), "v"(p[r & 3]));
        if (!M) asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(h) : "v"(x), "v"(Hg[r]), "v"(ng));
        else asm volatile("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(h) : "v"(x), "v"(Hg[r]), "v"(ng));
        if (k == 3) {                                                    // running maximum every 4th step
          if (r & 1) {
            if (!M) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(mx) : "v"(tp), "v"(h));
            else asm volatile("v_pk_minimum3_f16 %0, %0, %1, %2" : "+v"(mx) : "v"(tp), "v"(h));
          } else if (r + 1 < R) tp = h;
          else {
            if (!M) asm volatile("v_pk_max_f16 %0, %0, %1" : "+v"(mx) : "v"(h));
            else asm volatile("v_pk_min_f16 %0, %0, %1" : "+v"(mx) : "v"(h));
          }
        }
        diag = w;
        H[r] = h;
        ng = Hg[r] = sub_gap(h);
      }
    }
  }
  unsigned s = mx;
  for (int r = 0; r < R; ++r) s ^= H[r];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

typedef void (*kfn)(unsigned*, unsigned, unsigned, unsigned);
typedef void (*cfn)(unsigned*, const unsigned*, unsigned, int);
int main() {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
  const int ncu = prop.multiProcessorCount;
  const double clk = prop.clockRate * 1e3;                                  // Hz (peak engine clock)
  printf("%s, %d CUs, clock %.0f MHz\n", prop.gcnArchName, ncu, clk * 1e-6);
  unsigned* out; if (hipMalloc(&out, (size_t)ncu * 8 * 256 * 4) != hipSuccess) return 1;
  unsigned *pin0, *pin1;
  if (hipMalloc(&pin0, 4096) != hipSuccess || hipMalloc(&pin1, 4096) != hipSuccess) return 1;
  // profile entries: +3 / -3 scaled by 1/2048 as float16 in both halves (today's cell) and their negation (mirrored cell)
  unsigned hp0[1024], hp1[1024];
  for (int i = 0; i < 1024; ++i) { hp0[i] = ((i * 7) % 4 == 0) ? 0x1A001A00u : 0x9A009A00u; hp1[i] = hp0[i] ^ 0x80008000u; }
  hipMemcpy(pin0, hp0, 4096, hipMemcpyHostToDevice);
  hipMemcpy(pin1, hp1, 4096, hipMemcpyHostToDevice);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  struct E { const char* n; kfn f; } es[] = {
    {"v_add_u32 vgpr", k_addu32v}, {"v_add_u32 sgpr", k_addu32s}, {"v_pk_add_f16 sgpr", k_pkaddf16s},
    {"v_pk_add_f16 clamp", k_pkaddf16c}, {"v_pk_maximum3_f16", k_pkmax3}, {"v_pk_minimum3_f16", k_pkmin3}, {"v_bfi_b32", k_bfi}};
  for (int wps : {2, 4, 6}) {
    printf("== %d waves/SIMD\n", wps);
    for (auto& e : es) {
      dim3 grid(ncu * wps), block(256);
      hipLaunchKernelGGL(e.f, grid, block, 0, 0, out, 0x00080008u, 0x3a003a00u, 0x00040004u);
      hipDeviceSynchronize();
      hipEventRecord(e0);
      hipLaunchKernelGGL(e.f, grid, block, 0, 0, out, 0x00080008u, 0x3a003a00u, 0x00040004u);
      hipEventRecord(e1); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1);
      printf("%-24s %8.3f ms  %.2f cycles/wave-instr/SIMD\n", e.n, ms, ms * 1e-3 * clk / ((double)ITERS * 32 * wps));
    }
  }
  const int R = 19;
  struct C { const char* n; cfn f; const unsigned* p; unsigned gap2; } cs[] = {
    {"R=19 f16  add-clamp/max3/pk_add(sgpr)", k_cell<19, 0>, pin0, 0x90009000u /* -2/2048 */},
    {"R=19 f16m add-clamp/min3/add_u32(sgpr)", k_cell<19, 1>, pin1, 0x00020002u},
    {"R=19 f16m add-clamp/min3/add_u32(vgpr)", k_cell<19, 2>, pin1, 0x00020002u}};
  const int steps = 16384;
  double base4 = 0, best4 = 0;
  for (int wps : {2, 4, 6}) {
    printf("== cell loop, %d waves/SIMD\n", wps);
    for (auto& c : cs) {
      dim3 grid(ncu * wps), block(256);
      hipLaunchKernelGGL(c.f, grid, block, 0, 0, out, c.p, c.gap2, steps);
      hipDeviceSynchronize();
      hipEventRecord(e0);
      hipLaunchKernelGGL(c.f, grid, block, 0, 0, out, c.p, c.gap2, steps);
      hipEventRecord(e1); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1);
      const double cyc = ms * 1e-3 * clk / ((double)steps * R * wps);       // per register (cell pair) and lane
      printf("%-42s %8.3f ms  %.2f cycles/cell pair/lane\n", c.n, ms, cyc);
      if (wps == 4) { if (c.f == cs[0].f) base4 = cyc; else if (best4 == 0 || cyc < best4) best4 = cyc; }
    }
  }
  printf("gate at 4 waves/SIMD: best mirrored form %.2f vs %.2f cycles per cell pair: %.1f %% cheaper (needs >= 8 %%)\n",
         best4, base4, 100.0 * (1.0 - best4 / base4));
  return 0;
}
