// host_affine.h — affine-gap score, end cell and traceback.  Part of the single translation unit mi355_sw.hip
// (included there, in order; not a standalone header).  Four drivers:
//   affine_run    every query of the batch against ranges of the reference: affine_prof_run (sw_affine_prof_kernel, ranges of at most
//                 512 letters), affine_sweep (sw_affine_kernel) and the exact kernel behind both
//   affine_pairs  a list of (query, window) pairs, local or end-to-end (AffineCall::mode), with or without a diagonal band per pair:
//                 affine_pair_route sends each pair to affine_list_stage (sw_affine_pair_kernel, sw_affine_pair_e2e_kernel or
//                 sw_affine_band_kernel) or to the exact kernel (its E2E or BAND instance)
//   affine_extend the anchored seed extension of a list of (letters of a query, window) pairs, forward or backward: the same list
//                 stage on sw_affine_pair_ext_kernel, sw_affine_exact_ext_kernel and sw_affine_trace_ext_kernel behind it; with a
//                 diagonal band per pair: sw_affine_band_ext_kernel, sw_affine_exact_ext_band_kernel, sw_affine_trace_ext_band_kernel
//   affine_global the pairs of affine_extend anchored at both ends, plain and banded (the gap fill between two seeds of a chain): affine_extend's
//                 items and stages on sw_affine_pair_glob_kernel, sw_affine_band_glob_kernel and sw_affine_exact_glob_kernel, its
//                 traceback started at the corner
// The list kernels of the last three are seven names on two geometries (sw_affine_pair_kernel.h, sw_affine_band_kernel.h: one body per
// geometry, a name is an entry point that names its mode); affine_list_stage runs them through one family template per geometry,
// AffinePairFamily<M> and AffineBandFamily<M>, over a mode description M that holds what differs: the kernel instance of an R, the
// results per problem, the names, the op count and where an item comes from.
// All share one AffineCall (affine_begin .. affine_end, the latter with affine_trace: sw_affine_trace_kernel), affine_exact_stage
// (sw_affine_exact_kernel), affine_class_table, affine_download and affine_note_kernel.
namespace {

constexpr int64_t kAffineSweepMinCols = 1024;        // shorter references (ranges) are whole problems of the exact kernel
constexpr double kAffineExactCellsMax = 67108864.0;  // 2^26 cells: the largest whole problem one wavefront of the exact kernel takes
constexpr size_t kAffineTraceDirsMax = (size_t)1 << 30;   // decision bytes of one launch group of sw_affine_trace_kernel (ctx->dirs)
constexpr int kAffineF16Bound = 2040;                // smax * (rows + 1) and gap_open of the sweep's float16 cells (H / 2048)

// The scoring of one affine call over the reference's letters (any query byte against them, as plan_table)
struct AffineTable {
  std::vector<uint16_t> htab;     // [256][ncodes] float16 bits of s / 2048, scores below -2048 raised to it (the clamped
                                  // diagonal term is 0 either way: H <= 2040); pad column last
  int smax = 0, open = 0, ext = 0;
  int smin = 0;                   // the least substitution score (end-to-end mode: the low end of the diagonal term)
};

int affine_check(mi355_sw_ctx *ctx, const mi355_sw_affine_params *p) {
  if (!ctx) return MI355_SW_EINVAL;
  if (!p) return fail(ctx, MI355_SW_EINVAL, "params is NULL");
  if (!std::isfinite(p->gap_open) || !std::isfinite(p->gap_extend) || (!p->lut && (!std::isfinite(p->match) || !std::isfinite(p->mismatch))))
    return fail(ctx, MI355_SW_EINVAL, "affine scoring: a value is not finite");
  if (!(p->gap_extend > 0.0f)) return fail(ctx, MI355_SW_EINVAL, "affine scoring: gap_extend must be positive");
  if (p->gap_open < p->gap_extend) return fail(ctx, MI355_SW_EINVAL, "affine scoring: gap_open must be at least gap_extend");
  return 0;
}

// the score of byte a of x against the reference's letter with code c
inline float affine_score(const RefData &ref, const mi355_sw_affine_params &p, int a, int c) {
  return p.lut ? p.lut[(size_t)a * 256 + ref.byte_of[c]] : ((uint8_t)a == ref.byte_of[c] ? p.match : p.mismatch);
}

// the scoring as the exact and the traceback kernel take it: the 256 x 256 table, where there is one, goes to the device
int affine_scoring(mi355_sw_ctx *ctx, const mi355_sw_affine_params &p, AffineScoring &sc) {
  sc.lut = nullptr;
  if (p.lut) {
    if (ctx->lut.ensure(65536 * 4)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(scoring table) failed");
    HIPCHK(ctx, hipMemcpyAsync(ctx->lut.p, p.lut, 65536 * 4, hipMemcpyHostToDevice, ctx->stream));
    sc.lut = ctx->lut.as<float>();
  }
  sc.match = p.match; sc.mismatch = p.mismatch; sc.gap_open = p.gap_open; sc.gap_extend = p.gap_extend;
  return 0;
}

int affine_table(mi355_sw_ctx *ctx, const RefData &ref, const mi355_sw_affine_params &p, AffineTable &t) {
  const int nc = ref.ncodes;
  if (p.gap_open != std::floor(p.gap_open) || p.gap_extend != std::floor(p.gap_extend))
    return fail(ctx, MI355_SW_ENOTSUP, "affine scoring: gap costs must be integers");
  if (p.gap_open > 16777216.0f) return fail(ctx, MI355_SW_ENOTSUP, "affine scoring: gap_open beyond 2^24");
  t.open = (int)p.gap_open; t.ext = (int)p.gap_extend;
  t.htab.assign((size_t)256 * nc, half_bits(-8.0f));
  float smax = 0, smin = 0;
  for (int a = 0; a < 256; ++a)
    for (int c = 0; c < nc - 1; ++c) {
      const float s = affine_score(ref, p, a, c);
      if (!std::isfinite(s)) return fail(ctx, MI355_SW_EINVAL, "affine scoring: a table entry is not finite");
      if (s != std::floor(s)) return fail(ctx, MI355_SW_ENOTSUP, "affine scoring: substitution scores must be integers");
      if (std::fabs(s) > 1.0e6f) return fail(ctx, MI355_SW_ENOTSUP, "affine scoring: substitution score beyond +-10^6");
      smax = std::max(smax, s);
      smin = std::min(smin, s);
      t.htab[(size_t)a * nc + c] = half_bits(std::min(2048.0f, std::max(-2048.0f, s)) / kF16Scale);
    }
  t.smax = (int)smax;
  t.smin = (int)smin;
  return 0;
}

// AffineCall::mode of the extension calls: internal, beside the two public values (the public enum keeps its two members)
constexpr int kAffineModeExt = 2;

// One affine call, as every stage below takes it: where it runs, on what, its scoring and the table of that scoring
struct AffineCall {
  mi355_sw_ctx *ctx;
  const RefData &ref; const QueryBatch &q;   // the reference and the batch it runs on
  const mi355_sw_affine_params &p;
  AffineTable t;
  int mode = MI355_SW_AFFINE_LOCAL;          // pairs calls: MI355_SW_AFFINE_END_TO_END (no floor, row m wins; include/mi355_sw.h)
  bool e2e() const { return mode == MI355_SW_AFFINE_END_TO_END; }
  bool ext() const { return mode == kAffineModeExt; }              // the anchored model of the extension calls (affine_extend)
  float zdrop = INFINITY;                    // the extension calls' z-drop (include/mi355_sw.h "z-drop"); +inf: no stop rule
  bool zd() const { return zdrop < INFINITY; }
};

// End-to-end mode: are all values of a problem of m rows integers below 2^24 in magnitude (exact in float32, no bit reserved)?
// H >= -(o + (m-1) e) by the all-F path from the free row 0, so Ho, E, F >= -(2o + m e), E - e and F - e one e lower, and the
// diagonal term H + s >= -(o + (m-1) e) + smin; upwards H <= smax m.  (t.smin <= 0 <= t.smax.)
// The pair kernel also forms the table's s + o in [smin + o, smax + o] and the diagonal term as Ho + (s + o); one inequality covers
// its low side, 2o + (m+1) e - smin < 2^24.  The exact kernel forms neither: each of its values has its own inequality.
bool affine_e2e_exact(const AffineTable &t, double m) {
  const double low = 2.0 * t.open + (m + 1.0) * t.ext - t.smin, high = (double)t.smax * (m + 1.0) + t.open;
  return low < 16777216.0 && high < 16777216.0;
}
bool affine_e2e_whole_exact(const AffineTable &t, double m) {
  return 2.0 * t.open + (m + 1.0) * t.ext < 16777216.0 && t.open + m * t.ext - t.smin < 16777216.0 && (double)t.smax * (m + 1.0) < 16777216.0;
}

// Opens the call: fills c.t and starts the call's interval (ev[4]).  0: go on; 1: nothing to do, the caller's zeroed outputs
// stand; negative: the error.
int affine_begin(AffineCall &c) {
  { int rc = affine_table(c.ctx, c.ref, c.p, c.t); if (rc) return rc; }
  if (c.t.smax <= 0 && !c.e2e() && !c.ext()) return 1;             // no positive cell: every maximum is 0 (end-to-end, anchored: no floor)
  HIPCHK(c.ctx, hipEventRecord(c.ctx->ev[4], c.ctx->stream));
  return 0;
}

// One launch (the sweep: one bucket) of an affine score kernel over `cells` cells: counted in timings[5] and, where it is the
// largest of the call so far, described in last_kernel; `fmt` makes its name.
__attribute__((format(printf, 10, 11)))
void affine_note_kernel(mi355_sw_ctx *ctx, double cells, int cell, int lanes, int R, int64_t chunk_len, int64_t sub_len, int64_t warm,
                        double valu_ops_per_cell, const char *fmt, ...) {
  ctx->timings[5] += cells;
  if (!(cells > ctx->last_kernel.cells)) return;
  mi355_sw_kernel_info &ki = ctx->last_kernel;
  ki.cell = cell; ki.lanes = lanes; ki.rows_per_lane = R; ki.strips = 0; ki.twin = 0;
  ki.chunk_len = chunk_len; ki.sub_len = sub_len; ki.warm = warm; ki.cells = cells; ki.valu_ops_per_cell = valu_ops_per_cell;
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(ki.name, sizeof ki.name, fmt, ap);
  va_end(ap);
}

typedef void (*AffineKernel)(const ScoreArgs, const uint32_t, const uint32_t);
// the instance for a shape of pick_shape: every R of kR16 on 16 lanes, every R of kR8 on 8
AffineKernel affine_kernel(int SL, int R) {
  AffineKernel k = nullptr;
  if (SL == 8) with_listed_R<kR8>(R, [&](auto r) { k = &sw_affine_kernel<decltype(r)::value, 8>; });
  else with_listed_R<kR16>(R, [&](auto r) { k = &sw_affine_kernel<decltype(r)::value, 16>; });
  return k;
}

size_t affine_exact_lds(int m) { return (size_t)7 * (m + 2) * 4 + (size_t)m + 16; }
// the rows instance (sw_affine_exact_rows_band_kernel): the letters padded to a word, then a maximum and a column per row
constexpr size_t affine_exact_rows_lds(int m) { return (size_t)7 * (m + 2) * 4 + (((size_t)m + 3) & ~(size_t)3) + (size_t)8 * (m + 1) + 16; }
constexpr int kAffineExactRowsMax = 4398;    // its row limit (the other instances': 5600)
inline size_t affine_exact_lds(int m, bool rows) { return rows ? affine_exact_rows_lds(m) : affine_exact_lds(m); }
static_assert(affine_exact_rows_lds(kAffineExactRowsMax) <= kExactLdsMax && affine_exact_rows_lds(kAffineExactRowsMax + 1) > kExactLdsMax, "the bound the refusal names");

// A job of the exact kernel under a band, blo <= j - i <= bhi in its window's local coordinates: the BAND instance takes it.
struct ExactBandJob : ExactJob { int32_t blo = 0, bhi = 0; };

// The instance of the exact kernel for problems of either type: under a band, else by the call's mode.  (Plain overloads, the banded
// one first: kernels stand in the code object in the order of their first mention; inside a template, or reordered, they would move.)
inline auto affine_exact_instance(const AffineCall &, const ExactBandProblem *) { return &sw_affine_exact_kernel<false, true>; }
inline auto affine_exact_instance(const AffineCall &c, const ExactProblem *) { return c.e2e() ? &sw_affine_exact_kernel<true> : &sw_affine_exact_kernel<false>; }

// Runs jobs[lo, hi) on sw_affine_exact_kernel in one launch (ExactJob: q, ylo, nw, col_offset, own_lo, target -> best, ci, cj).
// Job: ExactJob, or ExactBandJob for the BAND instance, whose problem wraps the same ExactProblem (as affine_trace).
template <class Job>
int run_affine_exact(const AffineCall &c, std::vector<Job> &jobs, size_t lo, size_t hi) {
  constexpr bool BAND = std::is_same<Job, ExactBandJob>::value;
  typedef typename AffineExactProblemOf<BAND>::type Problem;
  mi355_sw_ctx *ctx = c.ctx; const RefData &ref = c.ref; const QueryBatch &q = c.q;
  const size_t n = hi - lo;
  if (n == 0) return 0;
  size_t lds = 0;
  for (size_t k = lo; k < hi; ++k) lds = std::max(lds, affine_exact_lds(q.len[jobs[k].q]));
  if (lds > kExactLdsMax) return fail(ctx, MI355_SW_ENOTSUP, "affine: query longer than the exact kernel's LDS diagonals hold");
  path_note(ctx, BAND ? "affine_exact_band" : "affine_exact");
  if (ctx->probs.ensure(n * sizeof(Problem)) || ctx->outs_f.ensure(n * 4) || ctx->outs_i.ensure(n * 16))
    return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(exact scratch) failed");
  std::vector<Problem> pr(n);
  for (size_t k = 0; k < n; ++k) {
    const Job &j = jobs[lo + k];
    ExactProblem *ep;
    if constexpr (BAND) { ep = &pr[k].e; pr[k].blo = j.blo; pr[k].bhi = j.bhi; } else ep = &pr[k];
    ExactProblem &e = *ep;
    e.x = q.bytes.as<uint8_t>() + q.off[j.q];
    e.y = ref.bytes.as<uint8_t>() + j.ylo;
    e.m = q.len[j.q];
    e.nw = j.nw;
    e.col_offset = j.col_offset;
    e.full_n = j.full_n;
    e.own_lo = j.own_lo;
    e.square_quirk = 0;
    e.target = j.target;
    e.dirs = nullptr;
    e.hout = nullptr;
    e.best = ctx->outs_f.as<float>() + k;
    e.cell = ctx->outs_i.as<int64_t>() + 2 * k;
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->probs.p, pr.data(), n * sizeof(Problem), hipMemcpyHostToDevice, ctx->stream));
  AffineScoring sc;
  { int rc = affine_scoring(ctx, c.p, sc); if (rc) return rc; }
  launch_dyn_lds(affine_exact_instance(c, pr.data()), dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->probs.as<Problem>(), sc);
  HIPCHK(ctx, hipGetLastError());
  ctx->exact_launches += 1;
  std::vector<float> bf(n);
  std::vector<int64_t> ci(2 * n);
  HIPCHK(ctx, hipMemcpyAsync(bf.data(), ctx->outs_f.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ci.data(), ctx->outs_i.p, n * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < n; ++k) { jobs[lo + k].best = bf[k]; jobs[lo + k].ci = ci[2 * k]; jobs[lo + k].cj = ci[2 * k + 1]; }
  return 0;
}

// Query q of the batch against the n columns from `lo` as a whole problem of the exact kernel, `index` the caller's range or pair.
// False where the kernel does not take it: too many cells, or scores beyond float32's integers (the caller words the refusal).
bool affine_whole_job(const AffineCall &c, int q, int64_t lo, int64_t n, size_t index, ExactJob &j) {
  const double m = (double)c.q.len[q];
  if (m * (double)n > kAffineExactCellsMax || (double)c.t.smax * (m + 1.0) >= 16777216.0) return false;
  if (c.e2e() && !affine_e2e_whole_exact(c.t, m)) return false;
  j.q = q; j.ylo = lo; j.nw = (int32_t)n; j.col_offset = 0; j.full_n = n; j.own_lo = 1; j.quirk = 0;
  j.target = -1.0f; j.want_dirs = false; j.index = index;
  return true;
}

// The exact kernel over all of `jobs` (ExactJob, or ExactBandJob: the BAND instance), 65536 per launch; its interval
// (ev[2]..ev[3]) goes to timings[1].
template <class Job>
int affine_exact_stage(const AffineCall &c, std::vector<Job> &jobs) {
  mi355_sw_ctx *ctx = c.ctx;
  if (jobs.empty()) return 0;
  HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
  for (size_t lo = 0; lo < jobs.size(); lo += 65536) {
    { int rc = run_affine_exact(c, jobs, lo, std::min(jobs.size(), lo + 65536)); if (rc) return rc; }
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
  ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  return 0;
}

// (best, cell) of the np problems launched since ev[0], from outs_f / outs_i through pin_out: closes the interval (ev[1]), copies,
// waits, adds the interval to timings[0].  h_best[np], h_cell[np][2]: views into pin_out.  `nomem`: the caller's ENOMEM message.
// tail_f: further bytes of outs_f behind the np results that ride with the same copy (the z-drop mode's row counter).
int affine_download(mi355_sw_ctx *ctx, size_t np, const char *nomem, const float *&h_best, const int64_t *&h_cell, size_t tail_f = 0) {
  HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
  const size_t o_cell = (np * 4 + tail_f + 15) & ~(size_t)15;
  if (ctx->pin_out.ensure(o_cell + np * 16)) return fail(ctx, MI355_SW_ENOMEM, nomem);
  uint8_t *pin = ctx->pin_out.as<uint8_t>();
  h_best = reinterpret_cast<const float *>(pin); h_cell = reinterpret_cast<const int64_t *>(pin + o_cell);
  HIPCHK(ctx, hipMemcpyAsync(pin, ctx->outs_f.p, np * 4 + tail_f, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(pin + o_cell, ctx->outs_i.p, np * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->timings[0] += elapsed_us(ctx, ctx->ev[0], ctx->ev[1]);
  return 0;
}

// One bucket of the batch on sw_affine_kernel over `ranges` (device copies in ctx->ranges, keys in ctx->keys).
int affine_sweep_launch(const AffineCall &c, const std::vector<Range> &ranges, Bucket &b) {
  mi355_sw_ctx *ctx = c.ctx; const RefData &ref = c.ref; const QueryBatch &q = c.q; const AffineTable &t = c.t;
  const size_t nr = ranges.size();
  int64_t maxlen = 0;
  double range_cols = 0;
  for (auto &r : ranges) { maxlen = std::max(maxlen, r.hi - r.lo); range_cols += (double)(r.hi - r.lo); }
  const size_t npairs = ((size_t)b.count + 1) / 2;
  b.sub_len = score_sub_len(MI355_SW_F32, b);
  b.chunk_len = pick_chunk_len(maxlen, npairs * nr, b.warm, b.SL, false, b.maxlen, b.sub_len, b.sub_len);
  if (b.sub_len > b.chunk_len || b.chunk_len % b.sub_len != 0) b.sub_len = b.chunk_len;
  const int64_t cpr = (maxlen + b.chunk_len - 1) / b.chunk_len;
  const int nslot = 256 / b.SL;
  const int64_t cgroups = (cpr + nslot - 1) / nslot;
  if ((double)npairs * (double)cgroups > 2.0e9) return fail(ctx, MI355_SW_ENOTSUP, "affine: grid too large");
  AffineKernel kern = affine_kernel(b.SL, b.R);
  if (!kern) return fail(ctx, MI355_SW_ENOTSUP, "affine: no sweep kernel instance for this tile shape");

  ScoreArgs a;
  memset(&a, 0, sizeof a);
  a.refcodes = ref.codes.as<uint8_t>();
  a.ref_len = (int64_t)ref.n;
  a.range_lo = ctx->ranges.as<int64_t>();
  a.range_hi = ctx->ranges.as<int64_t>() + nr;
  a.chunk_len = b.chunk_len;
  a.sub_len = b.sub_len;
  a.warm = (cpr == 1) ? 0 : b.warm;              // a single tile per range starts at the range's own border
  a.chunks_per_range = (int)cpr;
  a.qbytes = q.bytes.as<uint8_t>();
  a.qoff = q.offs.as<int64_t>();
  a.qlen = q.lens.as<int32_t>();
  a.qsel = q.sel.as<int32_t>();
  a.nq = (int)q.nq;
  a.stab = ctx->atab.p;
  a.ncodes = ref.ncodes;
  a.keys = ctx->keys.as<unsigned long long>();
  const uint32_t nopen2 = (uint32_t)half_bits(-(float)t.open / kF16Scale) * 0x00010001u;
  const uint32_t next2 = (uint32_t)half_bits(-(float)t.ext / kF16Scale) * 0x00010001u;
  const size_t shmem = profile_lds_bytes(ref.ncodes, b.R, b.SL) + (size_t)nslot * codebuf_bytes(b.SL);
  // keep single launches to a few seconds: split the bucket's pairs over several launches
  const double cells_per_pair = 2.0 * std::max(1, b.maxlen) * std::max(1.0, range_cols);
  const size_t pairs_per_launch = (size_t)std::max(1.0, std::min((double)npairs, 2.0e13 / cells_per_pair));
  for (size_t p0 = 0; p0 < npairs; p0 += pairs_per_launch) {
    const size_t pn = std::min(pairs_per_launch, npairs - p0);
    a.qfirst = b.first + (int)(p0 * 2);
    a.qcount = std::min(b.count - (int)(p0 * 2), (int)(pn * 2));
    launch_dyn_lds(kern, dim3((unsigned)(pn * cgroups), (unsigned)nr), dim3(256), shmem, ctx->stream, a, nopen2, next2);
    HIPCHK(ctx, hipGetLastError());
    ctx->timings[4] += 1;
  }
  path_note(ctx, "affine[cell=f16,SL=%d,R=%d]", b.SL, b.R);
  double cells = 0;
  for (int k = 0; k < b.count; ++k) cells += (double)q.len[q.order[b.first + k]] * range_cols;
  // as valu_ops_per_cell (host_score.h): per step seven ops per row and a maximum3 per two rows, the overhead of the linear
  // sweep (DPP move, profile address, code extract; border mask on 8-lane tiles) and F's DPP move (8 lanes: and its and-or),
  // over the two cells of a register
  affine_note_kernel(ctx, cells, MI355_SW_CELL_F16, b.SL, b.R, b.chunk_len, b.sub_len, a.warm,
                     (7.0 * b.R + (b.R + 1) / 2 + (b.SL == 8 ? 6.0 : 4.0)) / (2.0 * b.R), "sw_affine_kernel<R=%d, f16x2, SL=%d>", b.R, b.SL);
  return 0;
}

// ---- sw_affine_prof_kernel (sw_affine_prof_kernel.h): ranges of at most kWaveMaxLanesSide columns ----------------------------
constexpr double kAffineProfBound = 262144.0;        // 2^18: smax * (columns + 1) and gap_open, so that the key's five mantissa bits stay free
constexpr size_t kAffineProfLdsMax = 96 * 1024;      // the profile budget of wave_prof_ok
constexpr double kAffineProfMinCells = 262144.0;     // 2^18: a range whose problems hold fewer cells in all stays on the exact kernel, as before
constexpr size_t kAffineProfGroupProblems = (size_t)1 << 22;   // problems between two downloads of (best, cell)

// The classes of x's bytes: bytes with identical score rows against the reference's letters share a profile row.
struct AffineProfPlan {
  bool ok = false;
  int nclass = 0;                 // incl. the last one, "outside" (steps in front of and beyond a stream)
  uint8_t cls[256];
  std::vector<int> rep;           // a byte of every class but the last
};

// the classes alone (sw_affine_prof_kernel and sw_affine_pair_kernel)
// (open_bound: the key's five bits need gap_open < 2^18; the end-to-end pair instance has no key: affine_e2e_exact bounds gap_open)
void affine_byte_classes(const RefData &ref, const mi355_sw_affine_params &p, const AffineTable &t, AffineProfPlan &plan,
                         double open_bound = kAffineProfBound) {
  plan.ok = false;
  const int nl = ref.ncodes - 1;
  if (nl < 1 || nl > 255 || (double)t.open >= open_bound) return;
  plan.rep.clear();
  for (int a = 0; a < 256; ++a) {
    int c = 0;
    for (; c < (int)plan.rep.size(); ++c) {
      bool same = true;
      for (int l = 0; l < nl && same; ++l) same = affine_score(ref, p, a, l) == affine_score(ref, p, plan.rep[c], l);
      if (same) break;
    }
    if (c == (int)plan.rep.size()) {
      if (c == 255) return;                                        // (256 classes with "outside": the window holds bytes)
      plan.rep.push_back(a);
    }
    plan.cls[a] = (uint8_t)c;
  }
  plan.nclass = (int)plan.rep.size() + 1;
  plan.ok = true;
}

void affine_prof_plan(const RefData &ref, const mi355_sw_affine_params &p, const AffineTable &t, AffineProfPlan &plan) {
  plan.ok = false;
  if (!opt().no_affine_prof) affine_byte_classes(ref, p, t, plan);
}

bool affine_prof_range_ok(const AffineProfPlan &plan, const AffineTable &t, int64_t n) {
  if (!plan.ok || n < 1 || n > kWaveMaxLanesSide) return false;
  if ((double)t.smax * ((double)n + 1.0) >= kAffineProfBound) return false;
  return wave_prof_lds(plan.nclass, wave_prof_R((int)n)) <= kAffineProfLdsMax;
}

// The class table of sw_affine_prof_kernel / sw_affine_pair_kernel for cells of at most `side` + 1 steps of smax, built and sent to
// ctx->aprof: tab_floats floats, (s + o) 2^-k of class cl against letter l at [cl * cstride + l * lstride] and kPadScoreF elsewhere,
// then plan.cls.  Sets `tab` and sa's cls, open_s, ext_s, unscale.  `nomem`: the caller's ENOMEM message.
// (End-to-end mode has no clamp, so the scale decides nothing there: a power of two moves no mantissa bit.  It stays the same one.)
template <class Args>
int affine_class_table(const AffineCall &c, const AffineProfPlan &plan, int64_t side, size_t tab_floats, size_t cstride, size_t lstride,
                       const char *nomem, const float *&tab, Args &sa) {
  mi355_sw_ctx *ctx = c.ctx;
  // cells hold H * 2^-k, 2^k above every value of the call (as wave_prof_launch)
  const int k = std::max(1, std::ilogb((double)c.t.smax * ((double)side + 1.0) + 1.0) + 2);
  ctx->h_aprof.assign(tab_floats + 64, kPadScoreF);                // (outlives the asynchronous copy)
  for (int cl = 0; cl + 1 < plan.nclass; ++cl)
    for (int l = 0; l < c.ref.ncodes - 1; ++l)
      ctx->h_aprof[cl * cstride + l * lstride] = std::ldexp(affine_score(c.ref, c.p, plan.rep[cl], l) + (float)c.t.open, -k);
  memcpy(ctx->h_aprof.data() + tab_floats, plan.cls, 256);
  if (ctx->aprof.ensure((tab_floats + 64) * 4)) return fail(ctx, MI355_SW_ENOMEM, nomem);
  HIPCHK(ctx, hipMemcpyAsync(ctx->aprof.p, ctx->h_aprof.data(), (tab_floats + 64) * 4, hipMemcpyHostToDevice, ctx->stream));
  tab = ctx->aprof.as<float>();
  sa.cls = reinterpret_cast<const uint8_t *>(ctx->aprof.as<float>() + tab_floats);
  sa.open_s = std::ldexp((float)c.t.open, -k); sa.ext_s = std::ldexp((float)c.t.ext, -k); sa.unscale = std::ldexp(1.0f, k);
  return 0;
}

// Every non-empty query of the batch against each range of `which` (indices into `ranges`, all affine_prof_range_ok): one launch
// of sw_affine_prof_kernel per range over descriptors that batch_wave_setup builds on the device, longest sequence first; (best,
// cell) of a group of ranges come down in one copy.  maxima / ends as affine_run.
int affine_prof_run(const AffineCall &c, const std::vector<Range> &ranges, const std::vector<size_t> &which, const AffineProfPlan &plan,
                    float *maxima, int64_t *ends) {
  mi355_sw_ctx *ctx = c.ctx; const RefData &ref = c.ref; const QueryBatch &q = c.q;
  const size_t nq = q.nq;
  size_t first = 0;
  while (first < nq && q.len[q.order[first]] < 1) ++first;          // (sorted by length: the empty queries lead)
  const size_t count = nq - first;
  if (count == 0 || which.empty()) return 0;
  if (count > ((size_t)1 << 30)) return fail(ctx, MI355_SW_ENOTSUP, "affine: more than 2^30 queries");
  int64_t nmax = 0;
  for (size_t r : which) nmax = std::max(nmax, ranges[r].hi - ranges[r].lo);
  const int nl = ref.ncodes - 1;
  // class scores and the byte -> class table: [nclass][nl] floats, then 256 bytes
  AffineProfArgs sa;
  sa.nclass = plan.nclass; sa.nletters = nl;
  int rc = affine_class_table(c, plan, nmax, (size_t)plan.nclass * nl, nl, 1, "hipMalloc(affine profile classes) failed", sa.ctab, sa);
  if (rc) return rc;

  const size_t per_group = std::max<size_t>(1, kAffineProfGroupProblems / count);
  const unsigned blocks = (unsigned)((count + 15) / 16);
  double row_sum = 0;
  for (size_t s = first; s < nq; ++s) row_sum += (double)q.len[q.order[s]];
  for (size_t g0 = 0; g0 < which.size(); g0 += per_group) {
    const size_t ng = std::min(per_group, which.size() - g0), np = ng * count;
    const char *nomem = "affine: allocation of the batch scratch failed";
    if (ctx->wprobs.ensure(np * sizeof(WaveProblem)) || ctx->outs_f.ensure(np * 4 + 64) || ctx->outs_i.ensure(np * 16))
      return fail(ctx, MI355_SW_ENOMEM, nomem);
    BatchWaveArgs a;
    memset(&a, 0, sizeof a);
    a.qbytes = q.bytes.as<uint8_t>(); a.qoff = q.offs.as<int64_t>(); a.qlen = q.lens.as<int32_t>();
    a.qsel = q.sel.as<int32_t>(); a.qcum = q.cum.as<int64_t>();
    a.first = (int)first; a.count = (int)count; a.orient = 1; a.W = 1;
    for (size_t g = 0; g < ng; ++g) {                               // the descriptors: lanes = the CODES of the range, stream = x
      const Range &rg = ranges[which[g0 + g]];
      a.ref = ref.codes.as<uint8_t>() + rg.lo; a.nref = rg.hi - rg.lo;
      a.R = wave_prof_R((int)a.nref);
      a.probs = ctx->wprobs.as<WaveProblem>() + g * count;
      a.best = ctx->outs_f.as<float>() + g * count;
      a.cell = ctx->outs_i.as<int64_t>() + 2 * g * count;
      hipLaunchKernelGGL(batch_wave_setup, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (size_t g = 0; g < ng; ++g) {
      const Range &rg = ranges[which[g0 + g]];
      const int n = (int)(rg.hi - rg.lo), R = wave_prof_R(n);
      const WaveProblem *dp = ctx->wprobs.as<WaveProblem>() + g * count;
      with_wave_R(R, [&](auto r) {
        launch_dyn_lds(&sw_affine_prof_kernel<decltype(r)::value>, dim3(blocks), dim3(256), wave_prof_lds(plan.nclass, R), ctx->stream, dp, (int)count, sa);
      });
      HIPCHK(ctx, hipGetLastError());
      path_note(ctx, "affine_prof[R=%d]", R);
      ctx->timings[4] += 1;
      // per step and lane: seven ops and the key's v_or per cell, a maximum3 per two cells for the lane's best key, and seven of
      // overhead (two DPP moves, the profile address: multiply-add and shift, and compare, select, maximum for the first row)
      affine_note_kernel(ctx, row_sum * (double)n, MI355_SW_CELL_F32, 16, R, n, n, 0, (8.0 * R + (R + 1) / 2 + 7.0) / (double)R,
                         "sw_affine_prof_kernel<R=%d, f32>", R);
    }
    const float *h_best = nullptr; const int64_t *h_cell = nullptr;
    rc = affine_download(ctx, np, nomem, h_best, h_cell); if (rc) return rc;
    for (size_t g = 0; g < ng; ++g) {
      const size_t r = which[g0 + g];
      for (size_t kk = 0; kk < count; ++kk) {
        const int id = q.order[batch_sorted_pos((int)first, (int)count, (int)kk)];
        const float best = h_best[g * count + kk];
        maxima[r * nq + (size_t)id] = best > 0 ? best : 0.0f;
        if (ends && best > 0) { ends[2 * id] = h_cell[2 * (g * count + kk)]; ends[2 * id + 1] = h_cell[2 * (g * count + kk) + 1]; }
      }
    }
  }
  return 0;
}

// One alignment to trace back: query q of the batch against the range of the reference that starts at column lo, with the score
// and the end cell (row, column relative to lo, 1-based) its score pass found.
// banded: the alignment lies inside blo <= j - i <= bhi of the pair's own coordinates (the window of the traceback gets it shifted).
struct AffineTraceItem { int q; int64_t lo; float score; int64_t ex, ey; bool banded = false; int64_t blo = 0, bhi = 0; };

// Traceback of every item with a positive score: one sw_affine_trace_kernel problem per item over the window behind the end
// cell — the L17 window of columns and the L18 window of rows, each where it is shorter than the matrix, clamped
// at the item's own left border and at row 1 — in launch groups of at most kAffineTraceDirsMax decision bytes.
// tout[items.size()]: views into ctx->arenas.
// BAND: the banded items on the BAND instance of the kernel, the others on today's — one pass each (affine_end).  A banded alignment
// is an alignment, so the windows of L17 and L18 hold every banded path of value `score` into the end cell as well; the window's band
// is the pair's, shifted: delta_local = delta - wl + row_lo.
template <bool BAND = false>
int affine_trace(const AffineCall &c, const std::vector<AffineTraceItem> &items, std::vector<TraceOut> &tout) {
  mi355_sw_ctx *ctx = c.ctx; const RefData &ref = c.ref; const QueryBatch &q = c.q; const AffineTable &t = c.t;
  typedef typename AffineTraceProblemOf<BAND>::type Problem;
  struct Job { size_t item; int32_t m, nw; int64_t wl, row_lo; bool clamped, row_clamped; size_t dirs_off, cons_off; };
  std::vector<Job> jobs;
  for (size_t k = 0; k < items.size(); ++k) {
    if (items[k].banded != BAND) continue;
    const float score = items[k].score;
    const int64_t ex = items[k].ex, ey = items[k].ey;
    // end-to-end: every pair with an end cell (a non-empty query and window), whatever the sign of its score
    if (c.e2e() ? ex < 1 || ey < 1 : !(score > 0)) continue;
    const double spare = std::max(0.0, (double)t.smax * (double)ex - (double)score);   // (t.smax is max(smax, 0))
    const double W = (double)ex + std::ceil(spare / (double)t.ext) + 2.0;
    // lemma L18, the mirror image of L17: at most end_y diagonal or horizontal steps, hence at most (smax end_y - score) / e rows of gaps
    const double spare_r = std::max(0.0, (double)t.smax * (double)ey - (double)score);
    const double Wr = (double)ey + std::ceil(spare_r / (double)t.ext) + 2.0;
    Job j;
    j.item = k;
    j.row_clamped = c.e2e() || Wr >= (double)ex;                    // end-to-end (L19): all m rows belong to the alignment, no row window
    const int64_t mw = j.row_clamped ? ex : (int64_t)Wr;
    j.row_lo = ex - mw;
    j.clamped = W >= (double)ey;
    const int64_t nw = j.clamped ? ey : (int64_t)W;
    if (nw > (int64_t)kAffineTraceDirsMax || mw > (int64_t)kAffineTraceDirsMax || dirs_bytes(mw, nw) > kAffineTraceDirsMax) {
      char msg[200];
      std::snprintf(msg, sizeof msg, "affine traceback: a window of %lld rows x %lld columns needs more than %zu decision bytes",
                    (long long)mw, (long long)nw, kAffineTraceDirsMax);
      return fail(ctx, MI355_SW_ENOTSUP, msg);
    }
    j.m = (int32_t)mw;
    j.nw = (int32_t)nw;
    j.wl = ey - nw;
    j.dirs_off = j.cons_off = 0;
    if (affine_exact_lds(j.m) > kExactLdsMax) {
      char msg[200];
      std::snprintf(msg, sizeof msg, "affine traceback: a window of %lld rows x %lld columns has more rows than the exact kernel's LDS diagonals hold",
                    (long long)mw, (long long)nw);
      return fail(ctx, MI355_SW_ENOTSUP, msg);
    }
    jobs.push_back(j);
  }
  if (jobs.empty()) return 0;
  path_note(ctx, "affine_trace");
  AffineScoring sc;
  { int rc = affine_scoring(ctx, c.p, sc); if (rc) return rc; }
  for (size_t lo = 0; lo < jobs.size();) {
    size_t hi = lo, dirs_total = 0, cons_total = 0, lds = 0;
    while (hi < jobs.size() && hi - lo < 65536) {
      Job &j = jobs[hi];
      const size_t db = (dirs_bytes(j.m, j.nw) + 15) & ~(size_t)15;
      if (hi > lo && dirs_total + db > kAffineTraceDirsMax) break;
      j.dirs_off = dirs_total; dirs_total += db;
      j.cons_off = cons_total; cons_total += 2 * ((size_t)j.m + (size_t)j.nw);
      lds = std::max(lds, affine_exact_lds(j.m));
      ++hi;
    }
    const size_t n = hi - lo;
    if (ctx->wprobs.ensure(n * sizeof(Problem)) || ctx->walkp.ensure(n * 24) || ctx->dirs.ensure(dirs_total) ||
        ctx->cons.ensure(cons_total + 16))
      return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(affine traceback scratch) failed");
    std::vector<Problem> pr(n);
    for (size_t k = 0; k < n; ++k) {
      const Job &j = jobs[lo + k];
      memset(&pr[k], 0, sizeof pr[k]);
      AffineTraceProblem *ap;
      if constexpr (BAND) {
        ap = &pr[k].t;
        // (a window lies within 2^30 rows and columns of its end cell: the clamps keep the shifted band in int32 and lose nothing)
        const int64_t shift = j.row_lo - j.wl, big = (int64_t)1 << 30;
        pr[k].blo = (int32_t)std::max(-big, std::min(big, items[j.item].blo + shift));
        pr[k].bhi = (int32_t)std::max(-big, std::min(big, items[j.item].bhi + shift));
      } else ap = &pr[k];
      AffineTraceProblem &a = *ap;
      a.e.x = q.bytes.as<uint8_t>() + q.off[items[j.item].q] + j.row_lo;
      a.e.y = ref.bytes.as<uint8_t>() + items[j.item].lo + j.wl;
      a.e.m = j.m; a.e.nw = j.nw;
      a.e.col_offset = j.wl;
      a.e.own_lo = 1;
      a.e.target = items[j.item].score;
      a.e.dirs = ctx->dirs.as<uint8_t>() + j.dirs_off;
      a.cap = j.m + j.nw;
      a.cons_x = ctx->cons.as<char>() + j.cons_off;
      a.cons_y = a.cons_x + a.cap;
      a.clamped = j.clamped ? 1 : 0;
      a.row_clamped = j.row_clamped ? 1 : 0;
      a.out = ctx->walkp.as<int64_t>() + 3 * k;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->wprobs.p, pr.data(), n * sizeof(Problem), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[6], ctx->stream));
    void (*kern)(const Problem *, const AffineScoring);               // the instance: under a band, else by the call's mode
    if constexpr (BAND) kern = &sw_affine_trace_kernel<false, true>;
    else kern = c.e2e() ? &sw_affine_trace_kernel<true> : &sw_affine_trace_kernel<false>;
    launch_dyn_lds(kern, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->wprobs.as<Problem>(), sc);
    HIPCHK(ctx, hipGetLastError());
    ctx->trace_launches += 1;
    HIPCHK(ctx, hipEventRecord(ctx->ev[7], ctx->stream));
    std::vector<int64_t> wo(3 * n);
    std::vector<char> cons(cons_total);
    HIPCHK(ctx, hipMemcpyAsync(wo.data(), ctx->walkp.p, n * 24, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cons.data(), ctx->cons.p, cons_total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timings[2] += elapsed_us(ctx, ctx->ev[6], ctx->ev[7]);
    ctx->arenas.push_back(std::move(cons));
    const char *base = ctx->arenas.back().data();
    for (size_t k = 0; k < n; ++k) {
      const Job &j = jobs[lo + k];
      const int64_t len = wo[3 * k], st = wo[3 * k + 2];
      if (st == 1) return fail(ctx, MI355_SW_ENODEV, "internal: the affine traceback left its window (lemmas L17, L18)");
      if (st == 2) return fail(ctx, MI355_SW_ENODEV, "internal: the affine traceback exceeded its string capacity");
      if (st != 0) return fail(ctx, MI355_SW_ENODEV, "internal: the end cell of the affine traceback window does not hold the score");
      TraceOut &o = tout[j.item];
      o.len = (size_t)len;
      o.cx = base + j.cons_off;
      o.cy = base + j.cons_off + (size_t)j.m + (size_t)j.nw;
      o.pos = (uint32_t)wo[3 * k + 1];
    }
    lo = hi;
  }
  return 0;
}

// Closes the call: the traceback of `items` (tout may be null: none), whose scores and end cells are score[k] and ends[k][2], then
// the end of the call's interval (ev[5]), which goes to timings[3].
int affine_end(const AffineCall &c, std::vector<AffineTraceItem> &items, const float *score, const int64_t *ends, std::vector<TraceOut> *tout) {
  if (tout) {
    for (size_t k = 0; k < items.size(); ++k) { items[k].score = score[k]; items[k].ex = ends[2 * k]; items[k].ey = ends[2 * k + 1]; }
    { int rc = affine_trace(c, items, *tout); if (rc) return rc; }
    bool any_banded = false;
    for (const AffineTraceItem &it : items) any_banded |= it.banded;
    if (any_banded) { int rc = affine_trace<true>(c, items, *tout); if (rc) return rc; }
  }
  HIPCHK(c.ctx, hipEventRecord(c.ctx->ev[5], c.ctx->stream));
  c.ctx->timings[3] += elapsed_us(c.ctx, c.ctx->ev[4], c.ctx->ev[5]);
  return 0;
}

// The sweep's buckets: the non-empty queries of at most 512 rows by tile shape, and for each whether its float16 cells hold the
// call (fast).  qfast[id] = 1 for the queries of the fast ones; why_slow: what keeps a query or a bucket out, for the refusal.
std::vector<Bucket> affine_sweep_buckets(const AffineCall &c, const Margin &mg, std::vector<char> &qfast, std::string &why_slow) {
  const QueryBatch &q = c.q; const AffineTable &t = c.t;
  std::vector<Bucket> buckets;
  for (size_t pos = 0; pos < q.nq; ++pos) {
    const int len = q.len[q.order[pos]];
    if (len < 1) continue;
    if (len > kMaxRowsFast) { why_slow = "query longer than 512 rows"; break; }   // (sorted by length: all further ones too)
    int SL = 16, R = 2;
    pick_shape(len, SL, R);
    if (buckets.empty() || buckets.back().R != R || buckets.back().SL != SL) {
      Bucket b;
      b.first = (int)pos; b.R = R; b.SL = SL; b.sem = kSemF16;
      buckets.push_back(b);
    }
    buckets.back().count++;
    buckets.back().maxlen = std::max(buckets.back().maxlen, len);
  }
  for (Bucket &b : buckets) {
    b.warm = std::min(kColsMax, (mg.cols(b.maxlen) + 63) / 64 * 64);
    char msg[160];
    msg[0] = 0;
    if ((int64_t)t.smax * (b.maxlen + 1) > kAffineF16Bound)
      std::snprintf(msg, sizeof msg, "smax * (rows + 1) = %lld exceeds %d", (long long)t.smax * (b.maxlen + 1), kAffineF16Bound);
    else if (t.open > kAffineF16Bound) std::snprintf(msg, sizeof msg, "gap_open = %d exceeds %d", t.open, kAffineF16Bound);
    else if (profile_lds_bytes(c.ref.ncodes, b.R, b.SL) > kProfileLdsMax || c.ref.ncodes > 256)
      std::snprintf(msg, sizeof msg, "%d reference letters: the query profile of %d rows per lane does not fit LDS", c.ref.ncodes - 1, b.R);
    b.fast = msg[0] == 0;
    if (!b.fast) why_slow = msg;
    if (b.fast) for (int k = 0; k < b.count; ++k) qfast[q.order[b.first + k]] = 1;
  }
  return buckets;
}

// The sweep over `sweep_ranges` (indices into `ranges`), 32768 ranges per launch group: the maxima of the fast queries, and with
// want_ends (one range) their end-cell windows behind `jobs`.
int affine_sweep(const AffineCall &c, const std::vector<Range> &ranges, const std::vector<size_t> &sweep_ranges, std::vector<Bucket> &buckets,
                 const std::vector<char> &qfast, const Margin &mg, float *maxima, bool want_ends, std::vector<ExactJob> &jobs) {
  mi355_sw_ctx *ctx = c.ctx; const QueryBatch &q = c.q; const size_t nq = q.nq;
  bool any_fast = false;
  for (const Bucket &b : buckets) any_fast |= b.fast;
  if (!any_fast) return 0;
  if (ctx->atab.ensure(c.t.htab.size() * 2 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(affine score table) failed");
  ctx->h_atab = c.t.htab;                                          // (outlives the asynchronous copy)
  HIPCHK(ctx, hipMemcpyAsync(ctx->atab.p, ctx->h_atab.data(), ctx->h_atab.size() * 2, hipMemcpyHostToDevice, ctx->stream));
  for (size_t g0 = 0; g0 < sweep_ranges.size(); g0 += 32768) {
    const size_t g1 = std::min(sweep_ranges.size(), g0 + 32768), ng = g1 - g0;
    std::vector<Range> sub(ng);
    std::vector<int64_t> &rl = ctx->h_ranges;
    rl.resize(2 * ng);
    for (size_t k = 0; k < ng; ++k) { sub[k] = ranges[sweep_ranges[g0 + k]]; rl[k] = sub[k].lo; rl[ng + k] = sub[k].hi; }
    if (ctx->ranges.ensure(rl.size() * 8) || ctx->keys.ensure(nq * ng * 8)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
    HIPCHK(ctx, hipMemcpyAsync(ctx->ranges.p, rl.data(), rl.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->keys.p, 0, nq * ng * 8, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (Bucket &b : buckets) {
      if (!b.fast) continue;
      int rc = affine_sweep_launch(c, sub, b);
      if (rc) return rc;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    std::vector<unsigned long long> keys(nq * ng);
    HIPCHK(ctx, hipMemcpyAsync(keys.data(), ctx->keys.p, keys.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timings[0] += elapsed_us(ctx, ctx->ev[0], ctx->ev[1]);
    for (size_t k = 0; k < ng; ++k)
      for (size_t i = 0; i < nq; ++i)
        if (qfast[i]) maxima[sweep_ranges[g0 + k] * nq + i] = key_score(kKeyF16, (uint32_t)(keys[k * nq + i] >> 32), 0);
    if (!want_ends) continue;
    // (one range.)  The end cell: the first sub-chunk that reached the maximum holds the first maximum in column-major order —
    // or the up to SL - 1 trailing columns of the sub-chunk before it, reported with it — so one window per query, as the
    // linear float engine's locate_fast.  Only cells equal to the maximum compete: lemma L3 with g := gap_extend.
    const int64_t n = ranges[0].hi - ranges[0].lo;
    for (const Bucket &b : buckets) {
      if (!b.fast) continue;
      for (int k = 0; k < b.count; ++k) {
        const int id = q.order[b.first + k];
        const float score = maxima[id];
        if (!(score > 0)) continue;
        const int64_t first = (int64_t)(0xFFFFFFFFull - (keys[id] & 0xFFFFFFFFull));
        const double spare = std::max(0.0, mg.smax * (double)q.len[id] - (double)score);
        const int64_t warm = std::min<int64_t>(b.warm, clamp_cols((double)q.len[id] + std::ceil(spare / mg.g) + 2.0));
        const int64_t own_lo = std::max<int64_t>(0, first * b.sub_len - 63), own_hi = std::min((first + 1) * b.sub_len, n);
        const int64_t wl = std::max<int64_t>(0, own_lo - warm);
        ExactJob j;
        j.q = id; j.ylo = ranges[0].lo + wl; j.nw = (int32_t)(own_hi - wl); j.col_offset = wl; j.full_n = n;
        j.own_lo = (int32_t)(own_lo - wl + 1); j.quirk = 0; j.target = score; j.want_dirs = false;
        jobs.push_back(j);
      }
    }
  }
  return 0;
}

// Affine score (and, for one range, end cell) of every query of `q` over each range of `ref`, each range an independent
// problem.  maxima: [nranges][nq].  ends (may be null; one range only): [nq][2] = row, column relative to the range start.
// tout (may be null; needs ends): the traceback of every query, [nq] (affine_trace).
int affine_run(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const std::vector<Range> &ranges,
               const mi355_sw_affine_params &p, float *maxima, int64_t *ends, std::vector<TraceOut> *tout = nullptr) {
  const size_t nq = q.nq, nr = ranges.size();
  if (nq == 0 || nr == 0) return 0;
  for (size_t k = 0; k < nq * nr; ++k) maxima[k] = 0.0f;
  if (ends) for (size_t k = 0; k < 2 * nq; ++k) ends[k] = 0;
  if (tout) tout->assign(nq, TraceOut());
  AffineCall c{ctx, ref, q, p, AffineTable()};
  int rc = affine_begin(c);
  if (rc) return rc > 0 ? 0 : rc;
  const Margin mg = make_margin((double)c.t.smax, (double)c.t.ext, true, 0.0);   // lemma L15: L1-L4 with g := gap_extend

  // ---- ranges of at most 512 columns: every non-empty query is a problem of sw_affine_prof_kernel, whatever its length ---------
  // (a range whose problems hold fewer than kAffineProfMinCells cells in all, every one within the exact kernel's LDS, is so
  // little work that it stays where it was: one launch of the exact kernel)
  std::vector<char> rprof(nr, 0);
  std::vector<size_t> prof_ranges;
  AffineProfPlan plan;
  bool any_short = false;
  for (size_t r = 0; r < nr; ++r) any_short |= ranges[r].hi - ranges[r].lo >= 1 && ranges[r].hi - ranges[r].lo <= kWaveMaxLanesSide;
  if (any_short) affine_prof_plan(ref, p, c.t, plan);
  double batch_rows = 0;
  for (size_t k = 0; k < nq; ++k) batch_rows += (double)q.len[k];
  const bool exact_holds_all = affine_exact_lds(q.maxlen) <= kExactLdsMax;
  for (size_t r = 0; r < nr; ++r) {
    const int64_t n = ranges[r].hi - ranges[r].lo;
    if (!affine_prof_range_ok(plan, c.t, n) || (exact_holds_all && batch_rows * (double)n < kAffineProfMinCells)) continue;
    rprof[r] = 1; prof_ranges.push_back(r);
  }
  if (!prof_ranges.empty()) { rc = affine_prof_run(c, ranges, prof_ranges, plan, maxima, ends); if (rc) return rc; }

  // ---- which (query, range) the sweep takes -----------------------------------------------------------------------------
  std::vector<char> rsweep(nr, 0), qfast(nq, 0);
  std::vector<size_t> sweep_ranges;
  for (size_t r = 0; r < nr; ++r)
    if (!opt().no_affine_sweep && ranges[r].hi - ranges[r].lo >= kAffineSweepMinCols) { rsweep[r] = 1; sweep_ranges.push_back(r); }
  std::vector<Bucket> buckets; std::string why_slow;
  if (!sweep_ranges.empty()) buckets = affine_sweep_buckets(c, mg, qfast, why_slow);

  // ---- whole problems of the exact kernel: everything the sweep does not take (ExactJob::index: the range) --------------------
  std::vector<ExactJob> jobs;
  for (size_t r = 0; r < nr; ++r) {
    const int64_t n = ranges[r].hi - ranges[r].lo;
    for (size_t k = 0; k < nq; ++k) {
      if (rprof[r] || (rsweep[r] && qfast[k]) || q.len[k] < 1 || n < 1) continue;
      ExactJob j;
      if (!affine_whole_job(c, (int)k, ranges[r].lo, n, r, j)) {
        if (opt().no_affine_sweep) return fail(ctx, MI355_SW_ENOTSUP, "affine, option no_affine_sweep: a problem of more than 2^26 cells");
        return fail(ctx, MI355_SW_ENOTSUP, "affine: " + (why_slow.empty() ? std::string("problem outside the sweep") : why_slow) +
                                               " (beyond the sweep's float16 cells), and more than 2^26 cells for the exact kernel");
      }
      jobs.push_back(j);
    }
  }
  const size_t nwhole = jobs.size();

  // ---- the sweep with its end-cell windows, then the exact kernel: whole problems and end-cell windows ------------------------
  rc = affine_sweep(c, ranges, sweep_ranges, buckets, qfast, mg, maxima, ends != nullptr, jobs);
  if (!rc) rc = affine_exact_stage(c, jobs);
  if (rc) return rc;
  for (size_t k = 0; k < jobs.size(); ++k) {
    const ExactJob &j = jobs[k];
    if (k < nwhole) {
      maxima[j.index * nq + (size_t)j.q] = j.best > 0 ? j.best : 0.0f;
      if (ends && j.best > 0) { ends[2 * j.q] = j.ci; ends[2 * j.q + 1] = j.cj; }
    } else {
      if (j.best != j.target) return fail(ctx, MI355_SW_ENODEV, "internal: maximum of the affine sweep not found again by the exact kernel");
      ends[2 * j.q] = j.ci; ends[2 * j.q + 1] = j.cj;
    }
  }
  std::vector<AffineTraceItem> items(tout && ends ? nq : 0);        // every query of the batch against the one range
  for (size_t k = 0; k < items.size(); ++k) items[k] = AffineTraceItem{(int)k, ranges[0].lo, 0.0f, 0, 0};
  return affine_end(c, items, maxima, ends, ends ? tout : nullptr);
}

// ---- sw_affine_pair_kernel (sw_affine_pair_kernel.h): a list of (query, window of the resident reference) pairs -----------------
constexpr int64_t kAffinePairColsMax = (int64_t)1 << 20;   // columns of one window: keeps the slowest slot of a launch to about 2^20 steps
                                                          // of at most 32 rows — an estimate from the kernel's op count (some 0.3 s at
                                                          // R = 32); nobody has measured it
constexpr size_t kAffinePairLdsMax = 32 * 1024;            // the workgroup's score table [letters + 1][classes + 1]
constexpr size_t kAffinePairGroupProblems = (size_t)1 << 22;   // problems between two downloads of (best, cell)

size_t affine_pair_lds(const RefData &ref, const AffineProfPlan &plan) { return (size_t)ref.ncodes * (size_t)plan.nclass * 4; }

// The caller's list (validated there, not owned): pair k is query qid[k] of the batch against [lefts[k], rights[k]) of the reference,
// counting only cells with band_lo[k] <= j - i <= band_hi[k] (both null: no bands).
struct AffinePairList {
  size_t npairs; const int32_t *qid; const int64_t *lefts, *rights, *band_lo, *band_hi;
  int64_t cols(size_t k) const { return rights[k] - lefts[k]; }
};

// pair k as both list kernels take it: the query's bytes, the window's codes
template <class Problem>
void affine_pair_fill(const AffineCall &c, const AffinePairList &pl, size_t k, Problem &p) {
  p.x = c.q.bytes.as<uint8_t>() + c.q.off[pl.qid[k]];
  p.y = c.ref.codes.as<uint8_t>() + pl.lefts[k];
  p.m = c.q.len[pl.qid[k]];
  p.n = (int32_t)pl.cols(k);
}

// the instance of the least R of kPairR with 16 R >= rows, of kBandR with 16 R >= W diagonals (0: none)
int affine_pair_R(int rows) {
  for (int R : kPairR) if (16 * R >= rows) return R;
  return 0;
}
int affine_band_R(int64_t W) {
  for (int R : kBandR) if (16 * (int64_t)R >= W) return R;
  return 0;
}

// A kernel family as affine_list_stage takes it: the problem and the item it is made from, the instance R of either, what comes first
// among items of one R (the larger `size`), the instance itself, the cells of a problem and the description of a launch.  There is
// one family per geometry of the list kernels — AffinePairFamily (sw_affine_pair_kernel.h: sized by the window's length) and
// AffineBandFamily (sw_affine_band_kernel.h: sized by rows) — over a MODE M, which holds what differs between the kernels of a
// geometry and nothing else:
//   M::Source                 where an item comes from: the caller's pair list (AffineListedPair, AffineListedBandPair) or an item
//                             with its own pointers (AffineOwnItem, behind AffineExtItem): Item, id, rows, cols / W, fill
//   M::kernel<R>(c)           the kernel instance of an R
//   M::kOuts, M::keep_all(c)  (best, cell) a problem writes; whether a result that is not positive is kept
//   M::path(c), M::name(c)    the two name strings of a launch (path_note, mi355_sw_last_kernel)
//   M::ops(c, R)              the op count per cell of the compiled row loop
//   M::kNoInstance            the message of a missing instance
// M::kCountsRows (optional, the z-drop mode alone): the mode's wavefronts add the rows their loops ran to AffinePairArgs::zrows
template <class M, class = void> struct AffineModeCountsRows : std::false_type {};
template <class M> struct AffineModeCountsRows<M, std::void_t<decltype(M::kCountsRows)>> : std::integral_constant<bool, M::kCountsRows> {};
template <class M>
struct AffinePairFamily {
  typedef AffinePairProblem Problem; typedef typename M::Source Source; typedef typename Source::Item Item;
  const AffineCall &c; Source src;
  static constexpr const char *kNoInstance = M::kNoInstance;
  static constexpr int kOuts = M::kOuts;
  static constexpr bool kCountsRows = false;
  bool keep_all() const { return M::keep_all(c); }
  static uint32_t id(const Item &a) { return Source::id(a); }
  int R(const Item &a) const { return affine_pair_R(src.rows(c, a)); }
  static int R(const Problem &p) { return affine_pair_R(p.m); }
  int64_t size(const Item &a) const { return src.cols(a); }        // longest window first: the slots of a wavefront run similar step counts
  void fill(const Item &a, Problem &p) const { src.fill(c, a, p); }
  static double cells(const Problem &p) { return (double)p.m * (double)p.n; }
  auto kernel(int R) const {
    void (*kern)(const Problem *, int, const AffinePairArgs) = nullptr;
    with_listed_R<kPairR>(R, [&](auto r) { kern = M::template kernel<decltype(r)::value>(c); });
    return kern;
  }
  void note(double cells, int R, const Problem &first) const {
    path_note(c.ctx, M::path(c), R);
    affine_note_kernel(c.ctx, cells, MI355_SW_CELL_F32, 16, R, first.n, first.n, 0, M::ops(c, R), M::name(c), R);
  }
};
template <class M>
struct AffineBandFamily {
  typedef AffineBandProblem Problem; typedef typename M::Source Source; typedef typename Source::Item Item;
  const AffineCall &c; Source src;
  static constexpr const char *kNoInstance = M::kNoInstance;
  static constexpr int kOuts = M::kOuts;
  static constexpr bool kCountsRows = AffineModeCountsRows<M>::value;
  bool keep_all() const { return M::keep_all(c); }
  static uint32_t id(const Item &a) { return Source::id(a); }
  static int R(const Item &a) { return affine_band_R(a.W); }
  static int R(const Problem &p) { return affine_band_R(p.W); }
  int64_t size(const Item &a) const { return src.rows(c, a); }     // longest query first: the slots of a wavefront leave the row loop at similar steps
  void fill(const Item &a, Problem &p) const { src.fill(c, a, p); }
  static double cells(const Problem &p) { return (double)p.m * (double)p.W; }
  auto kernel(int R) const {
    void (*kern)(const Problem *, int, const AffinePairArgs) = nullptr;
    with_listed_R<kBandR>(R, [&](auto r) { kern = M::template kernel<decltype(r)::value>(c); });
    return kern;
  }
  void note(double cells, int R, const Problem &) const {          // all 16 R registers of a lane row work whatever W is: the model's time is rows x 16 R
    path_note(c.ctx, M::path(c), R);
    affine_note_kernel(c.ctx, cells, MI355_SW_CELL_F32, 16, R, 16 * R, 16 * R, 0, M::ops(c, R), M::name(c), R);
  }
};

// One banded pair as the band kernel takes it: the band clipped to the matrix, its lowest diagonal and its width.
struct AffineBandPair { uint32_t id; int32_t lo, W; };

// Items of the caller's pair list (affine_pairs): the pair's index, for the band kernel with its band
struct AffineListedPair {
  typedef uint32_t Item;
  const AffinePairList &pl;
  static uint32_t id(Item a) { return a; }
  int rows(const AffineCall &c, Item a) const { return c.q.len[pl.qid[a]]; }
  int64_t cols(Item a) const { return pl.cols(a); }
  void fill(const AffineCall &c, Item a, AffinePairProblem &p) const { affine_pair_fill(c, pl, a, p); }
};
struct AffineListedBandPair {
  typedef AffineBandPair Item;
  const AffinePairList &pl;
  static uint32_t id(const Item &a) { return a.id; }
  int rows(const AffineCall &c, const Item &a) const { return c.q.len[pl.qid[a.id]]; }
  void fill(const AffineCall &c, const Item &a, AffineBandProblem &p) const { affine_pair_fill(c, pl, a.id, p); p.lo = a.lo; p.W = a.W; }
};

// sw_affine_pair_kernel / sw_affine_pair_e2e_kernel, by the call's mode
struct AffinePairMode {
  typedef AffineListedPair Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_pair_kernel instance for this query";
  static constexpr int kOuts = 1;
  static bool keep_all(const AffineCall &c) { return c.e2e(); }    // end-to-end: a score may be <= 0
  template <int R> static auto kernel(const AffineCall &c) { return c.e2e() ? &sw_affine_pair_e2e_kernel<R> : &sw_affine_pair_kernel<R>; }
  static const char *path(const AffineCall &c) { return c.e2e() ? "affine_pair_e2e[R=%d]" : "affine_pair[R=%d]"; }
  static const char *name(const AffineCall &c) { return c.e2e() ? "sw_affine_pair_e2e_kernel<R=%d>" : "sw_affine_pair_kernel<R=%d>"; }
  static double ops(const AffineCall &c, int R) {
    // end-to-end, per step and lane: seven ops, the table address' v_add and the winner row's select per cell, and eleven of overhead
    // (the local instance's twelve without the key's v_or); no key, no maximum3 fold.  The 16 border steps of a slot are not counted
    // local, per step and lane: seven ops, the table address' v_add and the key's v_or per cell, a maximum3 per two cells for the
    // step's best key, and twelve of overhead as compiled (two DPP moves and their two copies, the row pointer's multiply
    // and add, the column, the code's address, and compare, two selects and the v_or of the value-only key update)
    return c.e2e() ? (9.0 * R + 11.0) / (double)R : (9.0 * R + (R + 1) / 2 + 12.0) / (double)R;
  }
};

// sw_affine_band_kernel: pairs with a diagonal band; the table is the pair kernel's.
struct AffineBandMode {
  typedef AffineListedBandPair Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_band_kernel instance for this band";
  static constexpr int kOuts = 1;
  static bool keep_all(const AffineCall &) { return false; }
  template <int R> static auto kernel(const AffineCall &) { return &sw_affine_band_kernel<R>; }
  static const char *path(const AffineCall &) { return "affine_band[R=%d]"; }
  static const char *name(const AffineCall &) { return "sw_affine_band_kernel<R=%d>"; }
  static double ops(const AffineCall &, int R) {
    // per step and lane, as compiled: fourteen ops per register — the table address' multiply-add, the clamped add,
    // sub / max for F, max for Ht, Ht - o, sub / max of the lane's scan, maximum3 for H, the cap's min, the key's v_or, H - o, the
    // carry's sub and one move — a maximum3 per two registers for the step's key, and 29 of overhead: two DPP moves for F, five DPP
    // moves (each with the move of its `old`) and four sub / max pairs for the lanes' scan, the explicit (value, column) compare
    // with its selects, the window addresses
    return (14.0 * R + (R + 1) / 2 + 29.0) / (double)R;
  }
};

// The kernel of family F (AffinePairFamily, AffineBandFamily) over `items`: by instance, then F's larger size first, then index; one
// class table for queries of at most mmax rows; per group of kAffinePairGroupProblems one upload of the descriptors, one launch per
// instance and one download; score / ends of the pairs with a positive maximum (F::keep_all: of every pair).  A problem of F
// writes F::kOuts results (best, cell): score[npairs][kOuts], ends[npairs][kOuts][2].
template <class F>
int affine_list_stage(const F &f, const AffineProfPlan &plan, std::vector<typename F::Item> &items, int mmax, float *score, int64_t *ends) {
  typedef typename F::Problem Problem;
  const AffineCall &c = f.c; mi355_sw_ctx *ctx = c.ctx;
  if (items.empty()) return 0;
  std::sort(items.begin(), items.end(), [&](const typename F::Item &a, const typename F::Item &b) {
    const int Ra = f.R(a), Rb = f.R(b);
    if (Ra != Rb) return Ra < Rb;
    const int64_t sa = f.size(a), sb = f.size(b);
    return sa != sb ? sa > sb : f.id(a) < f.id(b);
  });
  const int nl = c.ref.ncodes - 1, nrows = nl + 1, ncls = plan.nclass;
  const size_t tab_floats = (size_t)nrows * ncls;
  AffinePairArgs sa;
  sa.nrows = nrows; sa.ncls = ncls;
  int rc = affine_class_table(c, plan, mmax, tab_floats, 1, ncls, "hipMalloc(affine pair table) failed", sa.tab, sa);
  if (rc) return rc;
  sa.zdrop_s = std::floor(c.zdrop) / sa.unscale;                   // (a power of two: exact; read by the z-drop mode alone, as the word below)
  sa.zrows = nullptr;
  for (size_t g0 = 0; g0 < items.size(); g0 += kAffinePairGroupProblems) {
    const size_t np = std::min(kAffinePairGroupProblems, items.size() - g0);
    const char *nomem = "affine pairs: allocation of the pair scratch failed";
    constexpr size_t NO = F::kOuts;
    if (ctx->wprobs.ensure(np * sizeof(Problem)) || ctx->outs_f.ensure(NO * np * 4 + 64) || ctx->outs_i.ensure(NO * np * 16) ||
        ctx->pin_probs.ensure(np * sizeof(Problem)))
      return fail(ctx, MI355_SW_ENOMEM, nomem);
    Problem *pr = ctx->pin_probs.as<Problem>();
    // the z-drop mode's row counter: a word of outs_f behind the group's results (the 64 spare bytes), zeroed in front of the
    // launches and brought down by the results' own copy — no launch, copy or wait of its own
    const size_t zrows_at = (NO * np * 4 + 7) & ~(size_t)7, zrows_tail = F::kCountsRows ? zrows_at + 8 - NO * np * 4 : 0;
    if (F::kCountsRows) {
      sa.zrows = reinterpret_cast<unsigned long long *>(ctx->outs_f.as<uint8_t>() + zrows_at);
      HIPCHK(ctx, hipMemsetAsync(sa.zrows, 0, 8, ctx->stream));
    }
    for (size_t i = 0; i < np; ++i) f.fill(items[g0 + i], pr[i]);  // one upload of the pair list
    HIPCHK(ctx, hipMemcpyAsync(ctx->wprobs.p, pr, np * sizeof(Problem), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    for (size_t i0 = 0; i0 < np;) {                                // one launch per instance
      const int R = F::R(pr[i0]);
      size_t i1 = i0; double cells = 0;
      while (i1 < np && F::R(pr[i1]) == R) { cells += F::cells(pr[i1]); ++i1; }
      const auto kern = f.kernel(R);
      if (!kern) return fail(ctx, MI355_SW_ENODEV, F::kNoInstance);
      sa.best = ctx->outs_f.as<float>() + NO * i0;
      sa.cell = ctx->outs_i.as<int64_t>() + 2 * NO * i0;
      launch_dyn_lds(kern, dim3((unsigned)((i1 - i0 + 15) / 16)), dim3(256), tab_floats * 4, ctx->stream,
                     ctx->wprobs.as<Problem>() + i0, (int)(i1 - i0), sa);
      HIPCHK(ctx, hipGetLastError());
      ctx->timings[4] += 1;
      f.note(cells, R, pr[i0]);
      i0 = i1;
    }
    const float *h_best = nullptr; const int64_t *h_cell = nullptr;
    rc = affine_download(ctx, NO * np, nomem, h_best, h_cell, zrows_tail); if (rc) return rc;
    if (F::kCountsRows) {
      unsigned long long ran = 0;
      memcpy(&ran, reinterpret_cast<const uint8_t *>(h_best) + zrows_at, 8);
      ctx->zdrop_rows_run += (size_t)ran;
    }
    for (size_t i = 0; i < NO * np; ++i) {
      const size_t id = NO * f.id(items[g0 + i / NO]) + i % NO;
      if (!f.keep_all() && !(h_best[i] > 0)) continue;
      score[id] = h_best[i]; ends[2 * id] = h_cell[2 * i]; ends[2 * id + 1] = h_cell[2 * i + 1];
    }
  }
  return 0;
}

// Which kernel a pair takes.  kPairZeros: an empty query or window, or a band that misses the matrix — the zeroed outputs stand.  kPairKernel / kPairExact: the
// unbanded pair, which a band that covers the matrix is too.  kPairBand / kPairExactBand: a banded pair; it never runs on an unbanded kernel.
enum AffinePairKind { kPairZeros, kPairKernel, kPairBand, kPairExact, kPairExactBand };
struct AffinePairRoute {
  AffinePairKind kind; int64_t lo_e, hi_e;   // the band clipped to the matrix (no bands: the matrix, 1 - m .. n - 1)
  bool banded() const { return kind == kPairBand || kind == kPairExactBand; }
};

// The route of pair k.  table_ok: the call's class table fits the list kernels (affine_pairs).  The list kernels take 1..512 rows
// whose values are exact in float32 (local mode: the key's bits free, smax * (rows + 1) < 2^18; end-to-end: affine_e2e_exact) — the
// pair kernel windows of at most 2^20 columns, the band kernel at most 256 diagonals (an instance of kBandR) of windows whose
// columns fit int32 with room for the band; every other pair is a whole problem of the exact kernel (affine_pair_whole_job).
AffinePairRoute affine_pair_route(const AffineCall &c, const AffinePairList &pl, bool table_ok, size_t k) {
  const int64_t m = c.q.len[pl.qid[k]], n = pl.cols(k);
  AffinePairRoute r{kPairZeros, 1 - m, n - 1};
  if (m < 1 || n < 1) return r;
  if (pl.band_lo) { r.lo_e = std::max(pl.band_lo[k], r.lo_e); r.hi_e = std::min(pl.band_hi[k], r.hi_e); }
  if (r.lo_e > r.hi_e) return r;
  const bool exact_f32 = c.e2e() ? affine_e2e_exact(c.t, (double)m) : (double)c.t.smax * ((double)m + 1.0) < kAffineProfBound;
  if (r.lo_e != 1 - m || r.hi_e != n - 1) {
    const bool list = table_ok && !opt().no_affine_band && m <= kBandRowsMax && affine_band_R(r.hi_e - r.lo_e + 1) != 0 && n <= 0x7fff0000 && exact_f32;
    r.kind = list ? kPairBand : kPairExactBand;
  } else {
    r.kind = table_ok && m <= kMaxRowsFast && n <= kAffinePairColsMax && exact_f32 ? kPairKernel : kPairExact;
  }
  return r;
}

// why pair k, routed to the exact kernel, cannot run at all: outside its list kernel and too large for a whole problem
std::string affine_pair_refusal(const AffineCall &c, const AffinePairList &pl, const AffinePairRoute &r, size_t k) {
  const int m = c.q.len[pl.qid[k]];
  char msg[360];
  if (r.banded())
    std::snprintf(msg, sizeof msg, "affine pairs: banded pair %zu (%d rows x %lld columns, %lld diagonals) is outside the band kernel "
                  "(1..512 rows, at most 256 diagonals, smax * (rows + 1) < 2^18, gap_open < 2^18, a score table within 32 KiB%s) and has "
                  "more than 2^26 cells for the exact kernel", k, m, (long long)pl.cols(k), (long long)(r.hi_e - r.lo_e + 1),
                  opt().no_affine_band ? "; option no_affine_band is set" : "");
  else
    std::snprintf(msg, sizeof msg, "affine pairs: pair %zu (%d rows x %lld columns) is outside the pair kernel (1..512 rows, 1..2^20 columns, "
                  "%s) and has more than 2^26 cells for the exact kernel", k, m, (long long)pl.cols(k),
                  c.e2e() ? "end-to-end: 2 gap_open + (rows + 1) gap_extend - min(smin, 0) < 2^24, smax * (rows + 1) + gap_open < 2^24"
                          : "smax * (rows + 1) < 2^18, gap_open < 2^18");
  return msg;
}

// Pair k joins `jobs` as a whole problem of the exact kernel (ExactJob::index: the pair; ExactBandJob: under its clipped band), or the
// refusal: too many cells or scores beyond float32's integers (affine_whole_job), or more rows than the kernel's LDS diagonals hold.
template <class Job>
int affine_pair_whole_job(const AffineCall &c, const AffinePairList &pl, const AffinePairRoute &r, size_t k, std::vector<Job> &jobs) {
  Job j;
  if (!affine_whole_job(c, pl.qid[k], pl.lefts[k], pl.cols(k), k, j)) return fail(c.ctx, MI355_SW_ENOTSUP, affine_pair_refusal(c, pl, r, k));
  if (affine_exact_lds(c.q.len[pl.qid[k]]) > kExactLdsMax) return fail(c.ctx, MI355_SW_ENOTSUP, "affine pairs: query longer than the exact kernel's LDS diagonals hold");
  if constexpr (std::is_same<Job, ExactBandJob>::value) { j.blo = (int32_t)r.lo_e; j.bhi = (int32_t)r.hi_e; }   // (|lo_e|, |hi_e| < 2^26 cells: int32)
  jobs.push_back(j);
  return 0;
}

// (best, cell) of whole jobs back to their pairs: of those with a positive maximum (keep_all: of every one)
template <class Job>
void affine_scatter_jobs(const std::vector<Job> &jobs, bool keep_all, float *score, int64_t *ends) {
  for (const Job &j : jobs) {
    if (!keep_all && !(j.best > 0)) continue;
    score[j.index] = j.best; ends[2 * j.index] = j.ci; ends[2 * j.index + 1] = j.cj;
  }
}

// The pairs of `pl`, each an independent problem with zero borders.  score[npairs]; ends[npairs][2] = row, column relative to the
// window start; tout (may be null): the traceback of every pair (affine_trace).  Results come back in the caller's order.
// Every pair goes where affine_pair_route sends it; the stages run in a fixed order: the pair kernel, the band kernel, the exact
// kernel's unbanded and then its banded jobs, the traceback.
// mode MI355_SW_AFFINE_END_TO_END: the end-to-end model of the header on the E2E instances of the same kernels (no bands: the caller
// refuses them); only an empty query or an empty window leaves the zeros (a score may be <= 0).
int affine_pairs(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, int mode, const AffinePairList &pl, const mi355_sw_affine_params &p,
                 float *score, int64_t *ends, std::vector<TraceOut> *tout) {
  const size_t npairs = pl.npairs;
  for (size_t k = 0; k < npairs; ++k) { score[k] = 0.0f; ends[2 * k] = 0; ends[2 * k + 1] = 0; }
  if (tout) tout->assign(npairs, TraceOut());
  AffineCall c{ctx, ref, q, p, AffineTable(), mode};
  int rc = affine_begin(c);
  if (rc) return rc > 0 ? 0 : rc;
  const double open_bound = c.e2e() ? 16777216.0 : kAffineProfBound;
  AffineProfPlan plan;
  if (!opt().no_affine_pairs) {
    affine_byte_classes(ref, p, c.t, plan, open_bound);
    if (!plan.ok && ref.ncodes >= 2 && ref.ncodes <= 256 && (double)c.t.open < open_bound) {
      // a table that scores all 256 bytes differently: every byte is its own class
      plan.rep.resize(256);
      for (int a = 0; a < 256; ++a) { plan.cls[a] = (uint8_t)a; plan.rep[a] = a; }
      plan.nclass = 257;
      plan.ok = true;
    }
  }
  const bool table_ok = plan.ok && affine_pair_lds(ref, plan) <= kAffinePairLdsMax;

  if (npairs > 0xFFFFFFFFull) return fail(ctx, MI355_SW_ENOTSUP, "affine pairs: more than 2^32 pairs");
  std::vector<uint32_t> fast;                                      // pair indices of sw_affine_pair_kernel
  std::vector<AffineBandPair> band;                                // pairs of sw_affine_band_kernel
  std::vector<ExactJob> jobs;                                      // whole problems of the exact kernel
  std::vector<ExactBandJob> bjobs;                                 // and of its BAND instance
  std::vector<AffineTraceItem> items(tout ? npairs : 0);
  int mmax = 0, band_mmax = 0;
  for (size_t k = 0; k < npairs; ++k) {
    const AffinePairRoute r = affine_pair_route(c, pl, table_ok, k);
    const int m = q.len[pl.qid[k]];
    if (tout) {
      items[k] = AffineTraceItem{pl.qid[k], pl.lefts[k], 0.0f, 0, 0};
      if (r.banded()) { items[k].banded = true; items[k].blo = r.lo_e; items[k].bhi = r.hi_e; }
    }
    switch (r.kind) {
      case kPairZeros: break;
      case kPairKernel: fast.push_back((uint32_t)k); mmax = std::max(mmax, m); break;
      case kPairBand: band.push_back(AffineBandPair{(uint32_t)k, (int32_t)r.lo_e, (int32_t)(r.hi_e - r.lo_e + 1)}); band_mmax = std::max(band_mmax, m); break;
      case kPairExact: rc = affine_pair_whole_job(c, pl, r, k, jobs); break;
      case kPairExactBand: rc = affine_pair_whole_job(c, pl, r, k, bjobs); break;
    }
    if (rc) return rc;
  }

  // (one class table per list stage, each for its own tallest query)
  rc = affine_list_stage(AffinePairFamily<AffinePairMode>{c, {pl}}, plan, fast, mmax, score, ends);
  if (!rc) rc = affine_list_stage(AffineBandFamily<AffineBandMode>{c, {pl}}, plan, band, band_mmax, score, ends);
  if (!rc) rc = affine_exact_stage(c, jobs);
  if (!rc) rc = affine_exact_stage(c, bjobs);
  if (rc) return rc;
  affine_scatter_jobs(jobs, c.e2e(), score, ends);
  affine_scatter_jobs(bjobs, false, score, ends);
  return affine_end(c, items, score, ends, tout);
}

// ---- the anchored seed extension (include/mi355_sw.h "anchored seed extension", DESIGN.md §3.8 lemma L21) -------------------------
// The caller's list (validated there, not owned): pair k is the letters [q_lo[k], q_hi[k]) of query qid[k] (both null: the whole
// query) against [lefts[k], rights[k]) of the reference, backward[k] != 0: on both strings reversed (null: every pair forward).
// band_lo / band_hi (both null: no bands): pair k counts only cells with band_lo[k] <= j - i <= band_hi[k], i and j from the anchor.
struct AffineExtList {
  size_t npairs; const int32_t *qid, *q_lo, *q_hi; const int64_t *lefts, *rights; const uint8_t *backward;
  const int64_t *band_lo = nullptr, *band_hi = nullptr;
  bool back(size_t k) const { return backward && backward[k]; }
};

// Pair `id` as every kernel takes it: where its letters and its window lie on the device — in the resident buffers, or for a
// backward pair in their reversed copies — so that no stage below knows a direction.
// banded: the pair runs under its effective band blo <= j - i <= bhi (W diagonals), n the CLIPPED window (affine_extend).
struct AffineExtItem { uint32_t id; const uint8_t *x, *ycodes, *ybytes; int32_t m; int64_t n; bool banded = false; int32_t blo = 0, bhi = 0, W = 0; };

// Lemma L21, the admission test of sw_affine_pair_ext_kernel: every value of a real cell is an integer below 2^24 in magnitude.
// H(i,j) >= -(2o + (i+j-2) e), the path along row 0 and down column j, so Ho, E, F >= -(3o + (m+n-2) e), E - e and F - e one e
// lower, the diagonal term Ho + (s + o) >= -(2o + (m+n-2) e) + smin and the table's |s + o| <= o - smin: one inequality covers the
// low side, 3o + (m+n) e - smin < 2^24.  Upwards H <= smax m and s + o <= smax + o.  A positive H lends the key its five low
// mantissa bits: smax (m + 1) < 2^18, as in the local instance.  The exact kernel forms neither sum and has no key.
bool affine_ext_exact(const AffineTable &t, double m, double n) {
  return 3.0 * t.open + (m + n) * t.ext - t.smin < 16777216.0 && (double)t.smax * m + t.open < 16777216.0 &&
         (double)t.smax * (m + 1.0) < kAffineProfBound;
}
bool affine_ext_whole_exact(const AffineTable &t, double m, double n) {
  return 3.0 * t.open + (m + n) * t.ext < 16777216.0 && 2.0 * t.open + (m + n) * t.ext - t.smin < 16777216.0 &&
         (double)t.smax * (m + 1.0) < 16777216.0;
}

// Lemma L22, the admission test of sw_affine_band_ext_kernel for a pair of m rows under a band of W diagonals.  The low side is not
// L21's: the path along row 0 and down a column leaves the band.  The cheapest in-band path to (i,j) runs along diagonal 0 to
// (min(i,j), min(i,j)), every step at least smin = -a (a = max(-smin, 0); t.smin <= 0), and then one gap of |j-i| <= W - 1 letters, all
// of it in the band because the band holds diagonal 0: H(i,j) >= -(a min(i,j) + o + (|j-i|-1) e) >= -(a m + o + (W-2) e).
// So Ho, E, F >= -(a m + 2o + (W-2) e), the scan's Ht - o >= F - o >= -(a m + 3o + (W-2) e) and one e lower inside the lane, E - e and
// F - e one e lower, the diagonal term Ho + (s + o) >= -(a m + 2o + (W-2) e) + smin + o and the table's |s + o| <= o - smin: one
// inequality covers the low side, a m + 3o + (W+1) e - smin < 2^24.  (A decayed carry of the scan may fall below: it is rounded,
// stays below every real value and wins no maximum.)  Upwards H <= smax m and s + o <= smax + o; a positive H lends the key its
// five low mantissa bits: smax (m + 1) < 2^18.  The exact kernel under a band forms no s + o, runs no scan and has no key: its lowest
// values are H - o and E - e, F - e >= -(a m + 2o + (W-1) e) and the diagonal term H + s >= -(a m + o + (W-2) e) + smin.
bool affine_band_ext_exact(const AffineTable &t, double m, double W) {
  return -(double)t.smin * m + 3.0 * t.open + (W + 1.0) * t.ext - t.smin < 16777216.0 && (double)t.smax * m + t.open < 16777216.0 &&
         (double)t.smax * (m + 1.0) < kAffineProfBound;
}
bool affine_band_ext_whole_exact(const AffineTable &t, double m, double W) {
  return -(double)t.smin * m + 2.0 * t.open + W * t.ext - t.smin < 16777216.0 && (double)t.smax * (m + 1.0) < 16777216.0;
}

// Lemma L23, the admission tests of sw_affine_pair_glob_kernel and sw_affine_band_glob_kernel: the loops of the two kernels above
// without their folds, so every value they form is one L21 / L22 bound already — the same recurrence on the same borders (the same
// band), the same table of s + o, the same scan.  What the folds needed and these kernels do not is the key: no value lends five
// mantissa bits, and smax (m + 1) < 2^18 goes.  The capture forms no new value (a select; the band kernel's Ho + o is H, within
// [-(a m + o + (W-2) e), smax m]).  The exact kernel's bounds are the extension calls': affine_ext_whole_exact and
// affine_band_ext_whole_exact.
bool affine_glob_exact(const AffineTable &t, double m, double n) {
  return 3.0 * t.open + (m + n) * t.ext - t.smin < 16777216.0 && (double)t.smax * m + t.open < 16777216.0;
}
bool affine_band_glob_exact(const AffineTable &t, double m, double W) {
  return -(double)t.smin * m + 3.0 * t.open + (W + 1.0) * t.ext - t.smin < 16777216.0 && (double)t.smax * m + t.open < 16777216.0;
}

// The reversed copies of the resident reference (codes and bytes) and of the batch's bytes, built with reverse_bytes_kernel where
// the cached ones are of another version.
int affine_ext_reversed(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q) {
  auto reverse = [&](const DevBuf &src, DevBuf &dst, size_t n) -> int {
    if (n == 0) return 0;
    if (dst.ensure(n)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(reversed copy) failed");
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(reverse_bytes_kernel, dim3(blocks), dim3(256), 0, ctx->stream, src.as<uint8_t>(), dst.as<uint8_t>(), n);
    HIPCHK(ctx, hipGetLastError());
    return 0;
  };
  if (!ctx->rev_ref_valid || ctx->rev_ref_version != ref.version) {
    ctx->rev_ref_valid = false;
    { int rc = reverse(ref.codes, ctx->rev_codes, ref.n); if (rc) return rc; }
    { int rc = reverse(ref.bytes, ctx->rev_bytes, ref.n); if (rc) return rc; }
    ctx->rev_ref_valid = true; ctx->rev_ref_version = ref.version;
  }
  if (!ctx->rev_q_valid || ctx->rev_q_version != q.version) {
    ctx->rev_q_valid = false;
    size_t total = 0;
    for (size_t k = 0; k < q.nq; ++k) total = std::max(total, (size_t)q.off[k] + (size_t)q.len[k]);
    { int rc = reverse(q.bytes, ctx->rev_q, total); if (rc) return rc; }
    ctx->rev_q_total = total;
    ctx->rev_q_valid = true; ctx->rev_q_version = q.version;
  }
  return 0;
}

// What the anchored calls (affine_extend, affine_global) share in front of their routing.
// The classes of the call's scoring for the list kernels — none under option no_affine_pairs; every byte its own class where the table
// scores all 256 bytes differently, as affine_pairs — and whether their table fits the kernels' LDS.
bool affine_ext_plan(const AffineCall &c, AffineProfPlan &plan) {
  const RefData &ref = c.ref;
  if (!opt().no_affine_pairs) {
    affine_byte_classes(ref, c.p, c.t, plan, 16777216.0);
    if (!plan.ok && ref.ncodes >= 2 && ref.ncodes <= 256 && (double)c.t.open < 16777216.0) {
      plan.rep.resize(256);                                        // every byte its own class, as affine_pairs
      for (int a = 0; a < 256; ++a) { plan.cls[a] = (uint8_t)a; plan.rep[a] = a; }
      plan.nclass = 257;
      plan.ok = true;
    }
  }
  return plan.ok && affine_pair_lds(ref, plan) <= kAffinePairLdsMax;
}

// the reversed copies, where the list holds a backward pair
int affine_ext_any_reversed(const AffineCall &c, const AffineExtList &el) {
  bool any_back = false;
  for (size_t k = 0; k < el.npairs && !any_back; ++k) any_back = el.back(k);
  return any_back ? affine_ext_reversed(c.ctx, c.ref, c.q) : 0;
}

// pair k of the list as an item: its rows, its window and where both lie on the device (unbanded; the caller sets the band)
AffineExtItem affine_ext_item(const AffineCall &c, const AffineExtList &el, size_t k) {
  mi355_sw_ctx *ctx = c.ctx; const RefData &ref = c.ref; const QueryBatch &q = c.q;
  const int qi = el.qid[k];
  const int64_t qlo = el.q_lo ? el.q_lo[k] : 0, qhi = el.q_hi ? el.q_hi[k] : q.len[qi];
  AffineExtItem it;
  it.id = (uint32_t)k; it.m = (int32_t)(qhi - qlo); it.n = el.rights[k] - el.lefts[k];
  if (el.back(k)) {
    it.x = ctx->rev_q.as<uint8_t>() + ((int64_t)ctx->rev_q_total - q.off[qi] - qhi);
    it.ycodes = ctx->rev_codes.as<uint8_t>() + ((int64_t)ref.n - el.rights[k]);
    it.ybytes = ctx->rev_bytes.as<uint8_t>() + ((int64_t)ref.n - el.rights[k]);
  } else {
    it.x = q.bytes.as<uint8_t>() + q.off[qi] + qlo;
    it.ycodes = ref.codes.as<uint8_t>() + el.lefts[k];
    it.ybytes = ref.bytes.as<uint8_t>() + el.lefts[k];
  }
  return it;
}

// An item that carries its own pointers, its rows, its window and its band (AffineExtItem: affine_extend, affine_global)
struct AffineOwnItem {
  typedef AffineExtItem Item;
  static uint32_t id(const Item &a) { return a.id; }
  static int rows(const AffineCall &, const Item &a) { return a.m; }
  static int64_t cols(const Item &a) { return a.n; }
  static void fill(const AffineCall &, const Item &a, AffinePairProblem &p) { p.x = a.x; p.y = a.ycodes; p.m = a.m; p.n = (int32_t)a.n; }
  static void fill(const AffineCall &, const Item &a, AffineBandProblem &p) {   // the clipped window and the effective band
    p.x = a.x; p.y = a.ycodes; p.m = a.m; p.n = (int32_t)a.n; p.lo = a.blo; p.W = a.W;
  }
};

// sw_affine_pair_ext_kernel: two results per problem (best extension, to the end).
struct AffineExtMode {
  typedef AffineOwnItem Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_pair_ext_kernel instance for this query";
  static constexpr int kOuts = 2;
  static bool keep_all(const AffineCall &) { return true; }        // a to-end score may be <= 0, a best extension is 0 at least
  template <int R> static auto kernel(const AffineCall &) { return &sw_affine_pair_ext_kernel<R>; }
  static const char *path(const AffineCall &) { return "affine_pair_ext[R=%d]"; }
  static const char *name(const AffineCall &) { return "sw_affine_pair_ext_kernel<R=%d>"; }
  static double ops(const AffineCall &, int R) {
    // per step and lane: the local instance's count (AffinePairMode::ops) and two more per cell: the max with 0 in front of the
    // key and the row-m select; the row-0 subtract and max, the second compare and its selects are three more of overhead.  The 16
    // border steps of a slot are not counted
    return (11.0 * R + (R + 1) / 2 + 15.0) / (double)R;
  }
};

// sw_affine_band_ext_kernel: the banded pairs of the extension calls; two results per problem, as AffineExtMode.
struct AffineBandExtMode {
  typedef AffineOwnItem Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_band_ext_kernel instance for this band";
  static constexpr int kOuts = 2;
  static bool keep_all(const AffineCall &) { return true; }
  template <int R> static auto kernel(const AffineCall &) { return &sw_affine_band_ext_kernel<R>; }
  static const char *path(const AffineCall &) { return "affine_band_ext[R=%d]"; }
  static const char *name(const AffineCall &) { return "sw_affine_band_ext_kernel<R=%d>"; }
  static double ops(const AffineCall &, int R) {
    // per step and lane, as compiled: the local band instance's count (AffineBandMode::ops), one more per register — the max with
    // 0 in front of the key — and four more of overhead (the compare of the step's row with the slot's m in front of the to-end
    // branch, and moves of the -inf operands).  The branch's four scalar compares are no vector ops, and its fold (six ops per
    // register) runs at one step of a slot's rows: not counted
    return (15.0 * R + (R + 1) / 2 + 33.0) / (double)R;
  }
};

// ---- the z-drop stop rule of the banded extension (include/mi355_sw.h "z-drop", DESIGN.md §3.8 lemma L24) ----
// sw_affine_band_extz_kernel: AffineBandExtMode's items and results under the stop rule; the to-end half's first cell word is rows_done.
struct AffineBandExtZMode {
  typedef AffineOwnItem Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_band_extz_kernel instance for this band";
  static constexpr int kOuts = 2;
  static constexpr bool kCountsRows = true;                        // counter zdrop_rows_run (affine_list_stage)
  static bool keep_all(const AffineCall &) { return true; }
  template <int R> static auto kernel(const AffineCall &) { return &sw_affine_band_extz_kernel<R>; }
  static const char *path(const AffineCall &) { return "affine_band_extz[R=%d]"; }
  static const char *name(const AffineCall &) { return "sw_affine_band_extz_kernel<R=%d>"; }
  static double ops(const AffineCall &, int R) {
    // per step and lane, counted in the compiled row loop of all eight instances against the extension instance's loop: that mode's
    // count (AffineBandExtMode::ops), five more per register — the unsigned compare of the column against n, the compare with the
    // lane's row maximum, their and on the scalar side, two selects and the column's add — and 53 of overhead: four rounds of move,
    // DPP move, canonicalisation and max for the slot's row maximum (the maxima of moved values are canonicalised, those of results
    // of arithmetic are not), compare and select of the column's candidates, four rounds of move, DPP move and min for the column,
    // the freeze of the key, and the rule itself (row, the two diagonals, their distance and its conversion, multiply, add,
    // subtract, three compares, three selects, the ballot's compare).  5 R + 53 fits all eight instances to within one op
    return (20.0 * R + (R + 1) / 2 + 86.0) / (double)R;
  }
};

// Lemma L24, what the band kernel's stop test needs beyond L22 (affine_band_ext_exact): it compares r_i + d e with B - floor(zdrop).
// d is the distance of two in-band diagonals, at most W - 1; r_i + d e is an integer within (-2^24, smax m + (W - 1) e], and
// smax m + (W - 1) e < 2^24 follows from L22's 3o + (W + 1) e < 2^24 and smax (m + 1) < 2^18 for W <= 256 (o >= e).  B - floor(zdrop) lies
// in (-2^24, 2^18) where zdrop < 2^24.  B - r_i - d e is an integer, so it exceeds zdrop exactly where it exceeds floor(zdrop).
bool affine_band_zdrop_exact(float zdrop) { return zdrop < 16777216.0f; }

// The stop rule over rows 1..m-1 (include/mi355_sw.h "z-drop"): rmax[i-1] / rcol[i-1] = the maximum of row i over its in-band real
// columns (-inf: none) and its smallest column.  Returns rows_done: the stop row, or m.  Every operand is an integer below 2^25: exact
// in double.
int64_t affine_zdrop_stop_row(const float *rmax, const int32_t *rcol, int64_t m, double ext, double zdrop) {
  double B = 0.0; int64_t bdiag = 0;                               // the anchor (0, 0)
  for (int64_t i = 1; i < m; ++i) {
    const double r = rmax[i - 1];
    if (r > B) { B = r; bdiag = (int64_t)rcol[i - 1] - i; continue; }
    if (r == -INFINITY) return i;
    const int64_t cd = (int64_t)rcol[i - 1] - i, d = bdiag > cd ? bdiag - cd : cd - bdiag;
    if (B - r - (double)d * ext > zdrop) return i;
  }
  return m;
}
// The same on an empty window: row i is the border cell (i, 0) = -(o + (i-1) e) where -i >= band_lo, so B stays 0 at the anchor, d = i
// and the test reads o - e > zdrop in every row; a row below the band has no cell and stops.
int64_t affine_zdrop_stop_row_border(int64_t m, int64_t band_lo, double open, double ext, double zdrop) {
  if (m < 2) return m;
  if (open - ext > zdrop) return 1;
  return band_lo > -m + 1 ? -band_lo + 1 : m;                      // the first row i with -i < band_lo, where that is below m
}

// First step of the exact path under the stop rule: sw_affine_exact_rows_band_kernel over `jobs` (banded items on their clipped
// windows), the rule on the host, and m := rows_done in the job — the second step is affine_ext_exact_stage<true> on what is left.
int affine_ext_rows_stage(const AffineCall &c, std::vector<AffineExtItem> &jobs, int64_t *rows_done) {
  mi355_sw_ctx *ctx = c.ctx;
  if (jobs.empty()) return 0;
  path_note(ctx, "affine_exact_band_rows");
  AffineScoring sc;
  { int rc = affine_scoring(ctx, c.p, sc); if (rc) return rc; }
  HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
  for (size_t lo = 0; lo < jobs.size();) {
    size_t hi = lo, lds = 0, words = 0;                            // a launch: at most 65536 problems and 2^24 row words
    while (hi < jobs.size() && hi - lo < 65536 && (hi == lo || words + 2 * (size_t)jobs[hi].m <= ((size_t)1 << 24))) {
      lds = std::max(lds, affine_exact_lds(jobs[hi].m, true)); words += 2 * (size_t)jobs[hi].m; ++hi;
    }
    const size_t n = hi - lo;
    if (ctx->probs.ensure(n * sizeof(ExactBandProblem)) || ctx->hmat.ensure(words * 4))
      return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(exact scratch) failed");
    std::vector<ExactBandProblem> pr(n);
    size_t at = 0;
    for (size_t k = 0; k < n; ++k) {
      const AffineExtItem &j = jobs[lo + k];
      memset(&pr[k], 0, sizeof pr[k]);
      pr[k].blo = j.blo; pr[k].bhi = j.bhi;
      ExactProblem &e = pr[k].e;
      e.x = j.x; e.y = j.ybytes; e.m = j.m; e.nw = (int32_t)j.n; e.full_n = j.n; e.own_lo = 1; e.target = -1.0f;
      e.hout = ctx->hmat.as<float>() + at; at += 2 * (size_t)j.m;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->probs.p, pr.data(), n * sizeof(ExactBandProblem), hipMemcpyHostToDevice, ctx->stream));
    launch_dyn_lds(&sw_affine_exact_rows_band_kernel, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->probs.as<ExactBandProblem>(), sc);
    HIPCHK(ctx, hipGetLastError());
    ctx->exact_launches += 1;
    std::vector<float> rows(words);
    std::vector<int32_t> cols;
    HIPCHK(ctx, hipMemcpyAsync(rows.data(), ctx->hmat.p, words * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    at = 0;
    for (size_t k = 0; k < n; ++k) {
      AffineExtItem &j = jobs[lo + k];
      const int64_t m = j.m;
      static_assert(sizeof(int32_t) == sizeof(float), "the columns travel as bits");
      cols.resize((size_t)m);
      memcpy(cols.data(), rows.data() + at + m, (size_t)m * 4);
      const int64_t s = affine_zdrop_stop_row(rows.data() + at, cols.data(), m, (double)c.t.ext, (double)c.zdrop);
      at += 2 * (size_t)m;
      rows_done[j.id] = s;
      if (s < m) {                                                 // the truncated pair: its rows, its window clipped again, the same band
        j.m = (int32_t)s;
        j.n = std::min<int64_t>(j.n, s + j.bhi); j.bhi = (int32_t)std::min<int64_t>(j.bhi, j.n);
      }
    }
    lo = hi;
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
  ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  return 0;
}

// sw_affine_exact_ext_kernel over all of `jobs`, 65536 per launch: score[npairs][2], ends[npairs][2][2] as the list stage; its
// interval goes to timings[1].
// BAND: sw_affine_exact_ext_band_kernel over jobs that carry their band (AffineExtItem::blo, bhi) and their clipped window.
// GLOB (affine_global): sw_affine_exact_glob_kernel, one result per problem — score[npairs], ends[npairs][2].
template <bool BAND = false, bool GLOB = false>
int affine_ext_exact_stage(const AffineCall &c, const std::vector<AffineExtItem> &jobs, float *score, int64_t *ends) {
  typedef typename AffineExactProblemOf<BAND>::type Problem;
  constexpr size_t NO = GLOB ? 1 : 2;                              // (best, cell) a problem writes
  mi355_sw_ctx *ctx = c.ctx;
  if (jobs.empty()) return 0;
  path_note(ctx, BAND ? "affine_exact_band" : "affine_exact");
  AffineScoring sc;
  { int rc = affine_scoring(ctx, c.p, sc); if (rc) return rc; }
  HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
  for (size_t lo = 0; lo < jobs.size(); lo += 65536) {
    const size_t n = std::min<size_t>(65536, jobs.size() - lo);
    size_t lds = 0;
    for (size_t k = 0; k < n; ++k) lds = std::max(lds, affine_exact_lds(jobs[lo + k].m));
    if (ctx->probs.ensure(n * sizeof(Problem)) || ctx->outs_f.ensure(NO * n * 4) || ctx->outs_i.ensure(NO * n * 16))
      return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(exact scratch) failed");
    std::vector<Problem> pr(n);
    for (size_t k = 0; k < n; ++k) {
      const AffineExtItem &j = jobs[lo + k];
      memset(&pr[k], 0, sizeof pr[k]);
      ExactProblem *ep;
      if constexpr (BAND) { ep = &pr[k].e; pr[k].blo = j.blo; pr[k].bhi = j.bhi; } else ep = &pr[k];
      ExactProblem &e = *ep;
      e.x = j.x; e.y = j.ybytes; e.m = j.m; e.nw = (int32_t)j.n; e.full_n = j.n; e.own_lo = 1; e.target = -1.0f;
      e.best = ctx->outs_f.as<float>() + NO * k;
      e.cell = ctx->outs_i.as<int64_t>() + 2 * NO * k;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->probs.p, pr.data(), n * sizeof(Problem), hipMemcpyHostToDevice, ctx->stream));
    if constexpr (GLOB) launch_dyn_lds(&sw_affine_exact_glob_kernel<BAND>, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->probs.as<Problem>(), sc);
    else if constexpr (BAND) launch_dyn_lds(&sw_affine_exact_ext_band_kernel, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->probs.as<Problem>(), sc);
    else launch_dyn_lds(&sw_affine_exact_ext_kernel, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->probs.as<ExactProblem>(), sc);
    HIPCHK(ctx, hipGetLastError());
    ctx->exact_launches += 1;
    std::vector<float> bf(NO * n);
    std::vector<int64_t> ci(2 * NO * n);
    HIPCHK(ctx, hipMemcpyAsync(bf.data(), ctx->outs_f.p, NO * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ci.data(), ctx->outs_i.p, NO * n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < n; ++k) {
      const size_t id = jobs[lo + k].id;
      for (size_t v = 0; v < NO; ++v) score[NO * id + v] = bf[NO * k + v];
      for (size_t v = 0; v < 2 * NO; ++v) ends[2 * NO * id + v] = ci[2 * NO * k + v];
    }
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
  ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  return 0;
}

// Traceback of pair k from the cell (tx[k], ty[k]) of value ts[k]: one sw_affine_trace_ext_kernel problem over the whole rectangle
// from the anchor to that cell, in launch groups of at most kAffineTraceDirsMax decision bytes.  A cell in column 0 (the letters of
// x against as many '-') is written here from a copy of the letters: no kernel runs.  tout[npairs]: views into ctx->arenas.
// BAND: the banded pairs on sw_affine_trace_ext_band_kernel, the others on today's — one pass each (affine_extend); the pass without
// BAND writes the column-0 cells of both kinds (no kernel runs for them, and the whole of column 0 up to an in-band cell is in band).
template <bool BAND = false>
int affine_ext_trace(const AffineCall &c, const std::vector<AffineExtItem> &pairs, const float *ts, const int64_t *tx, const int64_t *ty,
                     std::vector<TraceOut> &tout) {
  typedef typename AffineTraceProblemOf<BAND>::type Problem;
  mi355_sw_ctx *ctx = c.ctx;
  struct Job { size_t k; size_t dirs_off, cons_off; };
  std::vector<Job> jobs;
  std::vector<size_t> col0;                                        // pairs traced from a cell in column 0
  size_t col0_bytes = 0;
  for (size_t k = 0; k < pairs.size(); ++k) {
    if (tx[k] < 1) continue;
    if (ty[k] < 1) { if (!BAND) { col0.push_back(k); col0_bytes += 2 * (size_t)tx[k]; } continue; }
    if (pairs[k].banded != BAND) continue;
    if (dirs_bytes(tx[k], ty[k]) > kAffineTraceDirsMax || affine_exact_lds((int)std::min<int64_t>(tx[k], 1 << 24)) > kExactLdsMax) {
      char msg[240];
      std::snprintf(msg, sizeof msg, "affine extension traceback: pair %zu needs a rectangle of %lld rows x %lld columns, more than %zu "
                    "decision bytes or more rows than the exact kernel's LDS diagonals hold", k, (long long)tx[k], (long long)ty[k], kAffineTraceDirsMax);
      return fail(ctx, MI355_SW_ENOTSUP, msg);
    }
    jobs.push_back(Job{k, 0, 0});
  }
  if (!col0.empty()) {                                             // one arena, one copy per pair, one wait for all of them
    std::vector<char> cons(col0_bytes, '-');
    size_t at = 0;
    hipError_t copied = hipSuccess;
    for (size_t k : col0) {
      copied = hipMemcpyAsync(cons.data() + at, pairs[k].x, (size_t)tx[k], hipMemcpyDeviceToHost, ctx->stream);
      if (copied != hipSuccess) break;
      at += 2 * (size_t)tx[k];
    }
    const hipError_t waited = hipStreamSynchronize(ctx->stream);    // (before `cons` can go: copies may be in flight)
    HIPCHK(ctx, copied);
    HIPCHK(ctx, waited);
    ctx->arenas.push_back(std::move(cons));
    char *base = ctx->arenas.back().data();
    at = 0;
    for (size_t k : col0) {
      const size_t len = (size_t)tx[k];
      std::reverse(base + at, base + at + len);                     // from the far end to the anchor
      TraceOut &o = tout[k];
      o.len = len; o.cx = base + at; o.cy = base + at + len; o.pos = 0;
      at += 2 * len;
    }
  }
  if (jobs.empty()) return 0;
  path_note(ctx, "affine_trace");
  AffineScoring sc;
  { int rc = affine_scoring(ctx, c.p, sc); if (rc) return rc; }
  for (size_t lo = 0; lo < jobs.size();) {
    size_t hi = lo, dirs_total = 0, cons_total = 0, lds = 0;
    while (hi < jobs.size() && hi - lo < 65536) {
      Job &j = jobs[hi];
      const size_t db = (dirs_bytes(tx[j.k], ty[j.k]) + 15) & ~(size_t)15;
      if (hi > lo && dirs_total + db > kAffineTraceDirsMax) break;
      j.dirs_off = dirs_total; dirs_total += db;
      j.cons_off = cons_total; cons_total += 2 * ((size_t)tx[j.k] + (size_t)ty[j.k]);
      lds = std::max(lds, affine_exact_lds((int)tx[j.k]));
      ++hi;
    }
    const size_t n = hi - lo;
    if (ctx->wprobs.ensure(n * sizeof(Problem)) || ctx->walkp.ensure(n * 24) || ctx->dirs.ensure(dirs_total) ||
        ctx->cons.ensure(cons_total + 16))
      return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(affine traceback scratch) failed");
    std::vector<Problem> pr(n);
    for (size_t k = 0; k < n; ++k) {
      const Job &j = jobs[lo + k];
      memset(&pr[k], 0, sizeof pr[k]);
      AffineTraceProblem *ap;
      if constexpr (BAND) { ap = &pr[k].t; pr[k].blo = pairs[j.k].blo; pr[k].bhi = pairs[j.k].bhi; } else ap = &pr[k];
      AffineTraceProblem &a = *ap;
      a.e.x = pairs[j.k].x; a.e.y = pairs[j.k].ybytes;
      a.e.m = (int32_t)tx[j.k]; a.e.nw = (int32_t)ty[j.k];
      a.e.own_lo = 1;
      a.e.target = ts[j.k];
      a.e.dirs = ctx->dirs.as<uint8_t>() + j.dirs_off;
      a.cap = a.e.m + a.e.nw;
      a.cons_x = ctx->cons.as<char>() + j.cons_off;
      a.cons_y = a.cons_x + a.cap;
      a.clamped = 1; a.row_clamped = 1;
      a.out = ctx->walkp.as<int64_t>() + 3 * k;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->wprobs.p, pr.data(), n * sizeof(Problem), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[6], ctx->stream));
    if constexpr (BAND) launch_dyn_lds(&sw_affine_trace_ext_band_kernel, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->wprobs.as<Problem>(), sc);
    else launch_dyn_lds(&sw_affine_trace_ext_kernel, dim3((unsigned)n), dim3(64), lds, ctx->stream, ctx->wprobs.as<AffineTraceProblem>(), sc);
    HIPCHK(ctx, hipGetLastError());
    ctx->trace_launches += 1;
    HIPCHK(ctx, hipEventRecord(ctx->ev[7], ctx->stream));
    std::vector<int64_t> wo(3 * n);
    std::vector<char> cons(cons_total);
    HIPCHK(ctx, hipMemcpyAsync(wo.data(), ctx->walkp.p, n * 24, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cons.data(), ctx->cons.p, cons_total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timings[2] += elapsed_us(ctx, ctx->ev[6], ctx->ev[7]);
    ctx->arenas.push_back(std::move(cons));
    const char *base = ctx->arenas.back().data();
    for (size_t k = 0; k < n; ++k) {
      const Job &j = jobs[lo + k];
      const int64_t st = wo[3 * k + 2];
      if (st == 2) return fail(ctx, MI355_SW_ENODEV, "internal: the affine extension traceback exceeded its string capacity");
      if (st != 0) return fail(ctx, MI355_SW_ENODEV, "internal: the traced cell of the affine extension does not hold its score");
      TraceOut &o = tout[j.k];
      o.len = (size_t)wo[3 * k];
      o.cx = base + j.cons_off;
      o.cy = base + j.cons_off + (size_t)tx[j.k] + (size_t)ty[j.k];
      o.pos = (uint32_t)wo[3 * k + 1];
    }
    lo = hi;
  }
  return 0;
}

// The pairs of `el` under the anchored model.  score[npairs][2] = best extension, to-end score; ends[npairs][2][2] = end_x, end_y
// (lengths), then m, to_end_y.  tout (may be null): the traceback of every pair, from the best extension's cell or, where
// to_end[k] != 0 (to_end may be null), from (m, to_end_y).  A pair runs on sw_affine_pair_ext_kernel while rows, columns, table and
// admission (affine_ext_exact) allow, else as a whole problem of the exact kernel; an empty window is filled in here.
// With bands (el.band_lo): a pair whose clipped band covers its matrix takes that same route; every other pair is a banded pair on its
// clipped window — sw_affine_band_ext_kernel while rows, diagonals, table and admission (affine_band_ext_exact) allow and option
// no_affine_band is off, else the exact kernel under the band — and never runs on an unbanded kernel.  The stages run in a fixed
// order: the pair kernel, the band kernel, the exact kernel's unbanded and then its banded jobs, the two passes of the traceback.
// zdrop < +inf (the z-drop calls; bands required, the caller checks): the stop rule of include/mi355_sw.h "z-drop" (DESIGN.md §3.8,
// L24).  rows_done[npairs] (may be null): the stop row of pair k, or m.  Every pair with m, n >= 1 is then a banded pair, a band that
// covers the matrix included: sw_affine_band_extz_kernel where the band kernel admits the pair and zdrop (affine_band_zdrop_exact),
// else the exact path in two steps — the rows instance and the rule on the host (affine_ext_rows_stage), then the exact kernel under
// the band on the first rows_done rows.  A pair that stopped never reached its row m: its to-end half is the `unreach` overwrite.  An
// empty window is the rule on the border column, here.  zdrop = +inf changes nothing: rows_done = m.
int affine_extend(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const AffineExtList &el, const mi355_sw_affine_params &p,
                  const uint8_t *to_end, float *score, int64_t *ends, std::vector<TraceOut> *tout, float zdrop = INFINITY,
                  int64_t *rows_done = nullptr) {
  const size_t npairs = el.npairs;
  for (size_t k = 0; k < 2 * npairs; ++k) { score[k] = 0.0f; ends[2 * k] = 0; ends[2 * k + 1] = 0; }
  if (tout) tout->assign(npairs, TraceOut());
  if (npairs > 0xFFFFFFFFull) return fail(ctx, MI355_SW_ENOTSUP, "affine extension: more than 2^32 pairs");
  AffineCall c{ctx, ref, q, p, AffineTable(), kAffineModeExt};
  c.zdrop = zdrop;
  int rc = affine_begin(c);
  if (rc) return rc > 0 ? 0 : rc;
  AffineProfPlan plan;
  const bool table_ok = affine_ext_plan(c, plan);
  rc = affine_ext_any_reversed(c, el); if (rc) return rc;
  std::vector<int64_t> own_rows_done;
  if (!rows_done && c.zd()) { own_rows_done.resize(npairs); rows_done = own_rows_done.data(); }
  std::vector<AffineExtItem> zfast;                                // z-drop: the banded pairs of sw_affine_band_extz_kernel

  std::vector<AffineExtItem> pairs(npairs), fast, jobs;
  std::vector<AffineExtItem> bfast, bjobs;                         // banded pairs of sw_affine_band_ext_kernel, and of the exact kernel under a band
  std::vector<char> unreach(el.band_lo ? npairs : 0, 0);           // the band misses row m: the host fills in to_end
  int mmax = 0, band_mmax = 0;
  for (size_t k = 0; k < npairs; ++k) {
    AffineExtItem &it = pairs[k];
    it = affine_ext_item(c, el, k);
    const int64_t m = it.m, n = it.n;
    if (rows_done) rows_done[k] = m;
    if (m < 1) continue;
    if (el.band_lo) {
      // the band clipped to the matrix; one that covers it leaves the pair unbanded: today's route below, today's bytes
      const int64_t lo_e = std::max(el.band_lo[k], -m), hi_e = std::min(el.band_hi[k], n);
      if (c.zd() && n < 1) {                                       // z-drop on an empty window: the rule on the border column
        const int64_t s = affine_zdrop_stop_row_border(m, el.band_lo[k], (double)c.t.open, (double)c.t.ext, (double)c.zdrop);
        if (s < m) { rows_done[k] = s; unreach[k] = 1; continue; } // nothing to extend, the end not reached: the zeros stand
      }
      if ((c.zd() && n >= 1) || lo_e != -m || hi_e != n) {         // (z-drop: a band that covers the matrix stays a band)
        const bool reach = lo_e <= n - m;                          // row m holds an in-band cell
        if (!reach) unreach[k] = 1;
        if (n < 1) continue;                                       // (lo_e > -m: unreachable) nothing to extend: the zeros stand
        // columns beyond m + hi_e are out of band in every row: the window is clipped before anything is sized
        const int64_t nc = std::min(n, m + hi_e), W = hi_e - lo_e + 1;
        it.n = nc; it.banded = true; it.blo = (int32_t)lo_e; it.bhi = (int32_t)std::min(hi_e, nc); it.W = (int32_t)std::min<int64_t>(W, 0x7fffffff);
        if (table_ok && !opt().no_affine_band && m <= kBandRowsMax && affine_band_R(W) != 0 && affine_band_ext_exact(c.t, (double)m, (double)W) &&
            (!c.zd() || affine_band_zdrop_exact(c.zdrop))) {
          (c.zd() ? zfast : bfast).push_back(it); band_mmax = std::max(band_mmax, (int)m);
          continue;
        }
        if (c.zd() && m > kAffineExactRowsMax) {
          char msg[480];
          std::snprintf(msg, sizeof msg, "affine extension with z-drop: banded pair %zu (%lld rows, %lld diagonals) is outside the band kernel (1..512 rows, "
                        "at most 256 diagonals, zdrop < 2^24%s) and has more rows than the rows instance of the exact kernel holds (at most %d rows: a "
                        "maximum and a column per row beside the LDS diagonals)", k, (long long)m, (long long)W,
                        opt().no_affine_band ? "; option no_affine_band is set" : opt().no_affine_pairs ? "; option no_affine_pairs is set" : "",
                        kAffineExactRowsMax);
          return fail(ctx, MI355_SW_ENOTSUP, msg);
        }
        if ((double)m * (double)nc > kAffineExactCellsMax || !affine_band_ext_whole_exact(c.t, (double)m, (double)W) || affine_exact_lds((int)m) > kExactLdsMax) {
          char msg[800];
          std::snprintf(msg, sizeof msg, "affine extension: banded pair %zu (%lld rows x %lld columns, clipped to %lld; %lld diagonals) is outside the band "
                        "kernel (1..512 rows, at most 256 diagonals, a rows + 3 gap_open + (diagonals + 1) gap_extend - min(smin, 0) < 2^24 with a = "
                        "max(-smin, 0), smax * (rows + 1) < 2^18, a score table within 32 KiB%s) and outside the exact kernel under a band (at most "
                        "2^26 cells of rows x clipped columns and 5600 rows, a rows + 2 gap_open + diagonals gap_extend - min(smin, 0) < 2^24, "
                        "smax * (rows + 1) < 2^24)", k, (long long)m,
                        (long long)n, (long long)nc, (long long)W,
                        opt().no_affine_band ? "; option no_affine_band is set" : opt().no_affine_pairs ? "; option no_affine_pairs is set" : "");
          return fail(ctx, MI355_SW_ENOTSUP, msg);
        }
        bjobs.push_back(it);
        continue;
      }
    }
    if (n < 1) {                                                   // the whole of x as one insertion; nothing to extend
      score[2 * k + 1] = -((float)c.t.open + (float)(m - 1) * (float)c.t.ext);
      ends[4 * k + 2] = m;
      continue;
    }
    if (table_ok && m <= kMaxRowsFast && n <= kAffinePairColsMax && affine_ext_exact(c.t, (double)m, (double)n)) {
      fast.push_back(it); mmax = std::max(mmax, (int)m);
      continue;
    }
    if ((double)m * (double)n > kAffineExactCellsMax || !affine_ext_whole_exact(c.t, (double)m, (double)n) || affine_exact_lds((int)m) > kExactLdsMax) {
      char msg[400];
      std::snprintf(msg, sizeof msg, "affine extension: pair %zu (%lld rows x %lld columns) is outside the pair kernel (1..512 rows, 1..2^20 columns, "
                    "3 gap_open + (rows + columns) gap_extend - min(smin, 0) < 2^24, smax * (rows + 1) < 2^18, a score table within 32 KiB%s) and "
                    "outside the exact kernel (at most 2^26 cells and 5600 rows, 3 gap_open + (rows + columns) gap_extend < 2^24)", k,
                    (long long)m, (long long)n, opt().no_affine_pairs ? "; option no_affine_pairs is set" : "");
      return fail(ctx, MI355_SW_ENOTSUP, msg);
    }
    jobs.push_back(it);
  }
  rc = affine_list_stage(AffinePairFamily<AffineExtMode>{c, {}}, plan, fast, mmax, score, ends);
  if (!rc) rc = affine_list_stage(AffineBandFamily<AffineBandExtMode>{c, {}}, plan, bfast, band_mmax, score, ends);
  if (!rc && !zfast.empty()) {
    // rows_done from where the other mode writes m (the stage also brings down the counter zdrop_rows_run)
    rc = affine_list_stage(AffineBandFamily<AffineBandExtZMode>{c, {}}, plan, zfast, band_mmax, score, ends);
    if (rc) return rc;
    for (const AffineExtItem &it : zfast) rows_done[it.id] = ends[4 * (size_t)it.id + 2];
  }
  if (!rc) rc = affine_ext_exact_stage(c, jobs, score, ends);
  if (!rc && c.zd()) rc = affine_ext_rows_stage(c, bjobs, rows_done);
  if (!rc) rc = affine_ext_exact_stage<true>(c, bjobs, score, ends);
  if (rc) return rc;
  if (c.zd())
    for (size_t k = 0; k < npairs; ++k)
      if (rows_done[k] < pairs[k].m) { unreach[k] = 1; ctx->zdrop_stopped += 1; }   // stopped: the read's end was not reached
  // a read whose end the band cannot reach: no kernel decides this.  Such a pair still ran on its kernel above, for the best
  // extension; what that kernel wrote for the to-end half (-inf / -1 as it happens) is deliberately ignored and overwritten here, so
  // that the header's rule band_lo > n - m alone decides.  Keep the overwrite.  Traced to the end the pair is an empty alignment
  // (row 0 of `ends`: affine_ext_trace skips it)
  for (size_t k = 0; k < unreach.size(); ++k)
    if (unreach[k]) { score[2 * k + 1] = -INFINITY; ends[4 * k + 2] = 0; ends[4 * k + 3] = -1; }
  if (tout) {
    std::vector<float> ts(npairs);
    std::vector<int64_t> tx(npairs), ty(npairs);
    for (size_t k = 0; k < npairs; ++k) {
      const size_t w = (to_end && to_end[k]) ? 1 : 0;
      ts[k] = score[2 * k + w]; tx[k] = ends[4 * k + 2 * w]; ty[k] = ends[4 * k + 2 * w + 1];
    }
    rc = affine_ext_trace(c, pairs, ts.data(), tx.data(), ty.data(), *tout);
    if (!rc && (!bfast.empty() || !zfast.empty() || !bjobs.empty())) rc = affine_ext_trace<true>(c, pairs, ts.data(), tx.data(), ty.data(), *tout);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
  ctx->timings[3] += elapsed_us(ctx, ctx->ev[4], ctx->ev[5]);
  return 0;
}

// ---- global alignment between two anchors (include/mi355_sw.h "global alignment between two anchors", DESIGN.md §3.8 lemma L23) ----
// sw_affine_pair_glob_kernel: AffineExtMode's items, one result per problem, the corner H(m, n).
struct AffineGlobMode {
  typedef AffineOwnItem Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_pair_glob_kernel instance for this query";
  static constexpr int kOuts = 1;
  static bool keep_all(const AffineCall &) { return true; }        // the corner's value may have any sign
  template <int R> static auto kernel(const AffineCall &) { return &sw_affine_pair_glob_kernel<R>; }
  static const char *path(const AffineCall &) { return "affine_pair_glob[R=%d]"; }
  static const char *name(const AffineCall &) { return "sw_affine_pair_glob_kernel<R=%d>"; }
  static double ops(const AffineCall &, int R) {
    // per step and lane, counted in the compiled steady-state loop (four steps, every R of kPairR): the extension instance's count
    // (AffineExtMode::ops) without the max with 0, the key's v_or and the maximum3 fold — seven ops, the table address' v_add and
    // the row-m select per cell — and 10.5 of overhead: the two DPP moves and their copies, the row pointer's multiply and add, the
    // code's address, the row-0 subtract and max, the capture's compare.  The compiler puts the capture behind an exec-mask branch
    // that a wavefront takes when one of its lanes stands on its column n, and moves a quarter of the selects out of line with it:
    // 8.75 R + 10.5 fits all six instances to within half an op.  The 16 border steps of a slot are not counted
    return (8.75 * R + 10.5) / (double)R;
  }
};

// sw_affine_band_glob_kernel: AffineBandExtMode's items (the window is never clipped: a band that holds the corner has
// n <= m + hi_e), one result per problem.
struct AffineBandGlobMode {
  typedef AffineOwnItem Source;
  static constexpr const char *kNoInstance = "internal: no sw_affine_band_glob_kernel instance for this band";
  static constexpr int kOuts = 1;
  static bool keep_all(const AffineCall &) { return true; }
  template <int R> static auto kernel(const AffineCall &) { return &sw_affine_band_glob_kernel<R>; }
  static const char *path(const AffineCall &) { return "affine_band_glob[R=%d]"; }
  static const char *name(const AffineCall &) { return "sw_affine_band_glob_kernel<R=%d>"; }
  static double ops(const AffineCall &, int R) {
    // per step and lane, counted in the compiled loop (every R of kBandR, to within five ops of a step): the extension instance's
    // count (AffineBandExtMode::ops) without the max with 0 and the key's v_or per register and without the step's (value, column)
    // compare — thirteen ops per register, a move per two registers, and 26 of overhead.  The corner's read (one compare and one
    // select per register) runs behind the branch, at one step of a slot's rows: not counted
    return (13.0 * R + (R + 1) / 2 + 26.0) / (double)R;
  }
};

// The pairs traced from a cell in row 0 (tx = 0, ty >= 1: an empty x against a window of ty columns, ty '-' against its letters) are
// written here from a copy of the window's bytes: no kernel runs, and affine_ext_trace skips them.  One arena, one copy per pair, one
// wait for all of them, as that function's column-0 cells.
int affine_glob_row0_fill(const AffineCall &c, const std::vector<AffineExtItem> &pairs, const int64_t *tx, const int64_t *ty,
                          std::vector<TraceOut> &tout) {
  mi355_sw_ctx *ctx = c.ctx;
  std::vector<size_t> row0;
  size_t bytes = 0;
  for (size_t k = 0; k < pairs.size(); ++k)
    if (tx[k] < 1 && ty[k] >= 1) { row0.push_back(k); bytes += 2 * (size_t)ty[k]; }
  if (row0.empty()) return 0;
  std::vector<char> cons(bytes, '-');
  size_t at = 0;
  hipError_t copied = hipSuccess;
  for (size_t k : row0) {
    copied = hipMemcpyAsync(cons.data() + at + (size_t)ty[k], pairs[k].ybytes, (size_t)ty[k], hipMemcpyDeviceToHost, ctx->stream);
    if (copied != hipSuccess) break;
    at += 2 * (size_t)ty[k];
  }
  const hipError_t waited = hipStreamSynchronize(ctx->stream);      // (before `cons` can go: copies may be in flight)
  HIPCHK(ctx, copied);
  HIPCHK(ctx, waited);
  ctx->arenas.push_back(std::move(cons));
  char *base = ctx->arenas.back().data();
  at = 0;
  for (size_t k : row0) {
    const size_t len = (size_t)ty[k];
    std::reverse(base + at + len, base + at + 2 * len);             // from the far end to the anchor
    TraceOut &o = tout[k];
    o.len = len; o.cx = base + at; o.cy = base + at + len; o.pos = 1;
    at += 2 * len;
  }
  return 0;
}

// The pairs of `el` under the anchored model, anchored at BOTH ends: score[npairs] = H(m, n), -INFINITY where the pair's band misses
// the corner; tout (may be null): the traceback of every pair from (m, n).  Items, class table, reversed copies, the stage order (the
// pair kernel, the band kernel, the exact kernel's unbanded and then its banded jobs, the two passes of the traceback) and the bounds
// of the exact kernel are affine_extend's.  A pair runs on sw_affine_pair_glob_kernel while rows, columns, table and admission
// (affine_glob_exact) allow, under a band that does not cover its matrix on sw_affine_band_glob_kernel (affine_band_glob_exact, option
// no_affine_band off), else as a whole problem of the exact kernel; a banded pair never runs on an unbanded kernel.  A pair without
// rows or without columns, and a pair whose band misses the corner, is filled in here: no kernel runs for it.
int affine_global(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const AffineExtList &el, const mi355_sw_affine_params &p,
                  float *score, std::vector<TraceOut> *tout) {
  const size_t npairs = el.npairs;
  for (size_t k = 0; k < npairs; ++k) score[k] = 0.0f;
  if (tout) tout->assign(npairs, TraceOut());
  if (npairs > 0xFFFFFFFFull) return fail(ctx, MI355_SW_ENOTSUP, "affine global: more than 2^32 pairs");
  AffineCall c{ctx, ref, q, p, AffineTable(), kAffineModeExt};
  int rc = affine_begin(c);
  if (rc) return rc > 0 ? 0 : rc;
  AffineProfPlan plan;
  const bool table_ok = affine_ext_plan(c, plan);
  rc = affine_ext_any_reversed(c, el); if (rc) return rc;

  std::vector<AffineExtItem> pairs(npairs), fast, jobs, bfast, bjobs;
  std::vector<int64_t> ends(2 * npairs, 0), tx(npairs, 0), ty(npairs, 0);   // (tx, ty): the cell a pair is traced from; 0 / 0: nothing
  int mmax = 0, band_mmax = 0;
  const float go = (float)c.t.open, ge = (float)c.t.ext;
  for (size_t k = 0; k < npairs; ++k) {
    AffineExtItem &it = pairs[k];
    it = affine_ext_item(c, el, k);
    const int64_t m = it.m, n = it.n;
    if (el.band_lo && (el.band_lo[k] > n - m || el.band_hi[k] < n - m)) { score[k] = -INFINITY; continue; }   // the band misses the corner
    tx[k] = m; ty[k] = n;
    if (m < 1 || n < 1) {                                          // one gap, or nothing: H(m,0) / H(0,n) of the border
      const int64_t g = m + n;
      score[k] = g < 1 ? 0.0f : -(go + (float)(g - 1) * ge);
      continue;
    }
    const int64_t lo_e = el.band_lo ? std::max(el.band_lo[k], -m) : -m, hi_e = el.band_lo ? std::min(el.band_hi[k], n) : n;
    if (lo_e != -m || hi_e != n) {                                 // a banded pair; its window needs no clip: n <= m + hi_e
      const int64_t W = hi_e - lo_e + 1;
      it.banded = true; it.blo = (int32_t)lo_e; it.bhi = (int32_t)hi_e; it.W = (int32_t)std::min<int64_t>(W, 0x7fffffff);
      if (table_ok && !opt().no_affine_band && m <= kBandRowsMax && affine_band_R(W) != 0 && affine_band_glob_exact(c.t, (double)m, (double)W)) {
        bfast.push_back(it); band_mmax = std::max(band_mmax, (int)m);
        continue;
      }
      if ((double)m * (double)n > kAffineExactCellsMax || !affine_band_ext_whole_exact(c.t, (double)m, (double)W) || affine_exact_lds((int)m) > kExactLdsMax) {
        char msg[800];
        std::snprintf(msg, sizeof msg, "affine global: banded pair %zu (%lld rows x %lld columns, %lld diagonals) is outside the band kernel (1..512 rows, "
                      "at most 256 diagonals, a rows + 3 gap_open + (diagonals + 1) gap_extend - min(smin, 0) < 2^24 with a = max(-smin, 0), "
                      "smax * rows + gap_open < 2^24, a score table within 32 KiB%s) and outside the exact kernel under a band (at most 2^26 cells "
                      "and 5600 rows, a rows + 2 gap_open + diagonals gap_extend - min(smin, 0) < 2^24, smax * (rows + 1) < 2^24)", k,
                      (long long)m, (long long)n, (long long)W,
                      opt().no_affine_band ? "; option no_affine_band is set" : opt().no_affine_pairs ? "; option no_affine_pairs is set" : "");
        return fail(ctx, MI355_SW_ENOTSUP, msg);
      }
      bjobs.push_back(it);
      continue;
    }
    if (table_ok && m <= kMaxRowsFast && n <= kAffinePairColsMax && affine_glob_exact(c.t, (double)m, (double)n)) {
      fast.push_back(it); mmax = std::max(mmax, (int)m);
      continue;
    }
    if ((double)m * (double)n > kAffineExactCellsMax || !affine_ext_whole_exact(c.t, (double)m, (double)n) || affine_exact_lds((int)m) > kExactLdsMax) {
      char msg[400];
      std::snprintf(msg, sizeof msg, "affine global: pair %zu (%lld rows x %lld columns) is outside the pair kernel (1..512 rows, 1..2^20 columns, "
                    "3 gap_open + (rows + columns) gap_extend - min(smin, 0) < 2^24, smax * rows + gap_open < 2^24, a score table within 32 KiB%s) and "
                    "outside the exact kernel (at most 2^26 cells and 5600 rows, 3 gap_open + (rows + columns) gap_extend < 2^24)", k,
                    (long long)m, (long long)n, opt().no_affine_pairs ? "; option no_affine_pairs is set" : "");
      return fail(ctx, MI355_SW_ENOTSUP, msg);
    }
    jobs.push_back(it);
  }
  rc = affine_list_stage(AffinePairFamily<AffineGlobMode>{c, {}}, plan, fast, mmax, score, ends.data());
  if (!rc) rc = affine_list_stage(AffineBandFamily<AffineBandGlobMode>{c, {}}, plan, bfast, band_mmax, score, ends.data());
  if (!rc) rc = affine_ext_exact_stage<false, true>(c, jobs, score, ends.data());
  if (!rc) rc = affine_ext_exact_stage<true, true>(c, bjobs, score, ends.data());
  if (rc) return rc;
  if (tout) {
    rc = affine_ext_trace(c, pairs, score, tx.data(), ty.data(), *tout);
    if (!rc && (!bfast.empty() || !bjobs.empty())) rc = affine_ext_trace<true>(c, pairs, score, tx.data(), ty.data(), *tout);
    if (!rc) rc = affine_glob_row0_fill(c, pairs, tx.data(), ty.data(), *tout);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
  ctx->timings[3] += elapsed_us(ctx, ctx->ev[4], ctx->ev[5]);
  return 0;
}

}  // namespace
