// host_pipeline.h — the per-call pipeline: locate, traceback routing, whole-matrix path, align_range, range_maxima
// Part of the single translation unit mi355_sw.hip (included there, in order; not a standalone header).
namespace {

void set_result(mi355_sw_result &r, float score, int64_t ix, int64_t iy, const TraceOut *t) {
  r.score = score;
  r.end_x = score > 0 ? ix : 0;
  r.end_y = score > 0 ? iy : 0;
  r.pos = t ? t->pos : 0;
  const size_t len = t ? t->len : 0;
  r.cons_len = len;
  // both strings live in ONE allocation owned through cons_x (mi355_sw_free_result frees only that)
  r.cons_x = (char *)malloc(2 * len + 2);
  r.cons_y = r.cons_x + len + 1;
  if (len) { memcpy(r.cons_x, t->cx, len); memcpy(r.cons_y, t->cy, len); }
  r.cons_x[len] = 0;
  r.cons_y[len] = 0;
}

// Traceback for located alignments of one range: windows left of the argmax, grown on demand.
int trace_located(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
                  const mi355_sw_params &p, const std::vector<int64_t> &qwarm, const ScoreTable &table,
                  const std::vector<int> &qidx, const std::vector<Located> &loc, std::vector<TraceOut> &tout) {
  tout.assign(qidx.size(), TraceOut());
  // A cell in row i is exact once it lies i + ceil(i * smax / g) columns into a window (lemma L2: the bound
  // for a path that can only use rows 1..i), so the window needs that margin at the argmax row plus room
  // for the horizontal excursions of the walk; the walk kernel checks every cell it visits against the bound.
  const Margin mg = table.margin(q.maxlen);
  const float slope = (float)mg.slope();
  auto row_need = [&](int64_t i) { return mg.finite() ? clamp_cols((double)i + std::ceil((double)i * (double)slope) + 2.0) : kColsMax; };
  std::vector<size_t> todo;
  // short reads with identity scoring: decisions by the register-wavefront kernel (lanes = rows of x);
  // long queries (identity scoring, or any table in the float engine): the pipelined strip kernel
  const bool wave_ok = wave_scoring_ok(p) && !opt().no_wave;
  const bool strip_ok = strip_scoring_ok(ref, p);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int> sub;
    std::vector<Located> sl;
    std::vector<size_t> owner;
    for (size_t k = 0; k < qidx.size(); ++k) {
      if (!(loc[k].score > 0)) continue;
      const bool is_long = q.len[qidx[k]] > kWaveMaxLanesSide;
      if (is_long != (pass == 1)) continue;
      if (is_long ? strip_ok : wave_ok) { sub.push_back(qidx[k]); sl.push_back(loc[k]); owner.push_back(k); }
      else todo.push_back(k);
    }
    // a lone long query whose sweep saved its columns / strip rows (host_saved.h): decisions from stored exact values, one
    // block per (strip, sub-chunk) the walk can reach; what the walk's checks refuse takes the zero-border windows below
    if (pass == 1 && q.nq == 1 && sub.size() == 1) {
      const int sr = saved_range_index(ctx, ref, q, rg, p, sub[0]);
      if (sr >= 0) {
        TraceOut t1;
        const int rc1 = trace_from_saved(ctx, ref, q, rg, p, sr, sub[0], sl[0], table, t1);
        if (rc1 < 0) return rc1;
        if (rc1 == 0) { tout[owner[0]] = t1; continue; }
        ctx->saved_fallbacks += 1;
      }
    }
    if (sub.empty()) continue;
    std::vector<TraceOut> t2;
    const bool latency_mode = pass == 0 && sub.size() <= kLatencyJobs && strip_ok;
    int rc = wave_trace(ctx, ref, q, rg, p, 0, sub, sl, t2, pass == 1 || latency_mode, &table);
    if (rc) return rc;
    for (size_t t = 0; t < sub.size(); ++t) tout[owner[t]] = std::move(t2[t]);
  }
  std::vector<int64_t> budget(qidx.size());
  for (size_t k : todo) budget[k] = (int64_t)q.len[qidx[k]] / 8 + 64;
  while (!todo.empty()) {
    // build jobs in memory-bounded groups
    std::vector<size_t> next;
    size_t pos = 0;
    while (pos < todo.size()) {
      std::vector<ExactJob> jobs;
      std::vector<size_t> owner;
      std::vector<std::pair<int32_t, int32_t>> starts;
      std::vector<int32_t> exlo;
      size_t bytes = 0;
      while (pos < todo.size()) {
        const size_t k = todo[pos];
        const int qi = qidx[k];
        const int64_t iy = loc[k].iy;
        const int64_t warm = qwarm[qi];
        int64_t wl = iy - (budget[k] + row_need(loc[k].ix));   // range-relative 0-based start of window
        if (wl < 0) wl = 0;
        const int64_t nw = iy - wl;
        const size_t need = dirs_bytes(q.len[qi], nw) + 16;
        if (need > kDirsBudget) return fail(ctx, MI355_SW_ENOTSUP, "traceback window exceeds the device scratch budget");
        if (!jobs.empty() && bytes + need > kDirsBudget) break;
        ExactJob j;
        j.q = qi; j.ylo = rg.lo + wl; j.nw = (int32_t)nw; j.col_offset = wl; j.full_n = rg.hi - rg.lo;
        j.own_lo = (int32_t)(nw + 1);                   // nothing competes: decisions only
        j.quirk = 0;                                    // |x| == |y| never reaches the score path (bucket_fast_ok)
        j.target = 1e30f; j.want_dirs = true;
        jobs.push_back(j); owner.push_back(k);
        starts.emplace_back((int32_t)loc[k].ix, (int32_t)nw);
        exlo.push_back(wl == 0 ? 0 : (int32_t)warm);
        bytes += need;
        ++pos;
      }
      int rc = run_exact(ctx, ref, q, p, jobs, 0, jobs.size(), nullptr);
      if (rc) return rc;
      std::vector<TraceOut> outs;
      std::vector<int> st;
      rc = run_walk(ctx, ref, q, jobs, 0, jobs.size(), starts, exlo, outs, st, slope);
      if (rc) return rc;
      for (size_t t = 0; t < jobs.size(); ++t) {
        const size_t k = owner[t];
        if (st[t] == 0) tout[k] = std::move(outs[t]);
        else if (st[t] == 1) { budget[k] *= 4; ctx->walk_widened += 1; next.push_back(k); }
        else return fail(ctx, MI355_SW_ENOTSUP, "consensus longer than |x| + window");
      }
    }
    todo.swap(next);
  }
  return 0;
}

// Whole-matrix path on the LDS anti-diagonal kernel (sw_exact_kernel.h) for the listed queries over one range.
int exact_full_lds(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
                   const mi355_sw_params &p, const std::vector<int> &qidx, bool want_trace,
                   std::vector<Located> &loc, std::vector<TraceOut> &tout) {
  const int64_t n = rg.hi - rg.lo;
  loc.assign(qidx.size(), Located());
  tout.assign(qidx.size(), TraceOut());
  size_t pos = 0;
  while (pos < qidx.size()) {
    std::vector<ExactJob> jobs;
    std::vector<size_t> owner;
    size_t bytes = 0;
    while (pos < qidx.size()) {
      const int qi = qidx[pos];
      const size_t need = dirs_bytes(q.len[qi], n) + 16;
      if (want_trace && need > kDirsBudget) return fail(ctx, MI355_SW_ENOTSUP, "problem needs the score kernel but is outside its coverage");
      if (!jobs.empty() && want_trace && bytes + need > kDirsBudget) break;
      if (jobs.size() >= 65536) break;
      ExactJob j;
      j.q = qi; j.ylo = rg.lo; j.nw = (int32_t)n; j.col_offset = 0; j.full_n = n; j.own_lo = 1;
      j.quirk = (p.semantics == MI355_SW_U8SAT && q.len[qi] == n) ? 1 : 0;
      j.target = -1.0f; j.want_dirs = want_trace;
      jobs.push_back(j); owner.push_back(pos);
      bytes += need;
      ++pos;
    }
    int rc = run_exact(ctx, ref, q, p, jobs, 0, jobs.size(), nullptr);
    if (rc) return rc;
    std::vector<std::pair<int32_t, int32_t>> starts;
    std::vector<int32_t> exlo(jobs.size(), 0);
    for (size_t t = 0; t < jobs.size(); ++t) {
      Located &L = loc[owner[t]];
      L.score = jobs[t].best > 0 ? jobs[t].best : 0;
      L.ix = jobs[t].ci; L.iy = jobs[t].cj;
      starts.emplace_back(L.score > 0 ? (int32_t)L.ix : 0, L.score > 0 ? (int32_t)L.iy : 0);
    }
    if (want_trace) {
      std::vector<TraceOut> outs;
      std::vector<int> st;
      rc = run_walk(ctx, ref, q, jobs, 0, jobs.size(), starts, exlo, outs, st);
      if (rc) return rc;
      for (size_t t = 0; t < jobs.size(); ++t) {
        if (st[t] != 0) return fail(ctx, MI355_SW_ENOTSUP, "traceback walk failed on a whole-matrix window");
        tout[owner[t]] = std::move(outs[t]);
      }
    }
  }
  return 0;
}

// Whole-matrix path for the listed queries over one range (problems the score kernel does not take).
// Small problems with identity scoring run on the register-wavefront kernel (sw_wave_kernel.h): argmax tracking
// for the float engine, traceback decisions for both engines; everything else on the LDS anti-diagonal kernel.
int exact_full(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
               const mi355_sw_params &p, const std::vector<int> &qidx, bool want_trace,
               std::vector<Located> &loc, std::vector<TraceOut> &tout) {
  HostTrace trace_("exact_full");
  const int64_t n = rg.hi - rg.lo;
  loc.assign(qidx.size(), Located());
  tout.assign(qidx.size(), TraceOut());
  const bool wave_ok = wave_scoring_ok(p) && !opt().no_wave;
  const bool u8 = p.semantics == MI355_SW_U8SAT;
  // orientation per query: -1 = LDS kernel for everything
  std::vector<int> orient(qidx.size(), -1);
  for (size_t k = 0; k < qidx.size(); ++k) {
    const int m = q.len[qidx[k]];
    if (!wave_ok || m < 1 || n < 1) continue;
    if (u8 && m == n) continue;                                   // |x| == |y| quirk lives in the LDS kernel
    if (m <= kWaveMaxLanesSide && m <= n) orient[k] = 0;
    else if (n <= kWaveMaxLanesSide) orient[k] = 1;
  }
  // 1. score + argmax
  std::vector<int> lds_all, lds_score_only;                       // positions k
  for (size_t k = 0; k < qidx.size(); ++k) {
    if (orient[k] < 0) lds_all.push_back((int)k);
    else if (u8) lds_score_only.push_back((int)k);                // uint8 storage order: LDS kernel's order_key
  }
  auto run_lds = [&](const std::vector<int> &ks, bool trace) -> int {
    if (ks.empty()) return 0;
    std::vector<int> sub(ks.size());
    for (size_t t = 0; t < ks.size(); ++t) sub[t] = qidx[ks[t]];
    std::vector<Located> l2;
    std::vector<TraceOut> t2;
    int rc = exact_full_lds(ctx, ref, q, rg, p, sub, trace, l2, t2);
    if (rc) return rc;
    for (size_t t = 0; t < ks.size(); ++t) { loc[ks[t]] = l2[t]; tout[ks[t]] = std::move(t2[t]); }
    return 0;
  };
  int rc = run_lds(lds_all, want_trace);
  if (rc) return rc;
  rc = run_lds(lds_score_only, false);
  if (rc) return rc;
  if (!u8) {
    for (int o = 0; o < 2; ++o) {
      std::vector<WaveJob> jobs;
      std::vector<size_t> owner;
      jobs.reserve(qidx.size()); owner.reserve(qidx.size());
      for (size_t k = 0; k < qidx.size(); ++k) {
        if (orient[k] != o) continue;
        WaveJob j;
        j.q = qidx[k]; j.orient = o; j.s_lo = 0; j.nb = o == 0 ? (int32_t)n : q.len[qidx[k]]; j.track = true; j.dirs = false;
        jobs.push_back(j); owner.push_back(k);
      }
      rc = run_wave(ctx, ref, q, rg, p, jobs);
      if (rc) return rc;
      parallel_for(jobs.size(), [&](size_t t0, size_t t1) {
        for (size_t t = t0; t < t1; ++t) {
          Located &L = loc[owner[t]];
          L.score = jobs[t].best > 0 ? jobs[t].best : 0;
          L.ix = jobs[t].ci; L.iy = jobs[t].cj;
        }
      });
    }
  }
  // 2. traceback of the wave-eligible ones
  if (want_trace) {
    for (int o = 0; o < 2; ++o) {
      std::vector<int> sub;
      std::vector<Located> sl;
      std::vector<size_t> owner;
      sub.reserve(qidx.size()); sl.reserve(qidx.size()); owner.reserve(qidx.size());
      for (size_t k = 0; k < qidx.size(); ++k)
        if (orient[k] == o) { sub.push_back(qidx[k]); sl.push_back(loc[k]); owner.push_back(k); }
      if (sub.empty()) continue;
      std::vector<TraceOut> t2;
      rc = wave_trace(ctx, ref, q, rg, p, o, sub, sl, t2);
      if (rc) return rc;
      for (size_t t = 0; t < sub.size(); ++t) tout[owner[t]] = std::move(t2[t]);
    }
  }
  return 0;
}

// Argmax cells for the score-kernel queries (qfast[q] != 0) over one range, from the score pass' keys.
// qchunk / qwarm: tile geometry of each query's bucket.
int locate_fast(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
                const mi355_sw_params &p, const std::vector<char> &qfast_in, const std::vector<int64_t> &qchunk,
                const std::vector<int64_t> &qwarm, const std::vector<char> &qfloat, const unsigned long long *keys,
                const ScoreTable &table, std::vector<Located> &loc, const std::vector<char> *skip = nullptr) {
  HostTrace trace_("locate_fast");
  const size_t nq = q.nq;
  std::vector<char> qfast = qfast_in;                    // (queries already located elsewhere are not ours)
  if (skip) for (size_t k = 0; k < nq; ++k) if ((*skip)[k]) qfast[k] = 0;
  const int64_t n = rg.hi - rg.lo;
  std::vector<ExactJob> jobs;
  std::vector<WaveJob> sjobs;                  // long queries with identity scoring: pipelined strip kernel
  std::vector<WaveJob> wjobs;                  // short queries, float engine, identity scoring: register wavefront
  const bool strip_ok = strip_scoring_ok(ref, p);
  // float order = (column, row): no cell left of the sub-chunk can equal the maximum (it would have been reported
  // by an earlier sub-chunk), so the wave kernel's plain first-maximum tracking over the whole window is the answer
  // the uint8 order needs the storage-order key of every cell that equals the maximum: keyed tracking
  const bool wave_locate = wave_scoring_ok(p) && !opt().no_wave;
  const bool wave_keyed = p.semantics == MI355_SW_U8SAT;
  auto qscore = [&](size_t k) { return key_score(qfloat[k], (uint32_t)(keys[k] >> 32), ctx->fshift); };
  // long queries are few and each re-run occupies one workgroup: cut their sub-chunk into pieces (each with its
  // own margin) so that the idle CUs share the work
  size_t nlong = 0;                       // workgroups the long queries' sub-chunks need before cutting
  for (size_t k = 0; k < nq; ++k)
    if (qfast[k] && q.len[k] > 512 && qscore(k) > 0) nlong += p.semantics == MI355_SW_U8SAT ? 5 : 1;
  for (size_t k = 0; k < nq; ++k) {
    if (!qfast[k]) continue;
    const unsigned long long key = keys[k];
    const float score = qscore(k);
    if (!(score > 0)) continue;
    const int64_t chunk_len = qchunk[k];           // sub-chunk granularity of this query's bucket
    const int64_t nchunks = (n + chunk_len - 1) / chunk_len;
    // only cells equal to the known maximum compete: a path that reaches `score` within |x| diagonal steps can
    // afford fewer gap columns than the general margin allows (lemma L3)
    int64_t warm = qwarm[k];
    const Margin mg = table.margin(q.len[k]);
    if (mg.finite()) {
      const double spare = std::max(0.0, mg.smax * (double)q.len[k] - (double)score);
      warm = std::min<int64_t>(warm, clamp_cols((double)q.len[k] + std::ceil(spare / mg.g) + 2.0));
    }
    const int64_t first = (int64_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
    loc[k].score = score;
    int64_t cand[5];
    int nc = 0;
    cand[nc++] = first;
    if (p.semantics == MI355_SW_U8SAT) {
      // storage order = anti-diagonal (mod ncols): the first maximum lies in the first tile that
      // reached the maximum or the next one, or in the corner triangles (first / last two tiles)
      const int64_t extra[4] = {first + 1, 0, nchunks - 2, nchunks - 1};
      for (int64_t c : extra) {
        if (c < 0 || c >= nchunks) continue;
        bool dup = false;
        for (int t = 0; t < nc; ++t) dup |= cand[t] == c;
        if (!dup) cand[nc++] = c;
      }
    }
    for (int t = 0; t < nc; ++t) {
      // lanes lag by up to 63 columns (whole-wavefront tiles): the end of the previous sub-chunk is reported with this one
      const int64_t sub_lo = std::max<int64_t>(0, cand[t] * chunk_len - 63);   // range-relative, 0-based
      const int64_t sub_hi = std::min((cand[t] + 1) * chunk_len, n);
      int64_t pieces = 1;
      if (q.len[k] > 512) pieces = std::max<int64_t>(1, std::min<int64_t>((sub_hi - sub_lo) / 256, (int64_t)(dev_cus() * 7 / 8) / (int64_t)nlong));   // one 1024-thread workgroup per CU
      const int64_t plen = (sub_hi - sub_lo + pieces - 1) / pieces;
      for (int64_t own_lo = sub_lo; own_lo < sub_hi; own_lo += plen) {
        const int64_t own_hi = std::min(own_lo + plen, sub_hi);
        const int64_t wl = std::max<int64_t>(0, own_lo - warm);
        if (wave_locate && q.len[k] <= kWaveMaxLanesSide) {
          WaveJob wj;
          wj.q = (int)k; wj.orient = 0; wj.s_lo = wl; wj.nb = (int32_t)(own_hi - wl); wj.track = true; wj.dirs = false;
          wj.target = score; wj.keyed = wave_keyed;
          // float order: nothing left of the sub-chunk can equal the maximum, so the whole window may compete
          wj.own_lo = wave_keyed ? (int32_t)(own_lo - wl) : 0;
          wjobs.push_back(wj);
          continue;
        }
        if (strip_ok && q.len[k] > kWaveMaxLanesSide) {
          WaveJob sj;
          sj.q = (int)k; sj.orient = 0; sj.s_lo = wl; sj.nb = (int32_t)(own_hi - wl); sj.track = true; sj.dirs = false;
          sj.target = score; sj.own_lo = (int32_t)(own_lo - wl);
          sjobs.push_back(sj);
          continue;
        }
        ExactJob j;
        j.q = (int)k; j.ylo = rg.lo + wl; j.nw = (int32_t)(own_hi - wl); j.col_offset = wl; j.full_n = n;
        j.own_lo = (int32_t)(own_lo - wl + 1); j.quirk = 0; j.target = score; j.want_dirs = false;
        jobs.push_back(j);
      }
    }
  }
  for (size_t lo = 0; lo < jobs.size(); lo += 65536) {
    int rc = run_exact(ctx, ref, q, p, jobs, lo, std::min(jobs.size(), lo + 65536), nullptr);
    if (rc) return rc;
  }
  std::vector<unsigned long long> bestkey(nq, ~0ull);
  for (const ExactJob &j : jobs) {
    if (j.best != j.target) continue;
    const unsigned long long kk = host_order_key(p.semantics, j.ci, j.cj, q.len[j.q], n);
    if (kk < bestkey[j.q]) { bestkey[j.q] = kk; loc[j.q].ix = j.ci; loc[j.q].iy = j.cj; }
  }
  if (!wjobs.empty() && wjobs.size() <= kLatencyJobs && strip_ok) {
    // latency mode: a handful of short problems — a whole wavefront each, few rows per lane
    sjobs.insert(sjobs.end(), wjobs.begin(), wjobs.end());
    wjobs.clear();
  }
  for (size_t lo = 0; lo < wjobs.size(); lo += 262144) {
    std::vector<WaveJob> part(wjobs.begin() + lo, wjobs.begin() + std::min(wjobs.size(), lo + 262144));
    int rc = run_wave(ctx, ref, q, rg, p, part);
    if (rc) return rc;
    for (const WaveJob &j : part) {
      if (j.best != j.target) continue;
      const unsigned long long kk = host_order_key(p.semantics, j.ci, j.cj, q.len[j.q], n);
      if (kk < bestkey[j.q]) { bestkey[j.q] = kk; loc[j.q].ix = j.ci; loc[j.q].iy = j.cj; }
    }
  }
  if (!sjobs.empty()) {
    // one launch per kernel instance (rows per lane)
    for (int R : {3, 5, 8, 10, 16}) {
      std::vector<WaveJob> group;
      for (const WaveJob &j : sjobs) if (strip_R_few(q.len[j.q], sjobs.size(), true) == R) group.push_back(j);
      for (size_t lo = 0; lo < group.size(); lo += 4096) {
        std::vector<WaveJob> part(group.begin() + lo, group.begin() + std::min(group.size(), lo + 4096));
        int rc = run_strip(ctx, ref, q, rg, p, part, R);
        if (rc) return rc;
        for (const WaveJob &j : part) {
          if (j.ci <= 0) continue;
          const unsigned long long kk = host_order_key(p.semantics, j.ci, j.cj, q.len[j.q], n);
          if (kk < bestkey[j.q]) { bestkey[j.q] = kk; loc[j.q].ix = j.ci; loc[j.q].iy = j.cj; }
        }
      }
    }
  }
  for (size_t k = 0; k < nq; ++k)
    if (qfast[k] && loc[k].score > 0 && bestkey[k] == ~0ull)
      return fail(ctx, MI355_SW_ENODEV, "internal: maximum of the score pass not found again by the exact kernel");
  return 0;
}

// (L5 — candidates of a sampled sweep —, L6 — flagged sub-chunks of a saturating sweep —, L3 for the margin.)
// Queries whose saturating float16 sweep reached the cap (host_score.h make_buckets): exact maximum and first maximum
// cell from the sub-chunks the sweep flagged — each re-evaluated on the pipelined strip kernel (kStripMax) over a window
// with the general warm-up margin in front.  `flagged` = {query id, sub-chunk}; done[k] is set for every query resolved.
int locate_saturated(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const mi355_sw_params &p,
                     const std::vector<int64_t> &qchunk, const std::vector<int64_t> &qwarm, const std::vector<float> &qlower,
                     const ScoreTable &table,
                     const std::vector<std::pair<uint32_t, uint32_t>> &flagged, std::vector<Located> &loc, std::vector<char> &done) {
  HostTrace trace_("locate_saturated");
  const int64_t n = rg.hi - rg.lo;
  std::vector<WaveJob> jobs;
  jobs.reserve(flagged.size());
  // long queries are few and each window occupies one workgroup: cut their sub-chunks into pieces (each with its own
  // margin) so that the idle CUs share the work, as locate_fast does
  size_t nlong = 0;
  for (const auto &f : flagged) nlong += q.len[f.first] > 512 ? 1 : 0;
  for (const auto &f : flagged) {
    const int k = (int)f.first;
    const int64_t sub_len = qchunk[k];
    const int64_t sub_lo = std::max<int64_t>(0, (int64_t)f.second * sub_len - 63);   // the lane lag of the sweep
    const int64_t sub_hi = std::min(((int64_t)f.second + 1) * sub_len, n);
    if (sub_lo >= sub_hi) continue;
    // only cells that hold the maximum M >= qlower[k] (the sweep's key: a lower bound) must come out exact: a path that
    // reaches M within |x| diagonal steps can afford fewer gap columns than the general margin allows (as locate_fast)
    int64_t warm = qwarm[k];
    const Margin mg = table.margin(q.len[k]);
    if (mg.finite() && qlower[k] > 0) {
      const double spare = std::max(0.0, mg.smax * (double)q.len[k] - (double)qlower[k]);
      warm = std::min<int64_t>(warm, clamp_cols((double)q.len[k] + std::ceil(spare / mg.g) + 2.0));
    }
    int64_t pieces = 1;
    if (q.len[k] > 512) pieces = std::max<int64_t>(1, std::min<int64_t>((sub_hi - sub_lo) / 256, (int64_t)(dev_cus() * 7 / 8) / (int64_t)std::max<size_t>(1, nlong)));
    if (warm >= sub_hi) pieces = 1;                               // (every piece would start at column 0: no point in cutting)
    const int64_t plen = (sub_hi - sub_lo + pieces - 1) / pieces;
    for (int64_t own_lo = sub_lo; own_lo < sub_hi; own_lo += plen) {
      const int64_t own_hi = std::min(own_lo + plen, sub_hi);
      const int64_t wl = std::max<int64_t>(0, own_lo - warm);
      WaveJob j;
      j.q = k; j.orient = 0; j.s_lo = wl; j.nb = (int32_t)(own_hi - wl); j.track = true; j.dirs = false; j.maxmode = true;
      j.target = -1.0f; j.own_lo = (int32_t)(own_lo - wl);
      jobs.push_back(j);
    }
  }
  std::vector<unsigned long long> bestkey(q.nq, ~0ull);
  for (int R : {3, 5, 8, 10, 16}) {
    std::vector<WaveJob> group;
    for (const WaveJob &j : jobs) if (strip_R_few(q.len[j.q], jobs.size(), true) == R) group.push_back(j);
    for (size_t lo = 0; lo < group.size(); lo += 4096) {
      std::vector<WaveJob> part(group.begin() + lo, group.begin() + std::min(group.size(), lo + 4096));
      int rc = run_strip(ctx, ref, q, rg, p, part, R);
      if (rc) return rc;
      for (const WaveJob &j : part) {
        if (!(j.best > 0) || j.ci <= 0) continue;
        const unsigned long long kk = host_order_key(p.semantics, j.ci, j.cj, q.len[j.q], n);
        Located &L = loc[j.q];
        if (j.best > L.score || (j.best == L.score && kk < bestkey[j.q])) { L.score = j.best; L.ix = j.ci; L.iy = j.cj; bestkey[j.q] = kk; }
        done[j.q] = 1;
      }
    }
  }
  return 0;
}

// locate_saturated, with the candidates of a lone long query taken from the state its sweep saved where that state covers
// them (host_saved.h): blocks with known left column and top row instead of windows behind a zero border and a margin.
int locate_flagged(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const mi355_sw_params &p,
                   const std::vector<int64_t> &qchunk, const std::vector<int64_t> &qwarm, const std::vector<float> &qlower,
                   const ScoreTable &table, const std::vector<std::pair<uint32_t, uint32_t>> &flagged, std::vector<Located> &loc,
                   std::vector<char> &done) {
  const int qid = q.nq == 1 ? q.order[0] : -1;
  const int sr = qid >= 0 ? saved_range_index(ctx, ref, q, rg, p, qid) : -1;
  if (sr < 0 || flagged.empty() || qchunk[qid] != ctx->lsaved.sub_len)
    return locate_saturated(ctx, ref, q, rg, p, qchunk, qwarm, qlower, table, flagged, loc, done);
  std::vector<uint32_t> subs, rest;
  for (const auto &f : flagged) if ((int)f.first == qid) subs.push_back(f.second);
  Located L;
  bool found = false;
  int rc = locate_from_saved(ctx, ref, q, rg, p, sr, qid, qlower[qid], table, subs, L, found, rest);
  if (rc) return rc;
  if (!rest.empty()) {
    ctx->saved_fallbacks += rest.size();
    std::vector<std::pair<uint32_t, uint32_t>> fr;
    for (uint32_t sgl : rest) fr.push_back({(uint32_t)qid, sgl});
    std::vector<Located> l2(q.nq);
    std::vector<char> d2(q.nq, 0);
    rc = locate_saturated(ctx, ref, q, rg, p, qchunk, qwarm, qlower, table, fr, l2, d2);
    if (rc) return rc;
    if (d2[qid]) {
      const int64_t m = q.len[qid], n = rg.hi - rg.lo;
      const bool better = !found || l2[qid].score > L.score ||
                          (l2[qid].score == L.score && host_order_key(p.semantics, l2[qid].ix, l2[qid].iy, m, n) < host_order_key(p.semantics, L.ix, L.iy, m, n));
      if (better) { L = l2[qid]; found = true; }
    }
  }
  if (found) { loc[qid] = L; done[qid] = 1; }
  return 0;
}

float elapsed_us(mi355_sw_ctx *ctx, hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0;
  (void)ctx;
  return ms * 1000.0f;
}

// The thin stage of a row-P pass at P rows (DESIGN.md §3.3 lemma L20; host_score.h kThinP2): its taller height P2, the columns W12 a
// crossing of row P2 may lie right of a flagged column of row P, the warm-up in front of an item's own columns (the margin of L1
// for P2 rows, as Bucket::warm without its rounding to whole segments), the sub-chunks D2 a survivor's end cell may lie right of it, and the values per item.  P2 = 0: no thin
// stage — option no_prefix_thin, a pass at P2 rows or more, reads of P2 rows or fewer, sub-chunks shorter than the 63 columns of lag
// (an item's own columns would start below its left neighbour), or a score table beyond the kernel's LDS.
struct ThinPlan {
  int P2 = 0, nout = 0;
  int64_t W12 = 0, warm2 = 0, D2 = 0;
};
constexpr size_t kThinTableMax = 32 * 1024;
ThinPlan thin_plan(const RefData &ref, const ScoreTable &t, int P, int minlen, int maxlen, int64_t E) {
  ThinPlan tp;
  if (opt().no_prefix_thin || !t.integral || t.gap <= 0 || t.smax <= 0 || t.ftab.empty()) return tp;
  if (P >= kThinP2 || minlen <= kThinP2 || E < 64 || E > (1 << 20) || (size_t)256 * ref.ncodes * 4 > kThinTableMax) return tp;
  const Margin mg = t.margin(kThinP2);
  if (!mg.finite()) return tp;
  tp.P2 = kThinP2;
  tp.W12 = (int64_t)(tp.P2 - P) + (int64_t)((int64_t)t.smax * (tp.P2 - P) / t.gap);
  tp.warm2 = mg.cols(tp.P2);
  const int64_t W2 = (int64_t)(maxlen - tp.P2) + (int64_t)((int64_t)t.smax * (maxlen - tp.P2) / t.gap);
  tp.D2 = (W2 + E - 1) / E;
  tp.nout = 3 + (int)((tp.W12 - 1) / E);
  return tp;
}

// sw_prefix_thin_kernel over `items` = {query id, sub-chunk}, sorted; thr2 by query id (> 0 for every listed query).  kept: the
// {query id, sub-chunk} whose row-P2 maximum reaches thr2, sorted and without duplicates.  vals (test hook): [items][tp.nout].
int run_thin(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const ScoreTable &table, const ThinPlan &tp, int64_t E,
             const std::vector<std::pair<uint32_t, uint32_t>> &items, const std::vector<float> &thr2,
             std::vector<std::pair<uint32_t, uint32_t>> &kept, std::vector<float> *vals = nullptr) {
  HostTrace trace_("run_thin");
  kept.clear();
  const size_t ni = items.size(), nq = q.nq;
  if (ni == 0) return 0;
  if (tp.P2 != kThinP2) return fail(ctx, MI355_SW_ENODEV, "internal: no sw_prefix_thin_kernel instance of that height");
  // an item as `split` lanes on sub-chunks of E / split columns: the same own columns, a shorter window per lane (host_score.h kThinSplit)
  int split = vals ? 1 : kThinSplit;
  while (split > 1 && (E % split != 0 || E / split < 64)) split /= 2;
  const size_t nl = ni * (size_t)split;
  const int64_t El = E / split;
  const int nout = vals ? tp.nout : 3 + (int)((tp.W12 - 1) / El);
  if (nl * (size_t)nout > 0x7FFFFFFFull) return fail(ctx, MI355_SW_ENOTSUP, "too many items for the thin stage");
  std::vector<uint32_t> raw(2 * nl);
  for (size_t k = 0; k < ni; ++k)
    for (int h = 0; h < split; ++h) { raw[2 * (k * split + h)] = items[k].first; raw[2 * (k * split + h) + 1] = items[k].second * (uint32_t)split + (uint32_t)h; }
  if (ctx->thin_items.ensure(nl * 8 + 16) || ctx->thin_out.ensure(8 + nl * (size_t)nout * 8 + 16) || ctx->pthr.ensure(nq * 4 + 16) ||
      (vals && ctx->thin_vals.ensure(nl * (size_t)nout * 4 + 16)))
    return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
  HIPCHK(ctx, hipMemcpyAsync(ctx->thin_items.p, raw.data(), nl * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->pthr.p, thr2.data(), nq * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->thin_out.p, 0, 8, ctx->stream));
  ThinArgs a;
  a.items = ctx->thin_items.as<uint2>(); a.nitems = (uint32_t)nl;
  a.thr2 = ctx->pthr.as<float>();
  a.codes = ref.codes.as<uint8_t>() + rg.lo; a.n = rg.hi - rg.lo;
  a.qbytes = q.bytes.as<uint8_t>(); a.qoff = q.offs.as<int64_t>();
  a.ftab = ctx->ftab.as<float>(); a.ncodes = ref.ncodes; a.gap = table.gapf;
  a.E = (int32_t)El; a.warm2 = (int32_t)tp.warm2; a.W12 = (int32_t)tp.W12; a.nout = nout;
  a.count = ctx->thin_out.as<unsigned int>(); a.list = reinterpret_cast<uint2 *>(ctx->thin_out.as<unsigned int>() + 2);
  a.vals = vals ? ctx->thin_vals.as<float>() : nullptr;
  hipLaunchKernelGGL(sw_prefix_thin_kernel<kThinP2>, dim3((unsigned)((nl + 63) / 64)), dim3(64), (size_t)256 * ref.ncodes * 4, ctx->stream, a);
  HIPCHK(ctx, hipGetLastError());
  unsigned int nkept = 0;
  HIPCHK(ctx, hipMemcpyAsync(&nkept, ctx->thin_out.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if ((size_t)nkept > nl * (size_t)nout) return fail(ctx, MI355_SW_ENODEV, "internal: the thin stage kept more than it was given");
  std::vector<uint32_t> out(2 * (size_t)nkept);
  if (nkept) HIPCHK(ctx, hipMemcpy(out.data(), ctx->thin_out.as<unsigned int>() + 2, (size_t)nkept * 8, hipMemcpyDeviceToHost));
  kept.reserve(nkept);
  for (size_t k = 0; k < nkept; ++k) kept.push_back({out[2 * k], out[2 * k + 1] / (uint32_t)split});
  std::sort(kept.begin(), kept.end());
  kept.erase(std::unique(kept.begin(), kept.end()), kept.end());
  if (vals) {
    vals->resize(ni * (size_t)tp.nout);
    HIPCHK(ctx, hipMemcpy(vals->data(), ctx->thin_vals.p, vals->size() * 4, hipMemcpyDeviceToHost));
  }
  ctx->prefix_thin_items += ni;
  return 0;
}

// (DESIGN.md §3.3 lemma L19.)  The prefix filter of one bucket (host_score.h prefix_ok), in front of the full sweep: a sampled sweep of
// the first P = kPrefixLanes * R rows of every read, then all rows only where those rows allow the maximum.
//   round 1: the sub-chunk of the read's prefix key and its right neighbours, evaluated exactly on all rows: B0, an exact alignment score;
//   round 2: sw_prefix_filter flags every sub-chunk whose prefix value reaches B0 - smax (m - P) - slack; each flagged sub-chunk f
//            stands for f .. f + D (D = ceil(W / sub_len): the end cell lies at most W columns right of its crossing of row P; the
//            left neighbour is covered by the 63 columns a candidate window starts in front of its sub-chunk, locate_saturated),
//            and what round 1 has not evaluated is evaluated now; the read's result is the first maximum over both rounds.
//            On the step tiles the flags pass the THIN stage first (thin_plan, run_thin; lemma L20): each is evaluated on the prefix of
//            P2 > P rows over its own columns, a survivor is the sub-chunk that holds a row-P2 cell at B0 - smax (m - P2) or more, and
//            stands for itself and D2 <= D right neighbours.  Thinned: every read over its cap (up to thin_flag_cap flags), and everybody
//            else once the pass has more than kThinMinFlags flags; only reads with B0 > smax max(m - P2, P2), and only ranges of
//            thin_cols_min() columns or more (option no_prefix_thin: none).
// A read is an OFFENDER (appended to `offenders`, nothing written for it) when B0 cannot certify — B0 <= smax (m - P) + slack —
// or when it sends more sub-chunks to the locate stage than its cap.  Everybody else: loc[] and qdone[] are final, qchunk[] / qwarm[] set.
// The prefix is P = kPrefixLanes * prefR rows, which need not be the bucket's own R (a probed bucket tries a lower height first,
// align_range_core).  rowp: the tiles fold row P alone — slack = rowp_slack, and a read also offends unless B0 > smax P (prefix_bound).
// vote (by query id, may be null; a probe at a lower height asks): could a row-P pass of voteR rows per lane certify the read?  1 when
// B0 is above that height's bound AND that height's threshold, B0 - smax (m - 2 voteR) - slack, applied to the values of THIS sweep
// stays within the cap.  The second part is a forecast, not a proof: row 2 voteR reads no lower than the row swept here against a
// random background, so a threshold that drowns here drowns there (10 % substitutions: B0 is about 360, above the bound 342 of
// R = 19, with a threshold of 18 that most sub-chunks reach).  It only steers the choice of the height; every result stays exact.
// ask: what a caller wants beyond the pass itself.  step: the tiles fold row P at EVERY step (rowp only) — rowp_slack is then 0, here and in
// the votes; one vote per height of voteR (votes[k][query id]); B0 (by query id) receives the exact round-1 score of every read of the
// pass, offenders included; gave_up is set when most of the pass offended and everybody was handed back.
struct PrefixAsk {
  bool step = false, second = false;
  bool bulk = false;                           // the tiles of the chained main pass whatever the pass's size (score_launch: chain_main)
  std::vector<int> voteR;
  std::vector<std::vector<char>> *votes = nullptr;
  std::vector<float> *B0 = nullptr;
  bool *gave_up = nullptr;
  // The seeded flow (prefix_seeded) knows B0 of most reads BEFORE the pass.  given[id] != 0: round 1 is not run for the read — its B0 is
  // (*B0)[id] on entry, an exact alignment score; what was evaluated for it are its entries of `f1` ({query id, sub-chunk} in sub-chunks
  // of f1_E columns, sorted), and their first maximum is (*loc1)[id].  B0 <= B is all L19 and L20 use, so the thresholds come from the
  // given B0 and the read's result is the first maximum over those windows and round 2.
  const std::vector<char> *given = nullptr;
  const std::vector<std::pair<uint32_t, uint32_t>> *f1 = nullptr;
  int64_t f1_E = 0;
  const std::vector<Located> *loc1 = nullptr;
};
int prefix_bucket(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const mi355_sw_params &p,
                  const ScoreTable &table, const Bucket &b, int prefR, bool rowp, std::vector<int64_t> &qchunk, std::vector<int64_t> &qwarm,
                  std::vector<Located> &loc, std::vector<char> &qdone, std::vector<int> &offenders, const PrefixAsk &ask = PrefixAsk()) {
  HostTrace trace_("prefix_bucket");
  const size_t nq = q.nq;
  const int64_t n = rg.hi - rg.lo;
  const std::vector<Range> ranges{rg};
  int rc = score_begin(ctx, q, ranges, table);
  if (rc) return rc;
  if (ctx->pkeys.ensure(nq * 8 + 16) || ctx->pthr.ensure(nq * 4 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
  HIPCHK(ctx, hipMemsetAsync(ctx->pkeys.p, 0, nq * 8, ctx->stream));
  // a. the prefix sweep: the instance of prefR rows at kPrefixLanes lanes; keys and sub-chunk values as the sampled sweep writes them
  Bucket pb = b;
  pb.SL = kPrefixLanes; pb.R = prefR; pb.prefix = true; pb.rowp = rowp; pb.step = rowp && ask.step; pb.second = ask.second; pb.bulk = ask.bulk;
  ScoreIO io;
  io.range_lo = ctx->ranges.as<int64_t>(); io.range_hi = ctx->ranges.as<int64_t>() + 1; io.keys = ctx->pkeys.as<unsigned long long>();
  rc = score_launch(ctx, ref, q, ranges, p, table, pb, &io);
  if (rc) return rc;
  std::vector<unsigned long long> pkeys;
  rc = score_fetch(ctx, nq, pkeys, ctx->pkeys.p);
  if (rc) return rc;
  const int P = pb.SL * pb.R;
  const int64_t E = pb.sub_len, nsub = (n + E - 1) / E;                            // sub-chunks that hold columns of the range
  const int64_t stride = ((n + pb.chunk_len - 1) / pb.chunk_len) * (pb.chunk_len / E);   // value row of one read (whole tiles)
  const float vslack = rowp_slack(table, rowp_mk(ask.step));                       // of a row-P pass on the same kind of tile
  const float slack = rowp ? vslack : sample_slack(table, pb), smax = (float)table.smax;
  const int64_t W = (int64_t)(b.maxlen - P) + (int64_t)((int64_t)table.smax * (b.maxlen - P) / table.gap);
  const int64_t D = (W + E - 1) / E;
  static_assert(kPrefixLanes - 1 + kScoreMK - 1 <= 63, "a candidate window starts 63 columns in front of its sub-chunk: the lag of a prefix value");
  // b. round 1
  std::vector<float> bound(nq, 0.0f), qlow(nq, 0.0f), B0(nq, 0.0f), thr(nq, 0.0f);
  std::vector<char> off(nq, 0), mine(nq, 0);
  std::vector<std::pair<uint32_t, uint32_t>> f1, f1given;
  auto is_given = [&](int id) { return ask.given && ask.B0 && ask.loc1 && ask.f1 && (*ask.given)[id] != 0; };
  for (int k = 0; k < b.count; ++k) {
    const int id = q.order[b.first + k];
    mine[id] = 1; qchunk[id] = E; qwarm[id] = b.warm;
    // windows of both rounds only have to be exact for cells that hold a maximum above the certification bound (L3)
    bound[id] = prefix_bound(table, q.len[id], P, slack, rowp);
    qlow[id] = bound[id];
    if (is_given(id)) {                                                          // (what the seed stage evaluated, where the sub-chunks are the same)
      if (ask.f1_E == E) {
        auto at = std::lower_bound(ask.f1->begin(), ask.f1->end(), std::make_pair((uint32_t)id, 0u));
        for (; at != ask.f1->end() && at->first == (uint32_t)id; ++at) f1given.push_back(*at);
      }
      continue;
    }
    if (!(key_score(kKeyF16, (uint32_t)(pkeys[id] >> 32), 0) > 0)) { off[id] = 1; continue; }
    const int64_t s0 = (int64_t)(0xFFFFFFFFull - (pkeys[id] & 0xFFFFFFFFull));
    for (int64_t sc = s0; sc <= s0 + D && sc < nsub; ++sc) f1.push_back({(uint32_t)id, (uint32_t)sc});
  }
  std::sort(f1.begin(), f1.end());
  std::vector<Located> loc1(nq), loc2(nq);
  std::vector<char> done1(nq, 0), done2(nq, 0);
  HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
  rc = locate_flagged(ctx, ref, q, rg, p, qchunk, qwarm, qlow, table, f1, loc1, done1);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
  ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  const size_t nlocated1 = f1.size();
  if (!f1given.empty()) {                                                        // from here on f1 is everything evaluated before round 2
    f1.insert(f1.end(), f1given.begin(), f1given.end());
    std::sort(f1.begin(), f1.end());
  }
  size_t noff = 0;
  for (int k = 0; k < b.count; ++k) {
    const int id = q.order[b.first + k];
    if (is_given(id)) { loc1[id] = (*ask.loc1)[id]; done1[id] = (*ask.B0)[id] > 0.0f ? 1 : 0; }
    B0[id] = done1[id] ? loc1[id].score : 0.0f;
    if (!off[id] && !(B0[id] > bound[id])) off[id] = 1;
    if (!off[id]) thr[id] = B0[id] - smax * (float)(q.len[id] - P) - slack;      // (> 0: B0 is above the bound)
    noff += off[id] ? 1 : 0;
    if (ask.B0) (*ask.B0)[id] = B0[id];
  }
  auto give_up = [&]() {                                                         // most of the bucket offends: the full sweep for all of it
    for (int k = 0; k < b.count; ++k) offenders.push_back(q.order[b.first + k]);
    if (ask.gave_up) *ask.gave_up = true;
    return 0;
  };
  // one filter launch over the bucket's value rows with per-query thresholds: flags in ctx->flags, their number and the per-query counts
  const uint32_t qcap = query_flag_cap(nq);
  unsigned int nflag = 0;
  std::vector<uint32_t> cnt(nq, 0);
  auto run_filter = [&](const std::vector<float> &t, uint32_t cap) -> int {
    HIPCHK(ctx, hipMemcpyAsync(ctx->pthr.p, t.data(), nq * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->flags.p, 0, 8, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->qcnt.p, 0, nq * 4, ctx->stream));
    for (int f0 = 0; f0 < b.count; f0 += 65535) {
      const int fc = std::min(65535, b.count - f0);
      const dim3 fgrid((unsigned)std::min<int64_t>(64, (stride + 255) / 256), (unsigned)fc);
      hipLaunchKernelGGL(sw_prefix_filter, fgrid, dim3(256), 0, ctx->stream, (const uint16_t *)ctx->submax.as<uint16_t>(), stride, stride,
                         (const int32_t *)q.sel.as<int32_t>(), b.first, f0, b.count, (const float *)ctx->pthr.as<float>(),
                         ctx->flags.as<unsigned int>(), reinterpret_cast<uint2 *>(ctx->flags.as<unsigned int>() + 2), ctx->flag_cap,
                         ctx->qcnt.as<unsigned int>(), cap);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(&nflag, ctx->flags.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cnt.data(), ctx->qcnt.p, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    nflag = std::min(nflag, ctx->flag_cap);
    return 0;
  };
  if (ask.votes) ask.votes->assign(ask.voteR.size(), std::vector<char>(nq, 0));
  for (size_t v = 0; ask.votes && v < ask.voteR.size(); ++v) {
    const int vP = kPrefixLanes * ask.voteR[v];
    std::vector<float> vthr(nq, 0.0f);
    for (int k = 0; k < b.count; ++k) {
      const int id = q.order[b.first + k];
      if (B0[id] > prefix_bound(table, q.len[id], vP, vslack, true)) vthr[id] = B0[id] - smax * (float)(q.len[id] - vP) - vslack;
    }
    rc = run_filter(vthr, qcap);
    if (rc) return rc;
    for (int k = 0; k < b.count; ++k) {
      const int id = q.order[b.first + k];
      (*ask.votes)[v][id] = vthr[id] > 0.0f && cnt[id] <= qcap;
    }
  }
  if (2 * noff > (size_t)b.count) return give_up();
  // c. round 2: the filter with the thresholds of this height, under query_flag_cap as ever: the per-read counts it returns are exact
  // whatever the cap, the list holds at most cap + 1 entries per read.
  int minlen = b.maxlen;
  for (int k = 0; k < b.count; ++k) minlen = std::min<int>(minlen, q.len[q.order[b.first + k]]);
  ThinPlan tp;
  if (rowp && ask.step && n >= thin_cols_min()) tp = thin_plan(ref, table, P, minlen, b.maxlen, E);
  rc = run_filter(thr, qcap);
  if (rc) return rc;
  std::vector<uint32_t> raw(2 * (size_t)nflag);
  if (nflag) HIPCHK(ctx, hipMemcpy(raw.data(), ctx->flags.as<unsigned int>() + 2, (size_t)nflag * 8, hipMemcpyDeviceToHost));
  // d. offenders by the cap.  A read over query_flag_cap is thinned instead, if row P2 can certify it — B0 > smax (m - P2) and B0 >
  // smax P2 (L20) — and while there is room: at most thin_flag_cap flags per read and kThinItemsMax for all such reads of the pass,
  // the reads with the fewest flags first (host_score.h).  Their flags are listed by a second filter launch with thresholds for them alone.
  std::vector<char> thin(nq, 0);
  std::vector<float> thr2(nq, 0.0f);
  auto thin_ok = [&](int id) { return tp.P2 && B0[id] > prefix_bound(table, q.len[id], tp.P2, 0.0f, true); };
  std::vector<std::pair<uint32_t, int>> over;                                      // {flags, read}: over the cap, and the stage may take it
  for (int k = 0; k < b.count; ++k) {
    const int id = q.order[b.first + k];
    if (off[id] || cnt[id] <= qcap) continue;
    if (cnt[id] <= thin_flag_cap(qcap) && thin_ok(id)) over.push_back({cnt[id], id});
    else { off[id] = 1; ++noff; }
  }
  std::sort(over.begin(), over.end());
  size_t room = kThinItemsMax;
  std::vector<float> thr_thin(nq, 0.0f);
  for (const auto &o : over) {
    if (o.first <= room) { room -= o.first; thin[o.second] = 1; thr_thin[o.second] = thr[o.second]; }
    else { off[o.second] = 1; ++noff; }
  }
  if (room < kThinItemsMax) {
    const std::vector<uint32_t> cnt_all(cnt);
    rc = run_filter(thr_thin, thin_flag_cap(qcap));
    if (rc) return rc;
    if (nflag >= ctx->flag_cap) {
      // the list may be cut short (kThinItemsMax + a read each is far below kFlagCap: not expected): nothing is read from it, and
      // these reads offend by the cap, as in the flow without the stage
      for (const auto &o : over)
        if (thin[o.second]) { thin[o.second] = 0; off[o.second] = 1; ++noff; }
    } else {
      const size_t was = raw.size();
      raw.resize(was + 2 * (size_t)nflag);
      if (nflag) HIPCHK(ctx, hipMemcpy(raw.data() + was, ctx->flags.as<unsigned int>() + 2, (size_t)nflag * 8, hipMemcpyDeviceToHost));
    }
    nflag = (unsigned int)(raw.size() / 2);
    cnt = cnt_all;
  }
  if (opt().trace) std::fprintf(stderr, "[mi355_sw] prefix filter: %u flagged sub-chunks, %zu of %d reads offend (D = %lld)\n", nflag, noff, b.count, (long long)D);
  if (2 * noff > (size_t)b.count) return give_up();
  // e. what the flags add to round 1
  std::vector<std::pair<uint32_t, uint32_t>> flagged, f2, f2new;
  for (size_t f = 0; f < nflag; ++f) {
    const uint32_t id = raw[2 * f];
    if (id >= nq || !mine[id] || off[id] || raw[2 * f + 1] >= (uint64_t)nsub) continue;
    flagged.push_back({id, raw[2 * f + 1]});
  }
  std::sort(flagged.begin(), flagged.end());
  flagged.erase(std::unique(flagged.begin(), flagged.end()), flagged.end());
  // Reads within query_flag_cap are thinned as well once the pass has more than kThinMinFlags flags beyond round 1's own sub-chunks for
  // the thin stage: below that its launch and synchronisation cost more than the locate candidates it saves (CHANGELOG.md).
  if (tp.P2) {
    size_t fresh = 0;
    for (const auto &f : flagged) fresh += (thin[f.first] || thin_ok((int)f.first)) && !std::binary_search(f1.begin(), f1.end(), f) ? 1 : 0;
    const bool everybody = fresh > kThinMinFlags;
    std::vector<std::pair<uint32_t, uint32_t>> items, kept;
    for (const auto &f : flagged)
      if (thin[f.first] || (everybody && thin_ok((int)f.first))) { thin[f.first] = 1; items.push_back(f); }
    if (!items.empty()) {
      size_t nthin = 0;
      for (int k = 0; k < b.count; ++k) {
        const int id = q.order[b.first + k];
        if (!thin[id]) continue;
        thr2[id] = B0[id] - smax * (float)(q.len[id] - tp.P2);                       // (> 0: thin_ok)
        ++nthin;
      }
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      rc = run_thin(ctx, ref, q, rg, table, tp, E, items, thr2, kept);
      if (rc) return rc;
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
      ctx->prefix_thinned += nthin;
      path_note(ctx, "prefix_thin[P2=%d,items=%zu,kept=%zu]", tp.P2, items.size(), kept.size());
      // whoever keeps more than query_flag_cap sub-chunks offends after all
      std::vector<uint32_t> nkept(nq, 0);
      for (const auto &f : kept) if (f.first < nq) ++nkept[f.first];
      for (int k = 0; k < b.count; ++k) {
        const int id = q.order[b.first + k];
        if (thin[id] && nkept[id] > qcap) { off[id] = 1; ++noff; }
      }
      for (const auto &f : kept) {
        if (f.first >= nq || !thin[f.first] || off[f.first]) continue;
        for (int64_t sc = f.second; sc <= (int64_t)f.second + tp.D2 && sc < nsub; ++sc) f2.push_back({f.first, (uint32_t)sc});
      }
    }
  }
  for (const auto &f : flagged) {
    if (thin[f.first] || off[f.first]) continue;
    for (int64_t sc = f.second; sc <= (int64_t)f.second + D && sc < nsub; ++sc) f2.push_back({f.first, (uint32_t)sc});
  }
  std::sort(f2.begin(), f2.end());
  f2.erase(std::unique(f2.begin(), f2.end()), f2.end());
  std::set_difference(f2.begin(), f2.end(), f1.begin(), f1.end(), std::back_inserter(f2new));
  ctx->candidates += nlocated1 + f2new.size();                                   // (a given read's windows were counted where they were evaluated)
  if (!f2new.empty()) {
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    rc = locate_flagged(ctx, ref, q, rg, p, qchunk, qwarm, B0, table, f2new, loc2, done2);
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  }
  for (int k = 0; k < b.count; ++k) {
    const int id = q.order[b.first + k];
    if (off[id]) { offenders.push_back(id); continue; }
    Located best = loc1[id];                                                     // (done1: B0 > 0 came from it)
    const int64_t m = q.len[id];
    if (done2[id] && (loc2[id].score > best.score ||
                      (loc2[id].score == best.score && host_order_key(p.semantics, loc2[id].ix, loc2[id].iy, m, n) < host_order_key(p.semantics, best.ix, best.iy, m, n))))
      best = loc2[id];
    loc[id] = best; qdone[id] = 1;
    ctx->prefix_certified += 1;
  }
  return 0;
}

// A view of the batch that lists only `ids` (same device bytes / offsets / lengths; its own id list, sorted by length, in `sel`) and
// the bucket that spans it
int prefix_view(mi355_sw_ctx *ctx, const QueryBatch &q, const std::vector<int> &ids, DevBuf &sel, QueryBatch &qv, const Bucket &like, Bucket &vb) {
  qv.bytes.alias(q.bytes.p); qv.lens.alias(q.lens.p); qv.offs.alias(q.offs.p); qv.cum.alias(q.cum.p);
  qv.len = q.len; qv.off = q.off; qv.nq = q.nq; qv.maxlen = q.maxlen;
  qv.order.assign(ids.begin(), ids.end());
  std::stable_sort(qv.order.begin(), qv.order.end(), [&](int32_t a, int32_t b2) { return q.len[a] < q.len[b2]; });
  if (sel.ensure(qv.order.size() * 4 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
  HIPCHK(ctx, hipMemcpy(sel.p, qv.order.data(), qv.order.size() * 4, hipMemcpyHostToDevice));
  qv.sel.alias(sel.p);
  vb = like;
  vb.first = 0; vb.count = (int)qv.order.size();
  return 0;
}

// The prefix filter of a probed bucket of at least kPrefixChain reads: its heights as a chain (host_score.h prefix_heights), every pass
// on tiles that fold row P alone — at every step (no slack) unless option no_prefix_step.
//   probe:  the first kPrefixProbe reads at the LOWEST height h0.  B0 is exact whatever the height; o[0] = the probe's offenders, and
//           o[i] of a taller height = the reads that height's vote does not certify (prefix_bucket: a forecast on the probe's values);
//   start:  the lowest height whose offenders pay less at the next height than everybody pays for starting there (prefix_start_height);
//           none: `failed`, the rest of the bucket skips the filter (prefix_probe_failed);
//   rest:   the rest of the bucket at the start height, with the probe's offenders that this height's vote certifies (riders);
//   second: ONE pass at the next height for the offenders of the rest — only those whose B0 is above that height's bound: a read
//           without a hit does not pay for a pass that cannot certify it — and for the probe's offenders with that height's vote.
// Whoever offends the second pass, and everybody it was not worth trying on, is an offender of the bucket (swept on all rows).
int prefix_chain(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const mi355_sw_params &p,
                 const ScoreTable &table, const Bucket &b, std::vector<int64_t> &qchunk, std::vector<int64_t> &qwarm,
                 std::vector<Located> &loc, std::vector<char> &qdone, std::vector<int> &offenders, bool &failed) {
  const size_t nq = q.nq;
  const bool step = !opt().no_prefix_step;
  const std::vector<int> hs = prefix_heights(table, b, q.len[q.order[b.first]], step);
  const size_t nh = hs.size();
  failed = false;
  Bucket part = b;
  part.count = kPrefixProbe;
  std::vector<std::vector<char>> votes;                              // votes[i - 1]: height i
  std::vector<float> B0(nq, 0.0f);
  std::vector<int> poff;
  PrefixAsk ask;
  ask.step = step; ask.voteR.assign(hs.begin() + 1, hs.end()); ask.votes = &votes; ask.B0 = &B0;
  int rc = prefix_bucket(ctx, ref, q, rg, p, table, part, hs[0], true, qchunk, qwarm, loc, qdone, poff, ask);
  if (rc) return rc;
  std::vector<int> P(nh), o(nh, 0);
  for (size_t i = 0; i < nh; ++i) P[i] = kPrefixLanes * hs[i];
  o[0] = (int)poff.size();
  for (size_t i = 1; i < nh; ++i)
    for (int k = 0; k < part.count; ++k) o[i] += votes[i - 1][q.order[part.first + k]] ? 0 : 1;
  const int start = prefix_start_height(P, o);
  if (start < 0) {
    offenders.insert(offenders.end(), poff.begin(), poff.end());
    path_note(ctx, "prefix_probe_failed");
    failed = true;
    return 0;
  }
  const bool taller = (size_t)start + 1 < nh;                        // there is a height for a second pass
  std::vector<int> riders, pend;
  for (int id : poff) {
    if (start > 0 && votes[start - 1][id]) riders.push_back(id);
    else if (taller && votes[start][id]) pend.push_back(id);
    else offenders.push_back(id);
  }
  if (riders.empty()) path_note(ctx, "prefix_height[R=%d,start]", hs[start]);
  else path_note(ctx, "prefix_height[R=%d,start,riders=%zu]", hs[start], riders.size());
  part.first = b.first + kPrefixProbe; part.count = b.count - kPrefixProbe;
  std::vector<int> roff;
  bool gave_up = false;
  PrefixAsk rask;
  rask.step = step; rask.B0 = &B0; rask.gave_up = &gave_up;
  if (riders.empty()) {
    rc = prefix_bucket(ctx, ref, q, rg, p, table, part, hs[start], true, qchunk, qwarm, loc, qdone, roff, rask);
  } else {
    std::vector<int> ids(riders);
    for (int k = 0; k < part.count; ++k) ids.push_back(q.order[part.first + k]);
    QueryBatch qv;
    Bucket vb;
    rc = prefix_view(ctx, q, ids, ctx->psel2, qv, part, vb);
    if (!rc) rc = prefix_bucket(ctx, ref, qv, rg, p, table, vb, hs[start], true, qchunk, qwarm, loc, qdone, roff, rask);
  }
  if (rc) return rc;
  // (a pass that gave up handed everybody back: most of the bucket has no hit its prefix could show, at any height)
  const float slack = rowp_slack(table, rowp_mk(step));
  for (int id : roff) {
    if (taller && !gave_up && B0[id] > prefix_bound(table, q.len[id], P[start + 1], slack, true)) pend.push_back(id);
    else offenders.push_back(id);
  }
  if (pend.empty()) return 0;
  QueryBatch qv;
  Bucket vb;
  rc = prefix_view(ctx, q, pend, ctx->psel2, qv, part, vb);
  if (rc) return rc;
  path_note(ctx, "prefix_second[R=%d,n=%zu]", hs[start + 1], pend.size());
  ctx->prefix_second_pass += pend.size();
  PrefixAsk sask;
  sask.step = step; sask.second = true;
  return prefix_bucket(ctx, ref, qv, rg, p, table, vb, hs[start + 1], true, qchunk, qwarm, loc, qdone, offenders, sask);
}

// ---- the seeded flow of a chained bucket -------------------------------------------------------------------------
// A host copy of the batch's bytes, fetched once per upload.  (Seeds only steer: B0 is what the locate stage finds on the device's
// own bytes, so a stale copy could cost time, never a result.)
int batch_host_bytes(mi355_sw_ctx *ctx, const QueryBatch &q, const uint8_t *&bytes) {
  size_t tot = 0;
  for (size_t k = 0; k < q.nq; ++k) tot = std::max(tot, (size_t)q.off[k] + (size_t)q.len[k]);
  if (ctx->h_qbytes_of != q.bytes.p || ctx->h_qbytes_version != q.version || ctx->h_qbytes.size() != tot) {
    ctx->h_qbytes.resize(tot);
    if (tot) HIPCHK(ctx, hipMemcpy(ctx->h_qbytes.data(), q.bytes.p, tot, hipMemcpyDeviceToHost));
    ctx->h_qbytes_of = q.bytes.p; ctx->h_qbytes_version = q.version;
  }
  bytes = ctx->h_qbytes.data();
  return 0;
}

// sw_seed_scan_kernel over the range for the seeds of the reads `ids`: count[id] hits (exact), the first kSeedHitCap of them as
// start[id * kSeedHitCap + j] (position - offset, relative to the range) and hoff[...] (the seed's offset in the read).
// usable (may be null): the seeds of every read that entered the table, by read id (u of lemma L21).
int seed_scan(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const std::vector<int32_t> &ids, int k,
              std::vector<uint32_t> &count, std::vector<int64_t> &start, std::vector<int32_t> &hoff, std::vector<uint32_t> *usable = nullptr) {
  HostTrace trace_("seed_scan");
  const size_t nq = q.nq;
  const int64_t n = rg.hi - rg.lo;
  count.assign(nq, 0u); start.assign(nq * kSeedHitCap, 0); hoff.assign(nq * kSeedHitCap, 0);
  if (usable) usable->assign(nq, 0u);
  if (k < 1 || k > kSeedMaxK) return fail(ctx, MI355_SW_EINVAL, "seed length outside 1 .. 32");
  const uint8_t *bytes = nullptr;
  int rc = batch_host_bytes(ctx, q, bytes);
  if (rc) return rc;
  SeedTable t;
  if (!seed_table_build(t, k, bytes, q.off.data(), q.len.data(), ids.data(), ids.size(), ref.code_of))
    return fail(ctx, MI355_SW_ENOTSUP, "too many seeds for the seed table");
  if (usable) seed_usable(t, nq, *usable);
  const size_t ns = t.nseeds();
  if (ns == 0 || n < k) return 0;
  const int64_t threads = (n - k + 1 + kSeedStretch - 1) / kSeedStretch, blocks = (threads + kSeedThreads - 1) / kSeedThreads;
  if (blocks > 0x7FFFFFFFll) return fail(ctx, MI355_SW_ENOTSUP, "range too long for the seed scan");
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t o_bucket = up16(t.slots.size() * 4), o_read = o_bucket + up16(t.bucket.size() * 4), o_off = o_read + up16(ns * 4),
               o_codes = o_off + up16(ns * 4), total = o_codes + up16(ns * (size_t)k);
  const size_t h_start = up16(nq * 4), h_off = h_start + nq * kSeedHitCap * 8, h_total = h_off + nq * kSeedHitCap * 4;
  if (ctx->seed_tab.ensure(total + 16) || ctx->seed_hits.ensure(h_total + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(seed table) failed");
  std::vector<uint8_t> blob(total, 0);
  memcpy(blob.data(), t.slots.data(), t.slots.size() * 4);
  memcpy(blob.data() + o_bucket, t.bucket.data(), t.bucket.size() * 4);
  memcpy(blob.data() + o_read, t.read.data(), ns * 4);
  memcpy(blob.data() + o_off, t.off.data(), ns * 4);
  memcpy(blob.data() + o_codes, t.codes.data(), ns * (size_t)k);
  HIPCHK(ctx, hipMemcpyAsync(ctx->seed_tab.p, blob.data(), total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->seed_hits.p, 0, h_start, ctx->stream));
  uint8_t *tab = ctx->seed_tab.as<uint8_t>(), *out = ctx->seed_hits.as<uint8_t>();
  SeedArgs a;
  a.codes = ref.codes.as<uint8_t>() + rg.lo; a.n = n; a.k = k; a.bk = t.bk;
  a.slots = reinterpret_cast<const uint2 *>(tab); a.bits = t.bits; a.bucket_log2 = t.bucket_log2;
  a.bucket = reinterpret_cast<const uint32_t *>(tab + o_bucket);
  a.seed_read = reinterpret_cast<const int32_t *>(tab + o_read); a.seed_off = reinterpret_cast<const int32_t *>(tab + o_off);
  a.seed_codes = tab + o_codes;
  a.count = reinterpret_cast<unsigned int *>(out); a.hit_start = reinterpret_cast<int64_t *>(out + h_start); a.hit_off = reinterpret_cast<int32_t *>(out + h_off);
  hipLaunchKernelGGL(sw_seed_scan_kernel, dim3((unsigned)blocks), dim3(kSeedThreads), t.bucket.size() * 4, ctx->stream, a);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(count.data(), out, nq * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(start.data(), out + h_start, nq * kSeedHitCap * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(hoff.data(), out + h_off, nq * kSeedHitCap * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// The background table (PrefixBackground) of the heights Rs for this reference, score table and range: kCalibReads prefixes cut from
// the reference itself at evenly spaced offsets — a function of the reference alone — swept by the step tiles of every height over
// the first kCalibCols columns of the range; each prefix's home sub-chunks left out, the rest counted per value and scaled to the
// range's sub-chunks.  One small launch per height, once per (reference, table, range): in real use the reference and the scoring
// stay while the batches change, and the table does not depend on the batch.  ctx->pbg.valid is left false where it cannot be
// measured (a range too short to cut the prefixes from).
constexpr int kCalibReads = 16;
constexpr int kCalibKeep = 12;                                         // prefixes whose tails make the table: the lowest three quarters at every value
constexpr int64_t kCalibCols = (int64_t)4 << 20;
int prefix_background(mi355_sw_ctx *ctx, const RefData &ref, const Range &rg, const mi355_sw_params &p, const ScoreTable &table,
                      const Bucket &like, const std::vector<int> &Rs) {
  PrefixBackground &g = ctx->pbg;
  if (g.valid && g.ref == (const void *)&ref && g.ref_version == ref.version && g.lo == rg.lo && g.hi == rg.hi && g.gap == table.gap &&
      g.smax == table.smax && g.R == Rs && g.stab == table.stab)
    return 0;
  HostTrace trace_("prefix_background");
  g.valid = false;
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t n = rg.hi - rg.lo;
  const int L = kPrefixLanes * Rs.back() + 2;                          // (longer than the tallest prefix: prefix tiles take the rows of LONGER reads)
  if (n < (int64_t)64 * kCalibReads * L) return 0;
  std::vector<std::vector<char>> cut(kCalibReads, std::vector<char>((size_t)L));
  std::vector<int64_t> at(kCalibReads);
  std::vector<const char *> xs(kCalibReads);
  std::vector<size_t> nxs(kCalibReads, (size_t)L);
  for (int i = 0; i < kCalibReads; ++i) {
    at[i] = std::min<int64_t>(n - L, (2 * (int64_t)i + 1) * n / (2 * kCalibReads));
    HIPCHK(ctx, hipMemcpy(cut[i].data(), ref.bytes.as<uint8_t>() + rg.lo + at[i], (size_t)L, hipMemcpyDeviceToHost));
    xs[i] = cut[i].data();
  }
  int rc = upload_queries(ctx, ctx->calib_q, kCalibReads, xs.data(), nxs.data());
  if (rc) return rc;
  const QueryBatch &cq = ctx->calib_q;
  const Range srg{rg.lo, std::min(rg.hi, rg.lo + kCalibCols)};
  const std::vector<Range> ranges{srg};
  const int64_t ns = srg.hi - srg.lo;
  // (the calibration is no pass of the call: what describes the call's sweep stays as it was)
  const mi355_sw_kernel_info kept_kernel = ctx->last_kernel;
  const bool kept_named = ctx->prefix_named;
  const double kept_launches = ctx->timings[4], kept_cells = ctx->timings[5];
  const std::string kept_path = ctx->path;
  struct Restore {                                                       // on every way out of the launches below, once
    std::function<void()> f;
    bool armed = true;
    void run() { if (armed) f(); armed = false; }
    ~Restore() { run(); }
  } restore_{[&]() { ctx->last_kernel = kept_kernel; ctx->prefix_named = kept_named; ctx->timings[4] = kept_launches; ctx->timings[5] = kept_cells; ctx->path = kept_path; }};
  g.R = Rs; g.tail.assign(Rs.size(), std::vector<double>());
  for (size_t h = 0; h < Rs.size(); ++h) {
    const int R = Rs[h], P = kPrefixLanes * R, top = table.smax * P;
    rc = score_begin(ctx, cq, ranges, table);
    if (rc) return rc;
    if (ctx->pkeys.ensure((size_t)kCalibReads * 8 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
    HIPCHK(ctx, hipMemsetAsync(ctx->pkeys.p, 0, (size_t)kCalibReads * 8, ctx->stream));
    Bucket pb = like;
    pb.first = 0; pb.count = kCalibReads;
    pb.SL = kPrefixLanes; pb.R = R; pb.prefix = true; pb.rowp = true; pb.step = true; pb.second = true;
    ScoreIO io;
    io.range_lo = ctx->ranges.as<int64_t>(); io.range_hi = ctx->ranges.as<int64_t>() + 1; io.keys = ctx->pkeys.as<unsigned long long>();
    rc = score_launch(ctx, ref, cq, ranges, p, table, pb, &io);
    if (rc) return rc;
    std::vector<unsigned long long> keys;
    rc = score_fetch(ctx, kCalibReads, keys, ctx->pkeys.p);
    if (rc) return rc;
    const int64_t E = pb.sub_len, stride = ((ns + pb.chunk_len - 1) / pb.chunk_len) * (pb.chunk_len / E), nsub = (ns + E - 1) / E;
    if (h == 0) g.E = E;
    if (E != g.E) return 0;
    std::vector<uint16_t> raw((size_t)kCalibReads * (size_t)stride);
    HIPCHK(ctx, hipMemcpy(raw.data(), ctx->submax.p, raw.size() * 2, hipMemcpyDeviceToHost));
    // one tail per prefix, scaled to the range; the table is the mean of the kCalibKeep lowest at every x: a quarter of the prefixes
    // may come out of a repeat family (thousands of sub-chunks near the full score, which say nothing about a read from elsewhere)
    // without moving it.  A read out of such a family is then forecast too low, offends its pass by the cap and moves on, as in the chain.
    std::vector<std::vector<double>> tails(kCalibReads, std::vector<double>((size_t)top + 1, 0.0));
    bool all_counted = true;
    for (int r = 0; r < kCalibReads; ++r) {
      const int64_t home = at[cq.order[r]];                              // (relative to the range, as the sample is)
      const int64_t x0 = (home - E) / E, x1 = (home + L + E) / E;          // the prefix's own copy, its lag and its decay
      std::vector<double> hist((size_t)top + 1, 0.0);
      double counted = 0;
      for (int64_t s = 0; s < nsub; ++s) {
        if (s >= x0 && s <= x1) continue;
        const long v = std::lround(half_value(raw[(size_t)r * (size_t)stride + (size_t)s]) * kF16Scale);
        hist[(size_t)std::max(0l, std::min<long>(v, top))] += 1.0;
        counted += 1.0;
      }
      if (counted < 1.0) { all_counted = false; break; }
      const double scale = ((double)n / (double)E) / counted;
      double acc = 0;
      for (int x = 0; x <= top; ++x) { acc += hist[(size_t)(top - x)]; tails[r][(size_t)x] = acc * scale; }
    }
    if (!all_counted) return 0;
    g.tail[h].assign((size_t)top + 1, 0.0);
    for (int x = 0; x <= top; ++x) {
      double col[kCalibReads];
      for (int r = 0; r < kCalibReads; ++r) col[r] = tails[r][(size_t)x];
      std::sort(col, col + kCalibReads);
      double sum = 0;
      for (int r = 0; r < kCalibKeep; ++r) sum += col[r];
      g.tail[h][(size_t)x] = sum / kCalibKeep;
    }
  }
  restore_.run();                                                        // (here, in front of the call's own note below)
  g.valid = true; g.ref = (const void *)&ref; g.ref_version = ref.version; g.lo = rg.lo; g.hi = rg.hi; g.gap = table.gap; g.smax = table.smax;
  g.stab = table.stab;
  ctx->prefix_calibrated += 1;
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  path_note(ctx, "prefix_calibrated[heights=%zu,ms=%.2f]", Rs.size(), ms);
  return 0;
}
// expected background sub-chunks of a read with deficit d (score units below smax m) at height R; huge where the table has no such height
double background_flags(const PrefixBackground &g, int R, long d) {
  for (size_t h = 0; h < g.R.size(); ++h)
    if (g.R[h] == R && !g.tail[h].empty()) return g.tail[h][(size_t)std::max(0l, std::min<long>(d, (long)g.tail[h].size() - 1))];
  return 1.0e30;
}

// The seeded flow of a bucket of at least kPrefixChain reads, in place of prefix_chain's probe:
//   seeds:   disjoint k-letter seeds of every read, one scan of the range (seed_scan), the hits of a read clustered by diagonal within
//            ceil(smax m / g) (sw_seed_kernel.h seed_cluster: most distinct seeds, then the lowest diagonal); a read without a hit, or
//            with more than kSeedHitCap, has no seed (a repeat family would steer by the order of the atomics);
//   B0:      the sub-chunks that hold the end columns of the cluster go through locate_flagged as round 1's list does in prefix_bucket:
//            the located score is an exact alignment score, B0 <= B, which is all L19 and L20 ask of it;
//   settled: a read whose hits are all listed and whose deficit d = smax m - B0 breaks fewer seeds than it has in the table,
//            floor(d / min(g, smax)) < u, has an intact seed in every alignment of score >= B0: the windows of ALL
//            its hits go through one more locate, the first maximum over them and the seed windows is its result, and it joins no
//            pass (seed_certify[n=..,windows=..]; option no_seed_certify, size gate seed_certify_min_cols).  A bucket settled whole
//            launches no score kernel at all;
//   height:  every other seeded read takes the lowest height P of prefix_heights_seeded with B0 > prefix_bound(P) whose background table
//            (prefix_background) expects at most query_flag_cap flags at the read's deficit; none: the full sweep, at once;
//   groups:  one pass per height that has a read, ascending, B0 given (PrefixAsk::given); whether a group of fewer than kSeedGroupMin
//            reads rides with a taller one is kSeedRideDefault's business (below: it does not).  The reads without a seed take the
//            chain's lowest height with B0 from their prefix key, as in prefix_chain;
//   after:   an offender of a pass takes ONE more pass, at the next height whose bound and table admit it, else it is an offender of
//            the bucket (requery).
// used = false: the stage did not apply (gates) or failed — more than half of the bucket without a seed B0, path note
// prefix_seed_failed — and nothing was settled: the caller runs prefix_chain as ever.
// kSeedGroupMin: a pass of its own saves n (P' - P) read-rows at the bulk rate of 1.85 us per read-row (50 Mbp) and pays what small
// passes were measured to cost, 2.2 - 2.5 us per read-row on 64 - 150 reads: at 2.5 against 1.85 a pass of its own loses whenever
// P / P' > 0.74, which holds for every pair of neighbouring heights (16 / 20, 20 / 26, 26 / 32, 32 / 38).  No pass between 150 and
// 960 reads has been measured; 256 is where a pass fills the chip with one tile per slot several times over and is taken as bulk.
// (The 2.2 - 2.6 us per read-row of a small pass were measured on the main pass's 16384-column tiles.  Since prefix_group_tile_len,
// host_score.h, a group's pass on a long range takes tiles by its launch's fill — kPrefixFillF0, kPrefixFillCap there, beside the
// rule that score_launch needs them for: 121 reads at P = 26 then run at 2.3 us per read-row, profiles/prefix_group_tiles_ab.json.)
constexpr int64_t kPrefixSeedMinCols = (int64_t)4 << 20;
constexpr size_t kSeedGroupMin = 256;
// The size gate of the settled reads (option seed_certify_min_cols), apart from prefix_seed_min_cols.  It has no performance reason:
// L21 holds at any size.  tests/test_gpu_prefix_seed_flow.py lowers prefix_seed_min_cols to 1 on a reference of 1 Mi columns and pins
// the group passes it sees there, three heights with the lowest on a low tile; with this gate left alone that file goes on testing
// the group passes, which a batch of mostly settled reads would no longer run.
constexpr int64_t kSeedCertifyMinCols = kPrefixSeedMinCols;
// How a group below kSeedGroupMin rides (option seed_ride): with the next taller group whatever its own height (cascade: 26 -> 32 ->
// 38), only while its OWN height is above kSeedRideRatio of the host's (near: the 0.74 of the argument above, which 26 / 38 = 0.68
// misses), or not at all (none: one pass per height that has a read).  Measured on the bench batch's residual, 121 / 39 / 3 reads at
// P = 26 / 32 / 38 after 1885 settled (bench.py, 20 steps, each rule twice, ms per step and score kernels alone): cascade 18.95 and
// 19.34 (14.6), near 18.26 and 18.35 (13.5), none 18.25 and 17.81 (11.9; 17.65 - 17.67 in three further runs).  The kernels follow
// the read-rows, 6194 / 5468 / 4508, at 2.4 - 2.6 us each whatever the pass's size: the small passes' rate that kSeedGroupMin's
// argument charges a pass of its own is paid by the riders too once every pass is small, and a further pass costs 0.3 - 0.4 ms of
// thin and locate launches.  So: none.
constexpr long kSeedRideCascade = 1, kSeedRideNear = 2, kSeedRideNone = 3;
constexpr double kSeedRideRatio = 0.74;
constexpr long kSeedRideDefault = kSeedRideNone;
// L21 charges every broken seed c = min(g, smax) or more; a substitution costs smax - s(a, b), so the rule is used only with tables
// whose mismatches of letters the reference holds all score smax - c or less (match / mismatch scoring with mismatch <= 0 always).
bool seed_certify_table_ok(const RefData &ref, const ScoreTable &t) {
  if (!t.integral || t.gap <= 0 || t.smax <= 0) return false;
  const int nc = ref.ncodes, c = std::min(t.gap, t.smax);
  for (int a = 0; a < 256; ++a) {
    if (ref.code_of[a] < 0) continue;
    for (int y = 0; y < nc - 1; ++y)
      if (y != ref.code_of[a] && (int)t.stab[(size_t)a * nc + y] > t.smax - c) return false;
  }
  return true;
}
constexpr int64_t kSeedEndPad = 16;                                    // columns an indel behind the last hit may move the end cell
int prefix_seeded(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg, const mi355_sw_params &p,
                  const ScoreTable &table, const Bucket &b, std::vector<int64_t> &qchunk, std::vector<int64_t> &qwarm,
                  std::vector<Located> &loc, std::vector<char> &qdone, std::vector<int> &offenders, bool &used) {
  used = false;
  const int64_t n = rg.hi - rg.lo;
  const long gate = opt().prefix_seed_min_cols;
  if (opt().no_prefix_seed || opt().no_prefix_step || n < (gate > 0 ? (int64_t)gate : kPrefixSeedMinCols)) return 0;
  HostTrace trace_("prefix_seeded");
  const size_t nq = q.nq;
  const int minlen = q.len[q.order[b.first]];
  const int k = seed_k(ref.ncodes - 1, minlen, n);
  if (k == 0) return 0;
  const std::vector<int> hs = prefix_heights_seeded(table, b, minlen);
  const int chainR = prefix_heights(table, b, minlen, true)[0];        // where prefix_chain would probe: the seedless reads' height
  std::vector<int32_t> ids(q.order.begin() + b.first, q.order.begin() + b.first + b.count);
  std::vector<uint32_t> count;
  std::vector<int64_t> start;
  std::vector<int32_t> hoff;
  std::vector<uint32_t> usable;
  HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
  int rc = seed_scan(ctx, ref, q, rg, ids, k, count, start, hoff, &usable);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
  const float scan_us = elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  // the windows: the sub-chunks (of the passes' own length) that hold the columns the cluster's alignments end in
  Bucket tb = b;
  tb.SL = kPrefixLanes; tb.prefix = true;
  const int64_t E = score_sub_len(p.semantics, tb);
  std::vector<std::pair<uint32_t, uint32_t>> f0;
  std::vector<char> given(nq, 0);
  size_t nhits = 0, seedless = 0;
  for (int id : ids) {
    const uint32_t c = count[id];
    nhits += c;
    bool ok = c > 0 && c <= (uint32_t)kSeedHitCap;
    int64_t lo = 0, hi = 0;
    int distinct = 0;
    if (ok) {
      std::vector<SeedHit> hits(c);
      for (uint32_t j = 0; j < c; ++j) hits[j] = SeedHit{start[(size_t)id * kSeedHitCap + j], hoff[(size_t)id * kSeedHitCap + j]};
      const int64_t m = q.len[id];
      ok = seed_cluster(hits, ((int64_t)table.smax * m + table.gap - 1) / table.gap, lo, hi, distinct);
      const int64_t c_lo = std::max<int64_t>(0, lo + m - 1 - kSeedEndPad), c_hi = std::min<int64_t>(n - 1, hi + m - 1 + kSeedEndPad);
      ok = ok && c_lo <= c_hi;
      if (ok) for (int64_t s = c_lo / E; s <= c_hi / E; ++s) f0.push_back({(uint32_t)id, (uint32_t)s});
    }
    if (ok) given[id] = 1; else ++seedless;
  }
  ctx->prefix_seed_hits += nhits;
  path_note(ctx, "prefix_seed[k=%d,hits=%zu,scan_us=%.0f]", k, nhits, (double)scan_us);
  if (2 * seedless > (size_t)b.count) { path_note(ctx, "prefix_seed_failed"); return 0; }
  // B0: round 1 on the seed windows
  const std::vector<Range> ranges{rg};
  rc = score_begin(ctx, q, ranges, table);
  if (rc) return rc;
  for (int id : ids) { qchunk[id] = E; qwarm[id] = b.warm; }
  std::sort(f0.begin(), f0.end());
  const std::vector<float> qlow(nq, 0.0f);                             // (no lower bound is known yet: the bucket's whole margin)
  std::vector<Located> loc0(nq);
  std::vector<char> done0(nq, 0);
  HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
  rc = locate_flagged(ctx, ref, q, rg, p, qchunk, qwarm, qlow, table, f0, loc0, done0);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
  ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
  std::vector<float> B0(nq, 0.0f);
  size_t nseeded = 0;
  for (int id : ids) {
    if (given[id] && done0[id] && loc0[id].score > 0.0f) { B0[id] = loc0[id].score; ++nseeded; }
    else given[id] = 0;
  }
  if (2 * ((size_t)b.count - nseeded) > (size_t)b.count) { path_note(ctx, "prefix_seed_failed"); return 0; }
  // settled: the reads an intact seed must find (L21) — B0 from the seed windows, every hit listed, floor(d / c) < u.  Chosen here on
  // the host; their windows are evaluated below, once the flow is known to go on.
  std::vector<char> settled(nq, 0);
  size_t nsettled = 0;
  const long cgate = opt().seed_certify_min_cols;
  if (!opt().no_seed_certify && n >= (cgate > 0 ? (int64_t)cgate : kSeedCertifyMinCols) && seed_certify_table_ok(ref, table)) {
    for (int id : ids) {
      if (!given[id] || count[id] > (uint32_t)kSeedHitCap) continue;
      const int64_t d = (int64_t)table.smax * q.len[id] - (int64_t)std::lround((double)B0[id]);
      if (seed_certify_ok(d, table.smax, table.gap, usable[id])) { settled[id] = 1; ++nsettled; }
    }
  }
  if (nsettled < (size_t)b.count) {                                     // (a bucket that is settled whole asks no height of anybody)
    rc = prefix_background(ctx, ref, rg, p, table, b, hs);
    if (rc) return rc;
    if (!ctx->pbg.valid || ctx->pbg.E != E) { path_note(ctx, "prefix_seed_failed"); return 0; }
  }
  ctx->candidates += f0.size();
  ctx->prefix_seeded += nseeded;
  // heights and groups
  const uint32_t qcap = query_flag_cap(nq);
  auto admits = [&](int R, int id) {
    const int P = kPrefixLanes * R, m = q.len[id];
    if (m <= P || !(B0[id] > prefix_bound(table, m, P, 0.0f, true))) return false;
    return background_flags(ctx->pbg, R, std::lround((double)table.smax * m - (double)B0[id])) <= (double)qcap;
  };
  std::map<int, std::vector<int>> groups;
  std::vector<int> none;                                                // no height can certify them: they pay for no pass
  for (int id : ids) {
    if (settled[id]) continue;                                          // (joins no group)
    if (!given[id]) { groups[chainR].push_back(id); continue; }
    int R = 0;
    for (int r : hs) if (admits(r, id)) { R = r; break; }
    if (R) groups[R].push_back(id);
    else none.push_back(id);
  }
  if (2 * none.size() > (size_t)b.count && (size_t)b.count == nq) {
    // most of the bucket is beyond every height (10 % substitutions: deficits of 90 and more) and the bucket is the whole batch: the
    // caller sweeps the whole batch again whatever the others do (whole_again), so nobody pays for a pass — what such a batch pays
    // for the filter is the scan and the seed windows, not a probe.  (With other buckets in the call that rule may not fire: then the
    // reads a height can certify take their passes below, and only the others go to the sweep.)
    offenders.insert(offenders.end(), ids.begin(), ids.end());
    path_note(ctx, "prefix_seed_hopeless[n=%zu]", none.size());
    used = true;
    return 0;
  }
  offenders.insert(offenders.end(), none.begin(), none.end());
  // (The "more than half" tests above — seedless, no seed B0, beyond every height — all count over the whole bucket with the settled
  // reads on the side that is served: a settled read has a seed, a B0, and needs no height.  A hopeless batch is swept whole, so it
  // returned before anything was settled.)
  if (nsettled) {
    // L21: every cell with H >= B0 ends in the window of one of the read's hits.  The sub-chunks of ALL hits' windows, less what the
    // seed windows above evaluated, go through one more locate with B0 as the lower bound (as round 2 of prefix_bucket); the read's
    // result is the first maximum over both, and it is final.
    std::vector<std::pair<uint32_t, uint32_t>> fc, fcnew;
    for (int id : ids) {
      if (!settled[id]) continue;
      const int64_t m = q.len[id], d = (int64_t)table.smax * m - (int64_t)std::lround((double)B0[id]);
      for (uint32_t j = 0; j < count[id]; ++j) {
        int64_t c_lo = 0, c_hi = 0;
        if (!seed_certify_window(start[(size_t)id * kSeedHitCap + j], m, d, table.smax, table.gap, n, c_lo, c_hi)) continue;
        for (int64_t s = c_lo / E; s <= c_hi / E; ++s) fc.push_back({(uint32_t)id, (uint32_t)s});
      }
    }
    std::sort(fc.begin(), fc.end());
    fc.erase(std::unique(fc.begin(), fc.end()), fc.end());
    std::set_difference(fc.begin(), fc.end(), f0.begin(), f0.end(), std::back_inserter(fcnew));
    std::vector<Located> locc(nq);
    std::vector<char> donec(nq, 0);
    if (!fcnew.empty()) {
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      rc = locate_flagged(ctx, ref, q, rg, p, qchunk, qwarm, B0, table, fcnew, locc, donec);
      if (rc) return rc;
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
    }
    for (int id : ids) {
      if (!settled[id]) continue;
      Located best = loc0[id];                                          // (B0 came from it)
      const int64_t m = q.len[id];
      if (donec[id] && (locc[id].score > best.score ||
                        (locc[id].score == best.score && host_order_key(p.semantics, locc[id].ix, locc[id].iy, m, n) < host_order_key(p.semantics, best.ix, best.iy, m, n))))
        best = locc[id];
      loc[id] = best; qdone[id] = 1;                                    // (qchunk / qwarm: set for the seed windows above)
    }
    ctx->candidates += fcnew.size();
    ctx->seed_certified += nsettled;
    path_note(ctx, "seed_certify[n=%zu,windows=%zu]", nsettled, fcnew.size());
  }
  const long ride = opt().seed_ride > 0 ? opt().seed_ride : kSeedRideDefault;
  std::vector<int> ownR(nq, 0);                                         // the height the read was given, wherever it rides
  for (const auto &gr : groups) for (int id : gr.second) ownR[id] = gr.first;
  for (auto it = groups.begin(); it != groups.end() && ride != kSeedRideNone;) {
    auto nx = std::next(it);
    if (nx == groups.end() || it->second.size() >= kSeedGroupMin) { ++it; continue; }
    std::vector<int> stay;
    for (int id : it->second) {
      if (ride == kSeedRideNear && !((double)ownR[id] > kSeedRideRatio * (double)nx->first)) stay.push_back(id);
      else nx->second.push_back(id);
    }
    if (stay.empty()) it = groups.erase(it);
    else { it->second.swap(stay); ++it; }
  }
  size_t biggest = 0;
  for (const auto &gr : groups) biggest = std::max(biggest, gr.second.size());
  std::vector<char> again(nq, 0);
  for (auto it = groups.begin(); it != groups.end(); ++it) {
    const int R = it->first;
    const std::vector<int> members(it->second);
    QueryBatch qv;
    Bucket vb;
    rc = prefix_view(ctx, q, members, ctx->psel2, qv, b, vb);
    if (rc) return rc;
    path_note(ctx, "prefix_group[R=%d,n=%zu]", R, members.size());
    bool gave_up = false;
    std::vector<int> roff;
    PrefixAsk ask;
    ask.step = true; ask.second = members.size() != biggest;           // (last_kernel describes the largest group, cells are everybody's)
    ask.bulk = true;
    ask.B0 = &B0; ask.gave_up = &gave_up; ask.given = &given; ask.f1 = &f0; ask.f1_E = E; ask.loc1 = &loc0;
    rc = prefix_bucket(ctx, ref, qv, rg, p, table, vb, R, true, qchunk, qwarm, loc, qdone, roff, ask);
    if (rc) return rc;
    for (int id : roff) {
      int next = 0;
      if (!gave_up && !again[id])
        for (int r : hs) if (r > R && admits(r, id)) { next = r; break; }
      if (next) { groups[next].push_back(id); again[id] = 1; ctx->prefix_second_pass += 1; }
      else offenders.push_back(id);
    }
  }
  used = true;
  return 0;
}

// All queries of `q` against one range of the reference: argmax cells and traceback views (into buffers the context
// keeps until its next call), indexed by query id.
// `pre` (mi355_sw_align_scored_range): the keys of an earlier mi355_sw_score_ranges sweep over this very range stand in
// for the score pass.
int align_range_core(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
                     const mi355_sw_params &p, int flags, std::vector<Located> &loc, std::vector<TraceOut> &tout,
                     const ScoredRanges *pre = nullptr, size_t pre_range = 0) {
  HostTrace trace_("align_range");
  const bool want_trace = !(flags & MI355_SW_SCORE_ONLY);
  const size_t nq = q.nq;
  const int64_t n = rg.hi - rg.lo;
  HIPCHK(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
  // (half a million small alignments per call: the per-query host arrays are sized only where a path reads them)
  PoolFromScope pool_from_;
  loc.resize(nq);
  tout.resize(want_trace ? nq : 0);
  auto fill_defaults = [&loc, &tout, nq, want_trace]() {
    HostTrace t_("  per-query arrays");
    parallel_for(nq, [&](size_t k0, size_t k1) {
      std::fill(loc.begin() + k0, loc.begin() + k1, Located());
      if (want_trace) std::fill(tout.begin() + k0, tout.begin() + k1, TraceOut());
    });
  };
  // The many-small-alignments batch (below: nothing takes the score kernel) touches these arrays only once its results are down:
  // the defaults are then written while the device works (exact_full_device runs ctx->while_device_works in front of its first
  // wait) — 31 MB of host stores for config 4's 561 356 alignments
  const bool devlist_first = !pre && n < 1024 && p.semantics == MI355_SW_F32 && wave_scoring_ok(p) && !opt().no_wave && !opt().no_devlist;
  if (devlist_first) ctx->while_device_works = fill_defaults;
  else fill_defaults();
  struct RunPending {                                              // (every exit: the deferred work is done or dropped, never left behind)
    mi355_sw_ctx *c;
    ~RunPending() { c->while_device_works = nullptr; }
  } run_pending_{ctx};
  // No score can be positive (uint8 engine whose match score saturates to 0; float engine whose best substitution
  // score is <= 0 with a positive gap): every cell of the matrix is 0 and the defined no-match result stands.
  bool all_zero = false;
  if (p.semantics == MI355_SW_U8SAT) all_zero = u8_params(p).M == 0;
  if (n >= 1 && nq > 0 && !all_zero) {
    const ScoreTable table = plan_table(ref, p);
    if (p.semantics == MI355_SW_F32 && table.ok && !(table.smaxf > 0)) all_zero = true;
  }
  if (n >= 1 && nq > 0 && !all_zero) {
    const ScoreTable table = plan_table(ref, p);
    // references shorter than 1024 columns never take the score kernel (bucket_fast_ok): skip the length classes
    std::vector<Bucket> buckets;
    // the float engine's saturating float16 sweep (make_buckets) needs the strip kernel for its flagged sub-chunks
    bool allow_sat = p.semantics == MI355_SW_F32 && strip_scoring_ok(ref, p);
    // ... and so does the sampled running maximum (sw_score_kernel MK), for the sub-chunks within its slack of the key
    bool allow_sample = strip_scoring_ok(ref, p);
    const size_t nsweep = (n >= 1024 || pre) ? nq : 0;             // only the score-kernel paths (below) index these
    std::vector<char> qfast(nq, 0), qfloat(nsweep, 0), qsat(nsweep, 0), qdone(nsweep, 0);
    std::vector<int64_t> qchunk(nsweep, 0), qwarm(nsweep, 0);
    std::vector<unsigned long long> keys;
    bool any_fast = false;
    if (pre) {
      qfast = pre->qfast; qfloat = pre->qfloat; qchunk = pre->qchunk; qwarm = pre->qwarm;
      keys.assign(pre->keys.begin() + pre_range * nq, pre->keys.begin() + (pre_range + 1) * nq);
      ctx->fshift = pre->fshift;
      for (size_t k = 0; k < nq; ++k) any_fast |= qfast[k] != 0;
      if (pre->sampled && nq == 1 && pre->has_located[pre_range]) { loc[0] = pre->located[pre_range]; qdone[0] = 1; }
    }
    ctx->long_margin = 0;
    // sw_long_kernel swept with an optimistic warm-up margin (long_score_launch): the lone query's maximum must lie above what
    // that margin certifies, else the sweep is repeated with the margin this maximum needs (which then certifies it)
    auto margin_certified = [&](float best) {
      if (!(ctx->long_cert >= 0.0f) || best > ctx->long_cert) return true;
      const double m = (double)q.maxlen;
      ctx->long_margin = (int64_t)(m + std::ceil(((double)table.smax * m - (double)best) / (double)table.gap)) + 2 + 64;
      if (!ctx->prefix_named) ctx->last_kernel.cells = 0;          // (cells swept by a prefix filter of this call stay counted)
      ctx->timings[4] = 0; ctx->timings[5] = 0;
      ctx->whole_again += 1;
      path_note(ctx, "margin_again");
      return false;
    };
    // uint8 engine, EARLY EXIT.  The maximum never exceeds 255, and the answer is the 255 that comes first in the
    // skewed storage order: on the lowest anti-diagonal i + j — so within the first sub-chunk s1 that truly holds a 255 or its right
    // neighbour (sub-chunks are longer than |x| + 64 columns) — unless the wrapped bottom-right triangle (the last two
    // sub-chunks) holds one, which the layout stores in front of everything.  Reads whose random BACKGROUND reaches the cap
    // (beyond ~300 bp at 3 / -3 / 2: the linear regime, about 0.6 per row) hold a 255 within the reference's first few hundred
    // columns: when the exact evaluation of sub-chunks 0 and 1 and of the last two finds a 255 in sub-chunk 0, that is s1 = 0,
    // every candidate has been evaluated, and the sweep of the remaining reference cannot change (maximum, first cell) — it is
    // skipped.  (The reference sweeps it all the same; its answer for such reads is decided where the matrix first saturates.)
    bool all_early = false;
    if (!pre && p.semantics == MI355_SW_U8SAT && n >= 1024 && allow_sample && !opt().no_u8_early && nq <= 4096 && table.ok) {
      std::vector<Bucket> bk = make_buckets(ref, q, table, p, n, false, false);
      std::vector<int64_t> echunk(nq, 0), ewarm(nq, 0);
      std::vector<float> elow(nq, 255.0f);
      std::vector<char> edone(nq, 0);
      std::vector<std::pair<uint32_t, uint32_t>> ff;
      bool likely = !bk.empty();
      for (Bucket &b : bk) {
        likely = likely && bucket_fast_ok(ref, table, b, n, p) && 0.3 * (double)table.smax * (double)q.len[q.order[b.first]] >= 255.0;
        if (!likely) break;
        const int64_t E = score_sub_len(p.semantics, b), nsub = (n + E - 1) / E;
        for (int k = 0; k < b.count; ++k) {
          const int id = q.order[b.first + k];
          echunk[id] = E; ewarm[id] = b.warm;
          int64_t seen[4]; int ns = 0;
          for (int64_t s : {(int64_t)0, (int64_t)1, nsub - 2, nsub - 1}) {
            bool dup = s < 0 || s >= nsub;
            for (int t = 0; t < ns; ++t) dup = dup || seen[t] == s;
            if (!dup) { seen[ns++] = s; ff.push_back({(uint32_t)id, (uint32_t)s}); }
          }
        }
      }
      if (likely && !ff.empty()) {
        HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
        int rc = locate_saturated(ctx, ref, q, rg, p, echunk, ewarm, elow, table, ff, loc, edone);
        if (rc) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
        all_early = true;
        for (size_t k = 0; k < nq && all_early; ++k) {
          const bool wrapped = loc[k].ix + loc[k].iy > n && n >= (int64_t)q.len[k];
          all_early = edone[k] && loc[k].score == 255.0f && (loc[k].iy - 1 < echunk[k] || wrapped);
        }
        if (all_early) {
          for (size_t k = 0; k < nq; ++k) { qfast[k] = 1; qdone[k] = 1; qchunk[k] = echunk[k]; qwarm[k] = ewarm[k]; }
          any_fast = true;
          ctx->early_settled += nq;
          path_note(ctx, "u8_early");
        } else {
          for (size_t k = 0; k < nq; ++k) loc[k] = Located();       // (the sweep decides for everybody)
        }
      }
    }
    // Prefix filter (lemma L19) in front of the sweep: the buckets it takes are settled here read by read; its offenders and the
    // queries of every other bucket form the view `qs` that the sweep below works on (requery: they are swept on all their rows)
    QueryBatch qrest;
    const QueryBatch *qs = &q;
    bool all_prefix = false;
    if (!pre && !all_early && p.semantics == MI355_SW_F32 && !opt().no_prefix && nq >= 2 && n >= 1024 && n >= prefix_cols_min() && table.ok &&
        rg.lo == 0 && (size_t)rg.hi == ref.n) {                        // (one range: the whole reference)
      std::vector<Bucket> bk = make_buckets(ref, q, table, p, n, allow_sat, allow_sample);
      std::vector<int> offenders;
      const size_t candidates_before = ctx->candidates;
      std::vector<char> tried(nq, 0);
      size_t ntried = 0;
      for (Bucket &b : bk) {
        b.fast = bucket_fast_ok(ref, table, b, n, p);
        if (!prefix_ok(table, b, q.len[q.order[b.first]], n, p)) continue;
        // A large bucket is PROBED first: its first kPrefixProbe reads alone (the shortest: the hardest to certify).  When more than half
        // of them offend — reads that differ too much from the reference for their first P rows to decide — the rest of the bucket
        // skips the filter and is swept as ever: what such a batch pays for the filter is the probe (CHANGELOG.md: 10 % substitutions),
        // not a prefix sweep of every read.  (A failed probe of the call's only eligible bucket ends in the rule below: whole_again.)
        // The probe also picks the HEIGHT (option no_prefix_low: not): it runs at the next lower listed R that is still eligible, on tiles
        // that fold row P alone (rowp_slack instead of sample_slack: a lower prefix certifies what the bucket's own certifies with
        // the fold over all rows).  B0 is an exact alignment score, whatever the height that found its window:
        //   * at most kPrefixProbe / 16 of the probe offend: the rest of the bucket runs at the low height;
        //   * more than half cannot be certified at the bucket's own R under the row-P fold either — B0 is not above that bound, or
        //     that threshold already draws more flags than the cap on the rows of the probe (prefix_bucket: vote): the probe has
        //     failed, as above;
        //   * else the rest runs at the bucket's own R with the row-P fold, and with it the probe's offenders that this height can
        //     certify (the others stay offenders).
        // A probed bucket of at least kPrefixChain reads takes its heights as a chain, with one taller pass for the offenders of the
        // height it starts at (prefix_chain; options no_prefix_cascade, no_prefix_low: the flow below, as for the smaller buckets)
        if (b.count >= kPrefixChain && !opt().no_prefix_cascade && !opt().no_prefix_low) {
          // ... unless seed hits give most of its reads their B0 before any sweep: then every read runs at the lowest height that can
          // certify IT, and there is no probe (prefix_seeded; option no_prefix_seed, size gate prefix_seed_min_cols)
          bool failed = false, seeded = false;
          int rc = prefix_seeded(ctx, ref, q, rg, p, table, b, qchunk, qwarm, loc, qdone, offenders, seeded);
          if (rc) return rc;
          if (!seeded) rc = prefix_chain(ctx, ref, q, rg, p, table, b, qchunk, qwarm, loc, qdone, offenders, failed);
          if (rc) return rc;
          const int ndone = failed ? kPrefixProbe : b.count;
          for (int k = 0; k < ndone; ++k) tried[q.order[b.first + k]] = 1;
          ntried += (size_t)ndone;
          continue;
        }
        Bucket part = b;
        int restR = b.R;
        bool rest_rowp = false;
        std::vector<int> riders;
        if (b.count >= 8 * kPrefixProbe) {
          part.count = kPrefixProbe;
          const int lowR = opt().no_prefix_low ? 0 : prefix_low_R(table, b, q.len[q.order[b.first]]);
          const size_t before = offenders.size();
          std::vector<std::vector<char>> votes;                        // could the bucket's own height certify the read?  (prefix_bucket: vote)
          PrefixAsk ask;
          if (lowR) { ask.voteR.push_back(b.R); ask.votes = &votes; }
          int rc = prefix_bucket(ctx, ref, q, rg, p, table, part, lowR ? lowR : b.R, lowR != 0, qchunk, qwarm, loc, qdone, offenders, ask);
          if (rc) return rc;
          const std::vector<char> own_ok = lowR ? votes[0] : std::vector<char>();
          for (int k = 0; k < part.count; ++k) tried[q.order[part.first + k]] = 1;
          ntried += (size_t)part.count;
          if (!lowR) {
            if (2 * (offenders.size() - before) > (size_t)part.count) { path_note(ctx, "prefix_probe_failed"); continue; }
          } else if (16 * (offenders.size() - before) <= (size_t)kPrefixProbe) {
            restR = lowR; rest_rowp = true;
            path_note(ctx, "prefix_height[R=%d,low]", restR);
          } else {
            size_t hopeless = 0;
            for (int k = 0; k < part.count; ++k) hopeless += own_ok[q.order[part.first + k]] ? 0 : 1;
            if (2 * hopeless > (size_t)part.count) { path_note(ctx, "prefix_probe_failed"); continue; }
            rest_rowp = true;
            for (size_t o = before; o < offenders.size(); ++o)
              if (own_ok[offenders[o]]) riders.push_back(offenders[o]);
            offenders.erase(std::remove_if(offenders.begin() + before, offenders.end(),
                                           [&](int id) { return std::find(riders.begin(), riders.end(), id) != riders.end(); }), offenders.end());
            path_note(ctx, "prefix_height[R=%d,own,riders=%zu]", restR, riders.size());
          }
          part.first = b.first + kPrefixProbe; part.count = b.count - kPrefixProbe;
        }
        int rc;
        if (riders.empty()) {
          rc = prefix_bucket(ctx, ref, q, rg, p, table, part, restR, rest_rowp, qchunk, qwarm, loc, qdone, offenders);
        } else {
          // the rest of the bucket with the riders in front: a view of the batch with its own sorted id list (ids index everything else)
          QueryBatch qv;
          qv.bytes.alias(q.bytes.p); qv.lens.alias(q.lens.p); qv.offs.alias(q.offs.p); qv.cum.alias(q.cum.p);
          qv.len = q.len; qv.off = q.off; qv.nq = q.nq; qv.maxlen = q.maxlen;
          qv.order.assign(riders.begin(), riders.end());
          for (int k = 0; k < part.count; ++k) qv.order.push_back(q.order[part.first + k]);
          std::stable_sort(qv.order.begin(), qv.order.end(), [&](int32_t a, int32_t b2) { return q.len[a] < q.len[b2]; });
          if (ctx->psel2.ensure(qv.order.size() * 4 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
          HIPCHK(ctx, hipMemcpy(ctx->psel2.p, qv.order.data(), qv.order.size() * 4, hipMemcpyHostToDevice));
          qv.sel.alias(ctx->psel2.p);
          Bucket vb = part;
          vb.first = 0; vb.count = (int)qv.order.size();
          rc = prefix_bucket(ctx, ref, qv, rg, p, table, vb, restR, rest_rowp, qchunk, qwarm, loc, qdone, offenders);
        }
        if (rc) return rc;
        for (int k = 0; k < part.count; ++k) tried[q.order[part.first + k]] = 1;
        ntried += (size_t)part.count;
      }
      if (ntried && (2 * offenders.size() > ntried || (opt().no_requery && !offenders.empty()))) {
        // most reads cannot be certified by their prefix (no hit, or a repeat family over the cap): the sweep decides for everybody
        for (size_t k = 0; k < nq; ++k) if (tried[k]) { loc[k] = Located(); qdone[k] = 0; }
        ctx->prefix_certified = 0; ctx->prefix_second_pass = 0; ctx->prefix_thinned = 0; ctx->prefix_thin_items = 0; ctx->seed_certified = 0; ctx->prefix_named = false; ctx->candidates = candidates_before;
        ctx->last_kernel.cells = 0; ctx->timings[4] = 0; ctx->timings[5] = 0;
        ctx->whole_again += 1;
        path_note(ctx, "whole_again");
      } else if (ntried) {
        std::vector<int> rest;
        std::vector<char> is_off(nq, 0);
        for (int id : offenders) is_off[id] = 1;
        for (size_t k = 0; k < nq; ++k) {
          if (tried[k] && !is_off[k]) { qfast[k] = 1; qfloat[k] = kKeyF16; any_fast = true; }
          else rest.push_back((int)k);
        }
        if (!offenders.empty()) { ctx->requeried += offenders.size(); path_note(ctx, "requery"); }
        if (rest.empty()) all_prefix = true;
        else {
          // a view of the batch that lists only `rest` (same device bytes / offsets / lengths, own sorted id list)
          qrest.bytes.alias(q.bytes.p); qrest.lens.alias(q.lens.p); qrest.offs.alias(q.offs.p); qrest.cum.alias(q.cum.p);
          qrest.len = q.len; qrest.off = q.off;
          qrest.order.assign(rest.begin(), rest.end());
          std::stable_sort(qrest.order.begin(), qrest.order.end(), [&](int32_t a, int32_t b2) { return q.len[a] < q.len[b2]; });
          qrest.nq = rest.size();
          qrest.maxlen = 0;
          for (int id : rest) qrest.maxlen = std::max(qrest.maxlen, (int)q.len[id]);
          if (ctx->psel.ensure(qrest.nq * 4 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
          HIPCHK(ctx, hipMemcpy(ctx->psel.p, qrest.order.data(), qrest.nq * 4, hipMemcpyHostToDevice));
          qrest.sel.alias(ctx->psel.p);
          qs = &qrest;
        }
      }
    }
    if (all_prefix) keys.assign(nq, 0ull);
    const bool prefix_kept = qs != &q || all_prefix;                   // reads settled above stay settled whatever the sweep below does
    for (int attempt = 0; attempt < 4 && !pre && !all_early && !all_prefix; ++attempt) {
      buckets.clear();
      if (n >= 1024) buckets = make_buckets(ref, *qs, table, p, n, allow_sat, allow_sample);
      any_fast = prefix_kept;
      bool any_sat = false;
      bool any_sweep = false;
      for (Bucket &b : buckets) {
        b.fast = bucket_fast_ok(ref, table, b, n, p); any_fast |= b.fast; any_sweep |= b.fast; any_sat |= b.fast && (b.satflag || b.sampled);
        // (not for the uint8 engine's unsaturated sweep: there every cell that reaches 255 must be exact, wherever it lies)
        b.opt_margin = b.longp && !b.unsat && nq == 1 && !opt().no_opt_margin;   // (certified below for a lone query only)
      }
      if (!any_sweep) { if (prefix_kept) keys.assign(nq, 0ull); break; }
      const std::vector<Range> ranges{rg};
      int rc = score_begin(ctx, q, ranges, table);
      if (rc) return rc;
      std::fill(qsat.begin(), qsat.end(), 0);
      for (Bucket &b : buckets) {
        if (!b.fast) continue;
        rc = score_launch(ctx, ref, *qs, ranges, p, table, b);
        if (rc) return rc;
        for (int k = 0; k < b.count; ++k) {
          const int id = qs->order[b.first + k];
          qfast[id] = 1; qchunk[id] = b.sub_len; qwarm[id] = b.warm; qsat[id] = b.sampled ? 2 : (b.satflag ? 1 : 0);
          qfloat[id] = key_kind(b);
        }
      }
      rc = score_fetch(ctx, nq, keys);
      if (rc == kRetryNoWait) {                                       // (an expired wait between workgroups: the non-waiting layout)
        if (!ctx->prefix_named) ctx->last_kernel.cells = 0;        // (cells swept by a prefix filter of this call stay counted)
        ctx->timings[4] = 0; ctx->timings[5] = 0;
        continue;
      }
      if (rc) return rc;
      if (!any_sat) {
        if (ctx->long_cert >= 0.0f && nq == 1) {                       // exact keys: the lone query's maximum as swept
          if (!margin_certified(key_score(kKeyF32Scaled, (uint32_t)(keys[0] >> 32), ctx->fshift))) continue;
        }
        break;
      }
      // the flagged (query, sub-chunk) pairs of the saturating sweep
      unsigned int nflag = 0;
      HIPCHK(ctx, hipMemcpy(&nflag, ctx->flags.p, 4, hipMemcpyDeviceToHost));
      size_t nsatq = 0;
      for (size_t k = 0; k < nq; ++k) nsatq += qsat[k] ? 1 : 0;
      const bool trace_on = opt().trace;
      if (trace_on) std::fprintf(stderr, "[mi355_sw] saturating / sampled sweep: %u candidate sub-chunks of %zu queries (budget %.0f)\n", nflag, nsatq,
                                 64.0 * (double)nsatq + 1024.0);
      auto whole_batch_again = [&]() {
        // saturated nearly everywhere (a background that reaches the cap): the exact sweep instead, for every query
        allow_sat = false;
        allow_sample = false;
        if (!ctx->prefix_named) ctx->last_kernel.cells = 0;         // the sweep that counts is the one that follows
        ctx->timings[4] = 0; ctx->timings[5] = 0;                    // launches / cells: only the sweep that produced the result
                                                                     // (its device time stays in timings[0]: honest extra cost)
        ctx->whole_again += 1;
        path_note(ctx, "whole_again");
      };
      if (nflag > ctx->flag_cap) { whole_batch_again(); continue; }  // (only the unfiltered saturating sweep can overflow the list)
      std::vector<uint32_t> raw(2 * (size_t)nflag);
      if (nflag) HIPCHK(ctx, hipMemcpy(raw.data(), ctx->flags.as<unsigned int>() + 2, (size_t)nflag * 8, hipMemcpyDeviceToHost));
      std::vector<std::pair<uint32_t, uint32_t>> flagged(nflag);
      for (size_t f = 0; f < nflag; ++f) flagged[f] = {raw[2 * f], raw[2 * f + 1]};
      std::sort(flagged.begin(), flagged.end());
      flagged.erase(std::unique(flagged.begin(), flagged.end()), flagged.end());
      ctx->candidates += flagged.size();
      // Per QUERY, not per call: a query with more candidates than its cap (a poly-A or microsatellite read against a repeat-rich
      // reference flags thousands of near-equal sub-chunks) is swept again on the exact instances, alone with the other
      // offenders; everybody else keeps the candidates of the first sweep.  Only when most of the batch offends (a background
      // that reaches the cap everywhere) is the whole batch swept again.
      const uint32_t qcap = query_flag_cap(nq);
      std::vector<uint32_t> qcount(nq, 0);
      for (const auto &f : flagged) if (f.first < nq) qcount[f.first]++;
      std::vector<int> offenders;
      for (size_t k = 0; k < nq; ++k) if (qsat[k] && qcount[k] > qcap) offenders.push_back((int)k);
      if (trace_on) std::fprintf(stderr, "[mi355_sw] %zu of %zu queries exceed %u candidates\n", offenders.size(), nsatq, qcap);
      // uint8 engine, key at the cap of 255: the answer is the 255 that comes first in the skewed storage order, i.e. on the
      // lowest anti-diagonal i + j (the bottom-right triangle i + j > |y| aside: the order wraps it to the front, and its two
      // sub-chunks are always evaluated).  Sub-chunks are longer than |x| + 64, so that cell lies in the first sub-chunk s1 that truly
      // holds a 255 or in s1 + 1; a sub-chunk that is no candidate holds none (its unsaturated maximum stays below 255, and the
      // saturating rule never exceeds the unsaturated one).  sw_sample_first listed the query's first candidates in order:
      // evaluate them exactly; when a 255 turns up and every candidate up to two sub-chunks right of the winner was on the
      // list, the query is settled without a second sweep (a read inside a repeat family: thousands of equal candidates).
      if (!offenders.empty() && ctx->first_valid && p.semantics == MI355_SW_U8SAT) {
        constexpr int K = kFirstCandidates;
        std::vector<uint32_t> first(nq * (size_t)(K + 1));
        HIPCHK(ctx, hipMemcpy(first.data(), ctx->first.p, first.size() * 4, hipMemcpyDeviceToHost));
        std::vector<std::pair<uint32_t, uint32_t>> ff;
        std::vector<int> tried;
        std::vector<float> qlow(nq, 0.0f);
        for (int id : offenders) {
          if (qsat[id] != 2 || qfloat[id] != kKeyF16 || qchunk[id] <= (int64_t)q.len[id] + 64) continue;
          if (half_value((uint16_t)(keys[id] >> 32)) * kF16Scale != 255.0f) continue;
          const uint32_t *f = &first[(size_t)id * (K + 1)];
          const uint32_t cnt = f[0] & 0x7FFFFFFFu;
          if (cnt == 0 || cnt > (uint32_t)K) continue;
          for (uint32_t e = 0; e < cnt; ++e) ff.push_back({(uint32_t)id, f[1 + e]});
          // ... and the last two sub-chunks: the storage order wraps the bottom-right triangle (i + j > |y|) in front of
          // everything else (order_key<1>, region 3), so a 255 there beats any other (locate_fast lists them for the same reason)
          const int64_t nsub = (n + qchunk[id] - 1) / qchunk[id];
          for (int64_t s : {nsub - 2, nsub - 1}) {
            bool listed = s < 0;
            for (uint32_t e = 0; e < cnt; ++e) listed = listed || (int64_t)f[1 + e] == s;
            if (!listed) ff.push_back({(uint32_t)id, (uint32_t)s});
          }
          tried.push_back(id);
          qlow[id] = 255.0f;
        }
        if (!ff.empty()) {
          HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
          rc = locate_saturated(ctx, ref, q, rg, p, qchunk, qwarm, qlow, table, ff, loc, qdone);
          if (rc) return rc;
          HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
          ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
          std::vector<char> settled(nq, 0);
          size_t nsettled = 0;
          for (int id : tried) {
            const uint32_t *f = &first[(size_t)id * (K + 1)];
            const uint32_t cnt = f[0] & 0x7FFFFFFFu;
            bool ok = qdone[id] && loc[id].score == 255.0f;
            // list cut short: every candidate up to two sub-chunks right of the winner must have been on it (f[cnt]: the last one
            // listed) — unless the winner lies in the wrapped triangle, which precedes every cell of the sub-chunks not listed
            if (ok && (f[0] & 0x80000000u) && !(loc[id].ix + loc[id].iy > n && n >= (int64_t)q.len[id]))
              ok = (int64_t)f[cnt] >= (loc[id].iy - 1) / qchunk[id] + 2;
            if (ok) { settled[id] = 1; ++nsettled; }
            else { loc[id] = Located(); qdone[id] = 0; }
          }
          if (nsettled) {
            flagged.erase(std::remove_if(flagged.begin(), flagged.end(), [&](const std::pair<uint32_t, uint32_t> &f) { return f.first < nq && settled[f.first]; }),
                          flagged.end());
            offenders.erase(std::remove_if(offenders.begin(), offenders.end(), [&](int id) { return settled[id] != 0; }), offenders.end());
            ctx->first_settled += nsettled;
            path_note(ctx, "first_settled");
          }
          if (trace_on) std::fprintf(stderr, "[mi355_sw] %zu of %zu offenders settled by their first candidates\n", nsettled, tried.size());
        }
      }
      if (!offenders.empty() && (opt().no_requery || 2 * offenders.size() > nsatq)) { whole_batch_again(); continue; }
      if (!offenders.empty()) {
        flagged.erase(std::remove_if(flagged.begin(), flagged.end(), [&](const std::pair<uint32_t, uint32_t> &f) { return qcount[f.first] > qcap; }),
                      flagged.end());
        // a view of the batch that lists only the offenders (same device bytes / offsets / lengths, own sorted id list)
        QueryBatch qo;
        qo.bytes.alias(q.bytes.p); qo.lens.alias(q.lens.p); qo.offs.alias(q.offs.p); qo.cum.alias(q.cum.p);
        qo.len = q.len; qo.off = q.off;
        qo.order.assign(offenders.begin(), offenders.end());
        std::stable_sort(qo.order.begin(), qo.order.end(), [&](int32_t a, int32_t b2) { return q.len[a] < q.len[b2]; });
        qo.nq = offenders.size();
        qo.maxlen = 0;
        for (int id : offenders) qo.maxlen = std::max(qo.maxlen, (int)q.len[id]);
        if (ctx->sel2.ensure(qo.nq * 4 + 16)) return fail(ctx, MI355_SW_ENOMEM, "hipMalloc(score scratch) failed");
        HIPCHK(ctx, hipMemcpy(ctx->sel2.p, qo.order.data(), qo.nq * 4, hipMemcpyHostToDevice));
        qo.sel.alias(ctx->sel2.p);
        std::vector<Bucket> again = make_buckets(ref, qo, table, p, n, false, false);
        rc = score_begin(ctx, q, ranges, table);                     // (clears every key: the first sweep's are on the host)
        if (rc) return rc;
        for (Bucket &b : again) {
          b.fast = bucket_fast_ok(ref, table, b, n, p);
          if (!b.fast) return fail(ctx, MI355_SW_ENODEV, "internal: an exact instance refuses a query the sampled one took");
          rc = score_launch(ctx, ref, qo, ranges, p, table, b);
          if (rc) return rc;
          for (int k = 0; k < b.count; ++k) {
            const int id = qo.order[b.first + k];
            qchunk[id] = b.sub_len; qwarm[id] = b.warm; qsat[id] = 0;
            qfloat[id] = key_kind(b);
          }
        }
        std::vector<unsigned long long> keys2;
        rc = score_fetch(ctx, nq, keys2);
        if (rc == kRetryNoWait) return fail(ctx, MI355_SW_ENODEV, "sw_long_kernel: a pipeline wait expired");   // (offenders never take sw_long_kernel)
        if (rc) return rc;
        for (int id : offenders) keys[id] = keys2[id];
        ctx->requeried += offenders.size();
        path_note(ctx, "requery");
      }
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      std::vector<float> qlower(nq, 0.0f);                          // the sweep's key: a lower bound of the query's maximum
      for (size_t k = 0; k < nq; ++k) {
        if (!qsat[k]) continue;
        qlower[k] = key_score(qfloat[k], (uint32_t)(keys[k] >> 32), ctx->fshift);   // (sampled and saturating sweeps: kKeyF16 or kKeyF32Scaled)
      }
      rc = locate_flagged(ctx, ref, q, rg, p, qchunk, qwarm, qlower, table, flagged, loc, qdone);
      if (rc) return rc;
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
      // every query whose key sits at the cap must have been resolved by a flagged sub-chunk
      for (size_t k = 0; k < nq; ++k)
        if (qsat[k] && !qdone[k] && (qsat[k] == 2 ? (keys[k] >> 32) != 0 : half_value((uint16_t)(keys[k] >> 32)) * kF16Scale >= kF16Scale))
          return fail(ctx, MI355_SW_ENODEV, "internal: a saturated or sampled query without a flagged sub-chunk");
      if (ctx->long_cert >= 0.0f && nq == 1 && !margin_certified(qdone[0] ? loc[0].score : 0.0f)) {
        loc[0] = Located(); qdone[0] = 0;
        continue;
      }
      break;
    }
    if (any_fast) {
      int rc = 0;
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      rc = locate_fast(ctx, ref, q, rg, p, qfast, qchunk, qwarm, qfloat, keys.data(), table, loc, &qdone);
      if (rc) return rc;
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
      if (want_trace) {
        std::vector<int> fq;
        std::vector<Located> floc;
        for (size_t k = 0; k < nq; ++k) if (qfast[k]) { fq.push_back((int)k); floc.push_back(loc[k]); }
        std::vector<TraceOut> ft;
        HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
        rc = trace_located(ctx, ref, q, rg, p, qwarm, table, fq, floc, ft);
        if (rc) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->timings[2] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
        for (size_t t = 0; t < fq.size(); ++t) tout[fq[t]] = std::move(ft[t]);
      }
    }
    // Many small whole problems (short reference or short queries: nothing took the score kernel): float engine with
    // identity scoring runs them on device-built job lists, one sorted range per orientation (host_batch.h)
    std::vector<char> &handled = ctx->handled_store;               // (2: written straight into the caller's view, host_batch.h)
    handled.assign(nq, 0);
    bool all_handled = false;
    size_t z_handled = 0;
    if (!any_fast && p.semantics == MI355_SW_F32 && wave_scoring_ok(p) && !opt().no_wave &&
        !opt().no_devlist) {
      auto len_at = [&](size_t pos) { return (int64_t)q.len[q.order[pos]]; };
      auto first_above = [&](int64_t v) {                          // first sorted position whose length exceeds v
        size_t lo = 0, hi = nq;
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (len_at(mid) <= v) lo = mid + 1; else hi = mid; }
        return lo;
      };
      const size_t z = first_above(0);                             // empty queries: score 0, nothing to run
      // lanes = rows of x (|x| <= 512, |x| <= |y|) — unless the range fits the lanes and the profile kernel takes it: then
      // every x streams past the shared profile (|x| + 16 steps instead of |y| + 16, on the cheaper cell)
      const bool all_stream = n <= kWaveMaxLanesSide && wave_prof_ok(ref, p, wave_R((int)n), (int)n, true);
      const size_t e0 = all_stream ? z : first_above(std::min<int64_t>(kWaveMaxLanesSide, n));
      const size_t e1 = n <= kWaveMaxLanesSide ? nq : e0;          // lanes = columns of y (|y| <= 512), x streams
      for (size_t pos = 0; pos < z; ++pos) handled[q.order[pos]] = 1;
      all_handled = true; z_handled = z;
      ctx->devlist_done = 0;
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      int rc = exact_full_device(ctx, ref, q, rg, p, z, e0 - z, 0, want_trace, loc, tout, handled);
      if (!rc) rc = exact_full_device(ctx, ref, q, rg, p, e0, e1 - e0, 1, want_trace, loc, tout, handled);
      if (rc) return rc;
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[2] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
    }
    if (ctx->while_device_works) { ctx->while_device_works(); ctx->while_device_works = nullptr; }   // (no launch took it)
    std::vector<int> slow;
    all_handled = all_handled && z_handled + ctx->devlist_done == nq;   // (half a million alignments: no scan when the lists took them all)
    if (!all_handled)
      for (size_t k = 0; k < nq; ++k) if (!qfast[k] && !handled[k]) slow.push_back((int)k);
    // Problems the score kernel does not take (no finite warm-up margin: a gap penalty that is, or truncates to, 0 ...) and whose
    // anti-diagonal does not fit the LDS kernel either: the strip kernel over the WHOLE range as one window — a window that starts
    // at column 0 needs no margin — for the first maximum (locate_saturated with one sub-chunk = the range) and for the decisions
    // (wave_trace starts its windows at 0 when no margin is finite).  Identity scoring; not the uint8 engine's |x| == |y| quirk.
    if (!slow.empty() && !pre && wave_scoring_ok(p) && strip_scoring_ok(ref, p) && n > kWaveMaxLanesSide) {
      std::vector<int> huge, rest;
      for (int id : slow) {
        const int64_t m = q.len[id];
        const bool quirk = p.semantics == MI355_SW_U8SAT && m == n;
        if (m > kWaveMaxLanesSide && !quirk && exact_lds_bytes((int)m, (int)std::min<int64_t>(n, INT32_MAX)) > kExactLdsMax) huge.push_back(id);
        else rest.push_back(id);
      }
      if (!huge.empty()) {
        std::vector<int64_t> hchunk(nq, n), hwarm(nq, kColsMax);
        std::vector<float> hlow(nq, 0.0f);
        std::vector<char> hdone(nq, 0);
        std::vector<std::pair<uint32_t, uint32_t>> whole;
        for (int id : huge) whole.push_back({(uint32_t)id, 0u});
        HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
        int rc = locate_saturated(ctx, ref, q, rg, p, hchunk, hwarm, hlow, table, whole, loc, hdone);
        if (rc) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
        if (want_trace) {
          std::vector<Located> hl;
          for (int id : huge) hl.push_back(loc[id]);
          std::vector<TraceOut> ht;
          HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
          rc = trace_located(ctx, ref, q, rg, p, hwarm, table, huge, hl, ht);
          if (rc) return rc;
          HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
          ctx->timings[2] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
          for (size_t t = 0; t < huge.size(); ++t) tout[huge[t]] = std::move(ht[t]);
        }
        slow.swap(rest);
      }
    }
    if (!slow.empty()) {
      std::vector<Located> sl;
      std::vector<TraceOut> st;
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      int rc = exact_full(ctx, ref, q, rg, p, slow, want_trace, sl, st);
      if (rc) {
        if (!table.ok && ctx->err.find("outside its coverage") != std::string::npos) ctx->err += " (" + table.why + ")";
        return rc;
      }
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[2] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
      for (size_t t = 0; t < slow.size(); ++t) { loc[slow[t]] = sl[t]; if (want_trace) tout[slow[t]] = std::move(st[t]); }
    }
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
  ctx->timings[3] += elapsed_us(ctx, ctx->ev[4], ctx->ev[5]);
  return 0;
}

// ... as an array of results with library-owned (malloc) strings: the C-ABI's classic form
int align_range(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
                const mi355_sw_params &p, int flags, mi355_sw_result *outs, const ScoredRanges *pre = nullptr, size_t pre_range = 0) {
  const bool want_trace = !(flags & MI355_SW_SCORE_ONLY);
  const size_t nq = q.nq;
  std::vector<Located> &loc = ctx->loc_store;
  std::vector<TraceOut> &tout = ctx->tout_store;
  int rc = align_range_core(ctx, ref, q, rg, p, flags, loc, tout, pre, pre_range);
  if (rc) return rc;
  HostTrace trace_results("set_results");
  const float t_iter = (float)(ctx->timings[0] > 0 ? ctx->timings[0] : ctx->timings[3]);
  parallel_for(nq, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; ++k) {
      set_result(outs[k], loc[k].score, loc[k].ix, loc[k].iy, (want_trace && loc[k].score > 0) ? &tout[k] : nullptr);
      outs[k].timings_us[0] = t_iter;
      outs[k].timings_us[1] = 0;
    }
  });
  return 0;
}

// ... as a struct of arrays in context-owned memory, strings as views into the D2H buffers: nothing per alignment is
// allocated (half a million small alignments per call)
int align_range_view(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const Range &rg,
                     const mi355_sw_params &p, int flags, mi355_sw_batch_view *out) {
  const bool want_trace = !(flags & MI355_SW_SCORE_ONLY);
  const size_t nq = q.nq;
  std::vector<Located> &loc = ctx->loc_store;
  std::vector<TraceOut> &tout = ctx->tout_store;
  PoolFromScope pool_from_;
  ViewStore &v = ctx->view;
  v.score.resize(nq); v.pos.resize(nq); v.cons_len.resize(nq); v.end_x.resize(nq); v.end_y.resize(nq);
  v.cx.resize(nq); v.cy.resize(nq);
  // the many-small-alignments batch writes the alignments its device list finishes straight into the view when it has them in
  // id order (exact_full_device, handled = 2): one pass over half a million results instead of two
  ctx->handled_store.clear();
  ctx->devlist_direct = 0;
  ctx->direct_view = &v;
  int rc = align_range_core(ctx, ref, q, rg, p, flags, loc, tout);
  ctx->direct_view = nullptr;
  if (rc) return rc;
  HostTrace trace_results("view_results");
  const std::vector<char> &direct = ctx->handled_store;
  const bool some_direct = direct.size() == nq && ctx->devlist_direct > 0;
  if (!(some_direct && ctx->devlist_direct == nq))
  parallel_for(nq, [&](size_t k0, size_t k1) {
    for (size_t k = k0; k < k1; ++k) {
      if (some_direct && direct[k] == 2) continue;
      const bool hit = loc[k].score > 0;
      const TraceOut *t = (want_trace && hit) ? &tout[k] : nullptr;
      v.score[k] = loc[k].score;
      v.end_x[k] = hit ? loc[k].ix : 0;
      v.end_y[k] = hit ? loc[k].iy : 0;
      v.pos[k] = t ? t->pos : 0;
      v.cons_len[k] = t ? (uint32_t)t->len : 0;
      v.cx[k] = t && t->len ? t->cx : nullptr;
      v.cy[k] = t && t->len ? t->cy : nullptr;
    }
  });
  out->n = nq;
  out->score = v.score.data(); out->pos = v.pos.data(); out->end_x = v.end_x.data(); out->end_y = v.end_y.data();
  out->cons_x = v.cx.data(); out->cons_y = v.cy.data(); out->cons_len = v.cons_len.data();
  out->timings_us[0] = (float)(ctx->timings[0] > 0 ? ctx->timings[0] : ctx->timings[3]);
  out->timings_us[1] = 0;
  return 0;
}

// Per-range maxima of every query (value half of find_index_of_maximum per piece).
// winner_only (mi355_sw_best_range; DESIGN.md §3.3 lemmas L10, L11): the caller only needs, per query, the first range with the greatest maximum — what
// OMPParallelLocalAligner does with the per-piece maxima (plocalaligner.cpp:122-129).  A lone long query is then swept with the
// sampled maximum (every 4th step: keys are lower bounds within three gaps), and only the ranges whose key lies within that
// slack of the best key — the only ones that can hold the greatest maximum — have their candidate sub-chunks re-evaluated
// exactly; the maxima of the other ranges stay lower bounds.
// known_best / exact_above (winner_only): the sweep of a lone long query uses an optimistic warm-up margin (long_score_launch)
// and is exact for maxima above *exact_above.  known_best > 0: a lower bound of the greatest maximum the caller already knows
// (from other ranks, or from a first call) — the margin is then the one THAT value needs, so that every range whose maximum
// reaches it comes out exact.  exact_above == nullptr: this function certifies its own best by sweeping again when needed.
int range_maxima(mi355_sw_ctx *ctx, const RefData &ref, const QueryBatch &q, const std::vector<Range> &ranges,
                 const mi355_sw_params &p, float *maxima /* [nranges][nq] */, bool winner_only = false, float known_best = 0.0f,
                 float *exact_above = nullptr) {
  const size_t nq = q.nq, nr = ranges.size();
  ctx->scored.valid = false;
  if (exact_above) *exact_above = -1.0f;
  if (nq == 0 || nr == 0) return 0;
  const ScoreTable table = plan_table(ref, p);
  // no positive score possible (see align_range): every maximum is 0
  if ((p.semantics == MI355_SW_U8SAT && u8_params(p).M == 0) ||
      (p.semantics == MI355_SW_F32 && table.ok && !(table.smaxf > 0))) {
    for (size_t k = 0; k < nr * nq; ++k) maxima[k] = 0.0f;
    return 0;
  }
  int64_t maxn = 0;
  for (auto &r : ranges) maxn = std::max(maxn, r.hi - r.lo);
  const bool try_sample = winner_only && nq == 1 && nr <= 4096 && strip_scoring_ok(ref, p) && !opt().no_sample;
  std::vector<Bucket> buckets = make_buckets(ref, q, table, p, maxn, false, try_sample);
  std::vector<char> qfast(nq, 0), qfloat(nq, 0);
  bool sampled = false;
  for (Bucket &b : buckets) {
    b.fast = true;
    for (auto &r : ranges) b.fast = b.fast && bucket_fast_ok(ref, table, b, r.hi - r.lo, p);
    if (!b.longp) b.sampled = false;                               // only sw_long_kernel lays out one value row per range
    sampled |= b.fast && b.sampled;
    b.opt_margin = winner_only && b.longp && !b.unsat && nq == 1 && !opt().no_opt_margin;
    // test hook (option prefix_tiles, one range): a bucket of the prefix shape is swept by its PREFIX instance — the maxima are then
    // the sampled keys of the reads' first P rows (lower bounds within sample_slack, tests/test_gpu_prefix_tiles.py)
    if (opt().prefix_tiles && nr == 1 && !winner_only && b.fast && b.sem == kSemF16 && b.mirror && !b.strips && !b.twin && !b.satflag && !b.unsat &&
        b.SL == 8 && b.count >= 2 && kernel_sem(b) == kSemF16M && listed(kR8M, b.R)) {
      b.SL = kPrefixLanes; b.prefix = true; b.sampled = true;
    }
    // ... (option prefix_rowp = R, a listed R whose prefix is shorter than the bucket's reads) by the instance of R rows per lane that
    // folds row P = 2 R alone; the value rows stay readable (mi355_sw_prefix_values, tests/test_gpu_prefix_rowp_tiles.py)
    // (option prefix_rowp_step = R: the instance that folds row P at every step, tests/test_gpu_prefix_step_tiles.py)
    // (the step tiles also at the low heights of kR2Step, R = 8 and 10: tests/test_gpu_prefix_low_tiles.py)
    const bool hook_step = prefix_step_listed(opt().prefix_rowp_step);
    const long hook_R = hook_step ? opt().prefix_rowp_step : opt().prefix_rowp;
    if ((hook_step || listed(kR8M, hook_R)) && nr == 1 && !winner_only && b.fast && b.sem == kSemF16 && b.mirror && !b.strips && !b.twin && !b.satflag &&
        !b.unsat && b.SL == 8 && b.count >= 2 && kernel_sem(b) == kSemF16M && kPrefixLanes * hook_R < q.len[q.order[b.first]] && ctx->hook_ids.empty()) {
      b.SL = kPrefixLanes; b.R = (int)hook_R; b.prefix = true; b.sampled = true; b.rowp = true; b.step = hook_step;
      for (int k = 0; k < b.count; ++k) ctx->hook_ids.push_back(q.order[b.first + k]);
    }
  }
  ctx->long_margin = 0;
  if (winner_only && nq == 1 && known_best > 0.0f && table.integral)
    ctx->long_margin = (int64_t)((double)q.maxlen + std::ceil(((double)table.smax * (double)q.maxlen - (double)known_best) / (double)table.gap)) + 2 + 64;
  // what a following mi355_sw_align_scored_range needs (one launch group only: the geometry is per launch)
  ScoredRanges &sc = ctx->scored;
  sc.valid = false;
  const bool keep = nr <= 32768 && p.lut == nullptr;
  if (keep) {
    sc.ref = &ref; sc.batch = &q; sc.ref_version = ref.version; sc.batch_version = q.version; sc.params = p; sc.ranges = ranges;
    sc.keys.assign(nr * nq, 0ull); sc.qfast.assign(nq, 0); sc.qfloat.assign(nq, 0); sc.qchunk.assign(nq, 0); sc.qwarm.assign(nq, 0);
    sc.sampled = false; sc.has_located.assign(nr, 0); sc.located.assign(nr, Located());
  }
  for (size_t lo = 0; lo < nr; lo += 32768) {
    const size_t hi = std::min(nr, lo + 32768);
    const std::vector<Range> sub(ranges.begin() + lo, ranges.begin() + hi);
    bool any = false;
    for (Bucket &b : buckets) any |= b.fast;
    if (!any) break;
    int rc = score_begin(ctx, q, sub, table);
    if (rc) return rc;
    for (Bucket &b : buckets) {
      if (!b.fast) continue;
      rc = score_launch(ctx, ref, q, sub, p, table, b);
      if (rc) return rc;
      for (int k = 0; k < b.count; ++k) {
        const int id = q.order[b.first + k];
        qfast[id] = 1; qfloat[id] = key_kind(b);
        if (keep) { sc.qchunk[id] = b.sub_len; sc.qwarm[id] = b.warm; }
      }
    }
    std::vector<unsigned long long> keys;
    rc = score_fetch(ctx, nq * sub.size(), keys);
    if (rc == kRetryNoWait) {                                       // (an expired wait between workgroups: the non-waiting layout)
      ctx->timings[4] = 0; ctx->timings[5] = 0; ctx->last_kernel.cells = 0;
      return range_maxima(ctx, ref, q, ranges, p, maxima, winner_only, known_best, exact_above);
    }
    if (rc) return rc;
    if (keep) { std::copy(keys.begin(), keys.end(), sc.keys.begin()); sc.qfast = qfast; sc.qfloat = qfloat; sc.fshift = ctx->fshift; }
    for (size_t r = 0; r < sub.size(); ++r)
      for (size_t k = 0; k < nq; ++k)
        if (qfast[k]) maxima[(lo + r) * nq + k] = key_score(qfloat[k], (uint32_t)(keys[r * nq + k] >> 32), ctx->fshift);
    if (sampled) {
      // (nq == 1, one launch group.)  The keys above are lower bounds within 3 gaps: re-evaluate the contenders exactly.
      unsigned int nflag = 0;
      HIPCHK(ctx, hipMemcpy(&nflag, ctx->flags.p, 4, hipMemcpyDeviceToHost));
      const uint32_t qcap = query_flag_cap(nq);
      float top = 0.0f;
      for (size_t r = 0; r < nr; ++r) top = std::max(top, maxima[r]);
      const float slack = (float)(kLongMK - 1) * table.gapf;
      bool ok = nflag <= ctx->flag_cap && nflag <= qcap;            // (the filter stops appending beyond the cap)
      std::vector<std::vector<std::pair<uint32_t, uint32_t>>> per_range(nr);
      if (ok && nflag) {
        std::vector<uint32_t> raw(2 * (size_t)nflag);
        HIPCHK(ctx, hipMemcpy(raw.data(), ctx->flags.as<unsigned int>() + 2, (size_t)nflag * 8, hipMemcpyDeviceToHost));
        for (size_t f = 0; f < nflag; ++f) {
          const size_t r = (size_t)(raw[2 * f + 1] / (uint64_t)ctx->long_nsub);
          if (r < nr) per_range[r].push_back({raw[2 * f], (uint32_t)(raw[2 * f + 1] % (uint64_t)ctx->long_nsub)});
        }
      }
      HIPCHK(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
      for (size_t r = 0; r < nr && ok; ++r) {
        if (!(maxima[r] > 0.0f) || maxima[r] < top - slack) continue;                     // cannot hold the greatest maximum
        auto &fl = per_range[r];
        std::sort(fl.begin(), fl.end());
        fl.erase(std::unique(fl.begin(), fl.end()), fl.end());
        std::vector<Located> loc(1);
        std::vector<char> done(1, 0);
        const std::vector<float> qlower(1, maxima[r]);
        std::vector<int64_t> qchunk(1, 0), qwarm(1, 0);
        for (Bucket &b : buckets) if (b.fast) { qchunk[0] = b.sub_len; qwarm[0] = b.warm; }
        rc = locate_flagged(ctx, ref, q, ranges[r], p, qchunk, qwarm, qlower, table, fl, loc, done);
        if (rc) return rc;
        if (!done[0]) { ok = false; break; }
        maxima[r] = loc[0].score;
        if (keep) { sc.has_located[r] = 1; sc.located[r] = loc[0]; }
        ctx->candidates += fl.size();
      }
      HIPCHK(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      ctx->timings[1] += elapsed_us(ctx, ctx->ev[2], ctx->ev[3]);
      if (!ok) {                                                     // too many near-equal candidates: the exact sweep instead
        ctx->whole_again += 1;
        ctx->timings[4] = 0; ctx->timings[5] = 0; ctx->last_kernel.cells = 0;
        return range_maxima(ctx, ref, q, ranges, p, maxima, false);
      }
      if (keep) sc.sampled = true;
    }
    if (winner_only && nq == 1 && ctx->long_cert >= 0.0f) {
      // optimistic margin: exact above long_cert.  The caller merges several ranks' results and checks the GLOBAL best
      // against it (exact_above); without a caller's check, this call certifies its own best
      float top = 0.0f;
      for (size_t r = 0; r < nr; ++r) top = std::max(top, maxima[r]);
      if (exact_above) *exact_above = ctx->long_cert;
      else if (!(top > ctx->long_cert)) {
        ctx->whole_again += 1;
        ctx->timings[4] = 0; ctx->timings[5] = 0; ctx->last_kernel.cells = 0;
        // the margin `top` needs; a second call is exact for every maximum >= top, hence for the true best
        return range_maxima(ctx, ref, q, ranges, p, maxima, true, std::max(top, 1.0f), nullptr);
      }
    }
  }
  std::vector<int> slow;
  for (size_t k = 0; k < nq; ++k) if (!qfast[k]) slow.push_back((int)k);
  for (size_t r = 0; r < nr && !slow.empty(); ++r) {
    std::vector<Located> loc;
    std::vector<TraceOut> t;
    int rc = exact_full(ctx, ref, q, ranges[r], p, slow, false, loc, t);
    if (rc) return rc;
    for (size_t i = 0; i < slow.size(); ++i) maxima[r * nq + slow[i]] = loc[i].score;
  }
  sc.valid = keep;
  return 0;
}

int check_params(mi355_sw_ctx *ctx, const mi355_sw_params *p) {
  if (!ctx) return MI355_SW_EINVAL;
  if (!p) return fail(ctx, MI355_SW_EINVAL, "params is NULL");
  if (p->semantics != MI355_SW_F32 && p->semantics != MI355_SW_U8SAT) return fail(ctx, MI355_SW_EINVAL, "unknown semantics");
  return 0;
}

void reset_timings(mi355_sw_ctx *ctx) {
  for (double &t : ctx->timings) t = 0;
  ctx->score_ev_used = 0; ctx->arenas.clear(); ctx->cons_used = 0;
  ctx->last_kernel = mi355_sw_kernel_info{};
  ctx->requeried = 0; ctx->whole_again = 0; ctx->candidates = 0; ctx->prefix_certified = 0; ctx->prefix_second_pass = 0; ctx->prefix_thinned = 0; ctx->prefix_thin_items = 0; ctx->prefix_seeded = 0; ctx->prefix_seed_hits = 0; ctx->seed_certified = 0; ctx->prefix_calibrated = 0; ctx->prefix_fill_moved = 0; ctx->prefix_fill_resident = 0; ctx->prefix_named = false; ctx->left_window = 0; ctx->beyond_f16 = 0; ctx->first_settled = 0;
  ctx->hook_ids.clear(); ctx->hook_nsub = 0;
  ctx->saved_locates = 0; ctx->saved_traces = 0; ctx->saved_fallbacks = 0; ctx->walk_widened = 0; ctx->wait_retries = 0; ctx->early_settled = 0;
  ctx->zdrop_stopped = 0; ctx->zdrop_rows_run = 0;
  ctx->exact_launches = 0; ctx->trace_launches = 0;
  ctx->path.clear();
}

// The single-alignment chain (host_solo.h) declined: the call starts over on the general path.  What the declined attempt
// launched did run, so its tags stay in the call's path (mi355_sw_last_path: "solo[...]" beside the general path's tags).
void reset_after_decline(mi355_sw_ctx *ctx) {
  const std::string ran = ctx->path;
  reset_timings(ctx);
  ctx->path = ran;
}

}  // namespace
