/*
 * mi355_sw.h — C-ABI of the MI355X (gfx950) Smith-Waterman engine.
 *
 * This is the drop-in boundary for the reference's hot path (kosta777/parallel-genomeseq):
 * the entry points are what a binding of `SWAligner<SMT>::calculateScore()` and
 * `OMPParallelLocalAligner<SMT,LAT>::calculateScore()` needs, with plain pointers and sizes.
 * Reference interfaces replaced (paths relative to the reference root):
 *
 *   mi355_sw_align        SWAligner<SMT>::calculateScore + getScore/getPos/getConsensus_x/_y
 *                         (src/aligner/smithwaterman.h:11-58, smithwaterman.cpp:80-108)
 *   mi355_sw_align_batch  the loop of independent alignments in src/sw_solve_small.cpp:82-93,
 *                         src/sw_solve_big.cpp:78-92, src/mpi_sw_solve_uniprot.cpp:95-138
 *   mi355_sw_align_split  OMPParallelLocalAligner<SMT,LAT>::calculateScore
 *                         (src/aligner/plocalaligner.h:6-33, plocalaligner.cpp:105-143)
 *   mi355_sw_make_string_range   _make_string_range (plocalaligner.cpp:44-67)
 *   mi355_sw_fill_matrix  Abstract_Similarity_Matrix::iterate + operator()(row,col)
 *                         (src/aligner/similaritymatrix.h:13-24,45,76-79)
 *   mi355_sw_argmax       Abstract_Similarity_Matrix::find_index_of_maximum
 *                         (similaritymatrix.cpp:21-28, :291-299)
 *
 * Semantics: MI355_SW_F32 follows Similarity_Matrix (float cells, linear gap), MI355_SW_U8SAT
 * follows Similarity_Matrix_Skewed (uint8 saturating cells; only f('A','A'), f('A','T') and the
 * gap are used, similaritymatrix.cpp:389-392).  Argmax tie-breaks, the greedy traceback and the
 * reversed consensus strings are those of the reference.
 *
 * Deliberate divergence: an all-zero matrix (no positive cell) is undefined behaviour in the
 * reference (smithwaterman.cpp:46-48); here it yields score 0, pos 0, empty consensus.
 *
 * Ownership: inputs are caller-owned and only read during the call.  Output strings are
 * library-owned (malloc) and released with mi355_sw_free_result(s).  One context per host
 * thread / per GPU; a context is not thread-safe.  All functions return 0 on success or a
 * negative MI355_SW_E* code; mi355_sw_last_error() gives the message.  There is NO CPU
 * fallback: without a usable HIP device every compute entry point fails with MI355_SW_ENODEV.
 */
#ifndef MI355_SW_H_
#define MI355_SW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MI355_SW_F32 = 0, MI355_SW_U8SAT = 1 };

enum {
  MI355_SW_OK = 0,
  MI355_SW_EINVAL = -22,   /* bad argument */
  MI355_SW_ENOMEM = -12,   /* host or device allocation failed */
  MI355_SW_ENODEV = -19,   /* no usable HIP device / HIP call failed */
  MI355_SW_ENOTSUP = -95,  /* input outside what this build's kernels cover (message says what) */
  MI355_SW_ERANGE = -34    /* the reference's own asserts would fire (plocalaligner.cpp:52,63,65) */
};

/* flags for mi355_sw_align_batch / mi355_sw_batch_run */
enum {
  MI355_SW_SCORE_ONLY = 1  /* score + argmax cell only: pos = 0, empty consensus */
};

typedef struct mi355_sw_ctx mi355_sw_ctx;

typedef struct {
  const float *lut;  /* 256x256 table, lut[(uint8)a*256 + (uint8)b] = f(a,b) with a from x, b from y;
                        NULL => f(a,b) = (a == b ? match : mismatch)  (smithwaterman.cpp:8) */
  float match;       /* reference default  3 */
  float mismatch;    /* reference default -3 */
  float gap;         /* gap_penalty, reference default 2 */
  int semantics;     /* MI355_SW_F32 | MI355_SW_U8SAT */
} mi355_sw_params;

typedef struct {
  float score;          /* getScore(): maximum cell value */
  uint32_t pos;         /* getPos(): 1-based column of y where the traceback stopped */
  int64_t end_x;        /* argmax row    (1-based index into x), 0 when score == 0 */
  int64_t end_y;        /* argmax column (1-based index into y), 0 when score == 0 */
  char *cons_x;         /* getConsensus_x(): reversed, '-' for gaps, NUL terminated */
  char *cons_y;         /* getConsensus_y(); lives in the same allocation as cons_x: release both with
                           mi355_sw_free_result, never with free() */
  size_t cons_len;
  float timings_us[2];  /* getTimings(): [0] DP-fill device time of the call that produced this
                           result (shared by all results of one batch), [1] sum over pieces */
} mi355_sw_result;

int mi355_sw_create(mi355_sw_ctx **ctx, int device);
void mi355_sw_destroy(mi355_sw_ctx *ctx);
const char *mi355_sw_last_error(const mi355_sw_ctx *ctx);
void mi355_sw_default_params(mi355_sw_params *p); /* 3 / -3 / 2, F32, no table */

/* A/B and diagnostic switches of one context (DESIGN.md §8.1 lists them; NONE changes a result — each selects another
 * kernel instance or pipeline for the same answer, which is what the parity tests use them for).  Defaults come from the
 * environment, MI355_SW_<NAME IN CAPITALS>, read once by mi355_sw_create.  key: e.g. "no_f16" (or "MI355_SW_NO_F16");
 * value: NULL, "", "0", "off", "false" = off, anything else = on (integer options: the number).
 * mi355_sw_option_names(): comma-separated list of the keys this build knows.  MI355_SW_EINVAL for an unknown key. */
int mi355_sw_set_option(mi355_sw_ctx *ctx, const char *key, const char *value);
const char *mi355_sw_option_names(void);

/* One alignment of x (rows) against y (columns).  The last y of such calls stays resident on the device and is
 * used again when a later call passes the same bytes: same length and same 128-bit content hash (two independent
 * 64-bit hashes; re-hashed on every call, on helper threads, while the call already runs on the resident copy; a
 * changed buffer costs one extra upload).  MI355_SW_NO_REF_CACHE=1 in the environment switches the reuse off (every
 * call uploads y).  A context serves one host thread at a time; use one context per thread. */
int mi355_sw_align(mi355_sw_ctx *ctx, const char *x, size_t nx, const char *y, size_t ny,
                   const mi355_sw_params *params, mi355_sw_result *out);

/* Make y resident in HBM for subsequent batch calls (copied; caller may free y). */
int mi355_sw_set_reference(mi355_sw_ctx *ctx, const char *y, size_t ny);

/* n independent alignments of xs[k] (length nxs[k]) against the resident reference. */
int mi355_sw_align_batch(mi355_sw_ctx *ctx, size_t n, const char *const *xs, const size_t *nxs,
                         const mi355_sw_params *params, int flags, mi355_sw_result *outs);

/* Same, with the queries made resident first so that a timed region can start with all inputs
 * in HBM (bench.py).  mi355_sw_batch_run may be called repeatedly. */
int mi355_sw_batch_upload(mi355_sw_ctx *ctx, size_t n, const char *const *xs, const size_t *nxs);
int mi355_sw_batch_run(mi355_sw_ctx *ctx, const mi355_sw_params *params, int flags,
                       mi355_sw_result *outs);
/* mi355_sw_batch_upload for a batch that already lies in ONE buffer: sequence k = buf[offsets[k], offsets[k + 1]), n + 1
 * ascending offsets — what a multi-FASTA reader has (the reference concatenates the lines of each of its 561 356 files into
 * one string, src/mpi_sw_solve_uniprot.cpp:97-110).  No pointer per sequence and no staging copy: the caller's bytes go to
 * the device as they are while the index is built. */
int mi355_sw_batch_upload_packed(mi355_sw_ctx *ctx, size_t n, const char *buf, const int64_t *offsets);

/* mi355_sw_batch_run with the results as a struct of arrays in LIBRARY-OWNED memory (valid until the next call on this
 * context; nothing to free): for batches of very many small alignments (the 561 356 sequences of
 * src/mpi_sw_solve_uniprot.cpp's run), where one malloc'ed string pair per alignment costs more than the alignments.
 * cons_x[k] / cons_y[k]: cons_len[k] bytes each, NOT NUL-terminated, NULL when cons_len[k] == 0. */
typedef struct {
  size_t n;
  const float *score;
  const uint32_t *pos;
  const int64_t *end_x;
  const int64_t *end_y;
  const char *const *cons_x;
  const char *const *cons_y;
  const uint32_t *cons_len;
  float timings_us[2];
} mi355_sw_batch_view;
int mi355_sw_batch_run_view(mi355_sw_ctx *ctx, const mi355_sw_params *params, int flags, mi355_sw_batch_view *out);

/* OMPParallelLocalAligner: split y into npiece overlapping pieces, pick the first piece with the
 * strictly greatest maximum under (params, sm_semantics), re-align it under la_semantics with
 * DEFAULT scoring (plocalaligner.cpp:135), pos += left.  winning_piece may be NULL. */
int mi355_sw_align_split(mi355_sw_ctx *ctx, const char *x, size_t nx, const char *y, size_t ny,
                         const mi355_sw_params *params, int sm_semantics, int la_semantics,
                         int npiece, float overlap_ratio, mi355_sw_result *out, int *winning_piece);

/* Maximum cell value of every resident query over each sub-range [lefts[k], rights[k]) of the resident
 * reference, each range an independent problem with a zero left border (what
 * OMPParallelLocalAligner's per-piece iterate + find_index_of_maximum produce, plocalaligner.cpp:110-129).
 * maxima[k * n_queries + q].  Used by multi-GPU reference sharding: every rank sweeps its own pieces. */
int mi355_sw_score_ranges(mi355_sw_ctx *ctx, size_t nranges, const int64_t *lefts, const int64_t *rights,
                          const mi355_sw_params *params, float *maxima);

/* mi355_sw_score_ranges for callers that only need the WINNER: per resident query the first range with the strictly
 * greatest maximum (best[q], best_range[q]; -1 / -1 without ranges) — all OMPParallelLocalAligner does with the per-piece
 * maxima (plocalaligner.cpp:106,122-129).  That freedom lets a lone long query take the cheaper sampled sweep: ranges that
 * cannot hold the greatest maximum are not re-evaluated, so their entries of `maxima` (optional, may be NULL) are LOWER BOUNDS
 * of unspecified slack (the sampled running maximum and the optimistic warm-up margin below both only ever lower a value; never
 * above the true maximum of the range).  Exact: best, best_range, and the entry of every range whose maximum equals `best`.
 * A lone long query is also swept with an OPTIMISTIC warm-up margin in front of its tiles: enough for maxima above 11/12 of
 * the best possible score, not for every cell.  exact_above == NULL: the call checks its own best against
 * what that margin certifies and sweeps again with the margin its best needs when it falls short — results as above.
 * exact_above != NULL (multi-GPU reference sharding: every rank calls this on its own pieces and the packed (best, ~piece)
 * keys are merged by one 8-byte all-reduce(MAX)): no second sweep here; *exact_above = the value above which this call was
 * exact (the same on every rank; -1: everything).  When the MERGED best does not exceed it, every rank calls again with
 * known_best = the merged best (a lower bound of the true one): the margin is then the one that value needs, and the second
 * merge is exact.  known_best <= 0: nothing known. */
int mi355_sw_best_range(mi355_sw_ctx *ctx, size_t nranges, const int64_t *lefts, const int64_t *rights,
                        const mi355_sw_params *params, float known_best, float *maxima, float *best, int64_t *best_range,
                        float *exact_above);

/* Finishes range `range_index` of the LAST mi355_sw_score_ranges / mi355_sw_best_range call on this context as a stand-alone problem: argmax
 * cell and traceback of every resident query within [lefts[k], rights[k]) — what LAT(sequence_x, winning piece) computes
 * (plocalaligner.cpp:132-137); pos / end_y are relative to the range start (the caller adds `left`, :137).  When `params`
 * equals the scoring and engine of that sweep, its per-range keys are used and only the argmax window and the traceback
 * run (the reference sweeps the winning piece a second time); otherwise the range is swept again under `params`.
 * outs[n_queries].  MI355_SW_EINVAL when reference or batch changed since the sweep. */
int mi355_sw_align_scored_range(mi355_sw_ctx *ctx, size_t range_index, const mi355_sw_params *params, int flags,
                                mi355_sw_result *outs);

/* ---- affine gaps: score, end cell and traceback -------------------------------------------------------------------
 * A gap of k consecutive columns (or rows) costs gap_open + (k - 1) * gap_extend.  With s = f(x[i], y[j]) (identity or
 * table, exactly as mi355_sw_params):
 *
 *   E(i,j) = max(E(i,j-1) - gap_extend, H(i,j-1) - gap_open)
 *   F(i,j) = max(F(i-1,j) - gap_extend, H(i-1,j) - gap_open)
 *   H(i,j) = max(0, H(i-1,j-1) + s, E(i,j), F(i,j))           H = 0 on the borders; E, F = -infinity there
 *
 * Score = max H.  End cell = the first maximum in column-major order (smallest column of y, then smallest row of x),
 * 1-based: the float engine's rule (similaritymatrix.cpp:21-28).  An all-zero matrix gives score 0 and end 0 / 0.  With
 * gap_open == gap_extend == g this is the linear recurrence of MI355_SW_F32, and score, end_x and end_y equal that
 * engine's bit for bit.
 *
 * Traceback (mi355_sw_affine_align_trace, mi355_sw_affine_batch_trace).  Scores are integers, so every equality below is
 * exact in float32.  The walk starts in state M at the end cell and follows the recurrence:
 *
 *   state M at (i,j):  H(i,j) == 0                    stop: this cell is not part of the alignment
 *                      H(i,j) == H(i-1,j-1) + s       emit (x[i], y[j]), go to M at (i-1, j-1)
 *                      H(i,j) == E(i,j)               go to state E at (i, j), nothing emitted yet
 *                      else (H(i,j) == F(i,j))        go to state F at (i, j)
 *   state E at (i,j):  emit ('-', y[j]);  E(i,j) == H(i,j-1) - gap_open ? M at (i, j-1) : E at (i, j-1)
 *   state F at (i,j):  emit (x[i], '-');  F(i,j) == H(i-1,j) - gap_open ? M at (i-1, j) : F at (i-1, j)
 *
 * The first case that holds wins (diagonal over E over F), and opening a gap wins a tie with extending it: the shortest
 * gap.  The result follows the conventions of mi355_sw_result: cons_x / cons_y are REVERSED strings (from the end cell
 * to the beginning of the alignment) with '-' for gaps, NUL terminated, in one allocation released by
 * mi355_sw_free_result(s); pos is the 1-based column of y of the last pair emitted, i.e. the alignment's first column
 * (begin_y); end_x / end_y are the end cell.  Score 0 gives pos 0, empty strings and cons_len 0.  The alignment's first row
 * is begin_x = end_x + 1 - (number of bytes of cons_x other than '-').  timings_us[0] (and [1]) is the sweep time of the
 * call.  The strings are an optimal alignment under the recurrence: their value under (f, gap_open, gap_extend) is the
 * score.  With gap_open == gap_extend score and end cell equal the linear float engine's, but the strings are NOT that
 * engine's: the reference's traceback (smithwaterman.cpp:40-78) greedily follows the largest neighbour,
 * not the recurrence.
 *
 * MI355_SW_EINVAL: a non-finite value, gap_extend <= 0, gap_open < gap_extend.
 * MI355_SW_ENOTSUP (the message names the bound that was crossed) outside what the kernels compute exactly; a wrong
 * number never comes back.  Always computed: integer-valued scores (match / mismatch, or the table's entries for any
 * query byte against the reference's letters, and both gap costs) with smax * (longest query + 1) <= 2040 and
 * gap_open <= 2040 (smax: the greatest substitution score), queries of 1..512 rows, any reference length, while the
 * query profile fits LDS (53 reference letters at 512 rows, more for shorter queries).  Also always computed: queries of any
 * length (the database sequences of a search) against a reference, or a range of it, of 1..512 letters, with integer-valued
 * scores, smax * (letters + 1) < 2^18 and gap_open < 2^18, while the profile of the byte classes fits LDS (96 KiB: 127
 * classes of bytes with equal scores up to 160 letters, 75 up to 320, 41 up to 512; a 20-letter table has 21).  Beyond both, integer scores are still
 * computed wherever a (query, reference or range) problem has at most 2^26 cells and the query at most about 5 600 rows;
 * everything else is refused.
 * Option no_affine_sweep (A/B, tests): every problem on the exact kernel, refused above 2^26 cells per problem.
 * Option no_affine_prof (A/B, tests): references (ranges) of at most 512 letters on the exact kernel as well.
 * Lists of pairs (mi355_sw_affine_pairs_run, mi355_sw_affine_pairs_trace): a pair is always computed by the pair kernel when its
 * query has 1..512 rows and its window 1..2^20 columns, with integer-valued scores, smax * (rows + 1) < 2^18 and
 * gap_open < 2^18, while the score table [reference letters + 1][classes of query bytes with equal scores + 1] fits 32 KiB of
 * LDS (a 20-letter table: 25 x 21 entries) — whatever the size of the call.  Every other pair is a whole problem of the exact
 * kernel under its limits (2^26 cells, about 5 600 rows); one pair beyond those fails the whole call with MI355_SW_ENOTSUP.
 * Option no_affine_pairs (A/B, tests): every pair on the exact kernel.
 * The traceback calls follow the same rules; in addition one alignment whose decision window (DESIGN.md §3.8, L17 and L18:
 * the columns and the rows an alignment into the end cell can reach) needs more than 2^30 bytes, or has more than about
 * 5 600 rows, is refused with MI355_SW_ENOTSUP.
 * mi355_sw_last_path: "affine[cell=f16,SL=..,R=..]" when the sweep kernel ran, "affine_prof[R=..]" when the kernel for
 * references of at most 512 letters ran (calls of fewer than 2^18 cells stay on the exact kernel), "affine_exact" when the
 * exact kernel ran, "affine_trace" when the traceback kernel ran, "affine_pair[R=..]" once per instance of the pair kernel
 * that ran.
 * mi355_sw_last_timings: [0] sweep kernel(s) (both of them), [1] exact kernel (whole problems and end-cell windows),
 * [2] traceback kernel, [3] whole call, [4] sweep launches, [5] cells swept. */
typedef struct {
  const float *lut;        /* as mi355_sw_params.lut */
  float match, mismatch;   /* used when lut == NULL */
  float gap_open;          /* cost of the first column (row) of a gap */
  float gap_extend;        /* cost of every further one; 0 < gap_extend <= gap_open */
} mi355_sw_affine_params;
void mi355_sw_default_affine_params(mi355_sw_affine_params *p); /* 3 / -3 / open 5 / extend 1, no table */

/* One alignment of x (rows) against y (columns); y stays resident as for mi355_sw_align. */
int mi355_sw_affine_align(mi355_sw_ctx *ctx, const char *x, size_t nx, const char *y, size_t ny,
                          const mi355_sw_affine_params *params, float *score, int64_t *end_x, int64_t *end_y);
/* Every query of mi355_sw_batch_upload[_packed] against the reference of mi355_sw_set_reference: arrays of n_queries. */
int mi355_sw_affine_batch_run(mi355_sw_ctx *ctx, const mi355_sw_affine_params *params,
                              float *score, int64_t *end_x, int64_t *end_y);
/* The same two calls with the traceback: pos and the reversed consensus strings by the rule above.  out / outs (n_queries
 * results) must not be NULL (MI355_SW_EINVAL); release the strings with mi355_sw_free_result(s). */
int mi355_sw_affine_align_trace(mi355_sw_ctx *ctx, const char *x, size_t nx, const char *y, size_t ny,
                                const mi355_sw_affine_params *params, mi355_sw_result *out);
int mi355_sw_affine_batch_trace(mi355_sw_ctx *ctx, const mi355_sw_affine_params *params, mi355_sw_result *outs);
/* The affine counterpart of mi355_sw_score_ranges: maxima[k * n_queries + q], each range an independent problem with a
 * zero left border. */
int mi355_sw_affine_score_ranges(mi355_sw_ctx *ctx, size_t nranges, const int64_t *lefts, const int64_t *rights,
                                 const mi355_sw_affine_params *params, float *maxima);

/* npairs independent problems: resident query query[k] (index into the batch of mi355_sw_batch_upload[_packed]) against the
 * window [lefts[k], rights[k]) of the resident reference (0-based, half open, as mi355_sw_affine_score_ranges).  Each pair is
 * a stand-alone problem with zero borders: score[k], end_x[k], end_y[k] are exactly what
 * mi355_sw_affine_align(x_query[k], y + lefts[k], rights[k] - lefts[k]) returns; end_y is relative to the window start
 * (1-based; the caller adds lefts[k]), 0 / 0 / 0 for an empty query, an empty window or no positive cell.  A query may occur
 * in any number of pairs; windows may overlap, touch column 0 or end at the reference's last column.  Results come back in
 * the caller's pair order.  npairs == 0 returns 0 and writes nothing.  MI355_SW_EINVAL: a NULL array, query[k] outside
 * [0, n_queries), lefts[k] < 0, rights[k] < lefts[k] or rights[k] > the reference length; the scoring checks and
 * MI355_SW_ENOTSUP as for every affine call (bounds: the paragraph above).  After any error the context stays usable.
 * mi355_sw_last_timings: [0] pair kernel, [1] exact kernel, [2] traceback kernel, [3] whole call, [4] pair-kernel launches,
 * [5] cells of the pair kernel. */
int mi355_sw_affine_pairs_run(mi355_sw_ctx *ctx, size_t npairs, const int32_t *query, const int64_t *lefts, const int64_t *rights,
                              const mi355_sw_affine_params *params, float *score, int64_t *end_x, int64_t *end_y);
/* The same with the traceback: outs[k] as mi355_sw_affine_align_trace on that slice (pos relative to the window start);
 * outs must not be NULL; release the strings with mi355_sw_free_results. */
int mi355_sw_affine_pairs_trace(mi355_sw_ctx *ctx, size_t npairs, const int32_t *query, const int64_t *lefts, const int64_t *rights,
                                const mi355_sw_affine_params *params, mi355_sw_result *outs);

/* ---- lists of pairs, end-to-end mode ("fit", "glocal": a mapper's extension stage that must not clip the read) --------
 * Every letter of the query x (m rows) is aligned, the flanks of the window y (n columns) are free, and the score may be
 * negative.  With s = f(x[i], y[j]), o = gap_open, e = gap_extend, o >= e > 0:
 *
 *   E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)
 *   F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)
 *   H(i,j) = max(H(i-1,j-1) + s, E(i,j), F(i,j))                       no zero floor
 *   H(0,j) = 0, E(0,j) = F(0,j) = -infinity   for j = 0..n             the window's flanks are free
 *   H(i,0) = F(i,0) = -(o + (i-1) e), E(i,0) = -infinity   for i >= 1  (column 0: the same recurrence with only its F term)
 *
 * Score = max over 1 <= j <= n of H(m, j); it may be negative or 0.  end_x = m; end_y = the smallest such j, 1-based and
 * relative to the window start.  An empty query or an empty window has no alignment: score 0, end 0 / 0, empty strings.
 *
 * Traceback: the priorities of the local rule (diagonal over E over F, opening wins a tie with extending).
 *
 *   state M at (i,j):  i == 0                         stop
 *                      j == 0                         go to state F at (i, 0)
 *                      H(i,j) == H(i-1,j-1) + s       emit (x[i], y[j]), go to M at (i-1, j-1)
 *                      H(i,j) == E(i,j)               go to state E at (i, j)
 *                      else                           go to state F at (i, j)
 *   states E and F: as in the local rule; in column 0 only F moves happen, until row 0.
 *
 * So cons_x without its '-' is all of x, reversed, and begin_x = 1; pos = begin_y is the column of the last emitted pair
 * that carries a letter of y, 0 if there is none; the value of the two strings under (f, o, e) is the score.
 *
 * mode: MI355_SW_AFFINE_LOCAL is mi355_sw_affine_pairs_run / _trace themselves (same code path, same bytes, same
 * mi355_sw_last_path); MI355_SW_AFFINE_END_TO_END is the model above; any other value: MI355_SW_EINVAL.  Arguments, their
 * checks and their order, ownership of the results, timings, mi355_sw_last_kernel and "the context stays usable after any
 * error" are those of the two calls above.  Dispatch is theirs as well: the pair kernel for 1..512 rows and 1..2^20 columns
 * while the score table fits 32 KiB of LDS, the exact kernel (2^26 cells, about 5 600 rows) for every other pair, else
 * MI355_SW_ENOTSUP; option no_affine_pairs sends every pair to the exact kernel.  End-to-end mode reserves no mantissa bits
 * and floors nothing, so its admission test is that every value formed is an integer below 2^24 in magnitude — with smin
 * (smax) the least (greatest) substitution score, both taken with 0:
 *     2 gap_open + (rows + 1) gap_extend - smin < 2^24     and     smax (rows + 1) + gap_open < 2^24
 * (H >= -(o + (m-1) e) by the all-F path from row 0; H - o, E, F >= -(2o + m e), and one e lower before their maximum; the
 * diagonal term >= -(2o + m e) + (smin + o), which the first inequality covers as well; upwards H <= smax m and the table
 * holds s + o).  A pair outside it goes to the exact kernel, which forms no s + o and holds a pair while
 * 2 gap_open + (rows + 1) gap_extend < 2^24, gap_open + rows gap_extend - smin < 2^24 and smax (rows + 1) < 2^24; a pair
 * beyond that is MI355_SW_ENOTSUP.  mi355_sw_last_path: "affine_pair_e2e[R=..]" once per instance of the pair kernel that ran, "affine_exact" and
 * "affine_trace" as above.  The traceback window: DESIGN.md §3.8, L19. */
enum { MI355_SW_AFFINE_LOCAL = 0, MI355_SW_AFFINE_END_TO_END = 1 };
int mi355_sw_affine_pairs_run_mode(mi355_sw_ctx *ctx, int mode, size_t npairs, const int32_t *query, const int64_t *lefts,
                                   const int64_t *rights, const mi355_sw_affine_params *params, float *score, int64_t *end_x,
                                   int64_t *end_y);
int mi355_sw_affine_pairs_trace_mode(mi355_sw_ctx *ctx, int mode, size_t npairs, const int32_t *query, const int64_t *lefts,
                                     const int64_t *rights, const mi355_sw_affine_params *params, mi355_sw_result *outs);

/* ---- lists of pairs, banded pairs (a mapper extends inside a band around its seed's diagonal: BWA-MEM -w, minimap2 -r) ----
 * Pair k is query x (m rows) against window y (n columns) as in mi355_sw_affine_pairs_run, and has a band
 *
 *     band_lo[k] <= j - i <= band_hi[k]          i the 1-based row, j the 1-based column relative to the window start; signed
 *
 * (a seed at read offset p and window offset q with half width w: [q - p - w, q - p + w]).  Cells outside the band are not part
 * of the matrix: H = E = F = -infinity there.  Inside the band the local recurrence above holds unchanged, the zero floor
 * included, and the borders keep H = 0 where they lie in the band.  For the local model this is the same as saying that an
 * out-of-band neighbour holds H = 0 and E = F = -infinity: it then contributes at most -gap_open < 0 and never wins.
 *
 * Score: the maximum of H over the in-band cells.  End cell: the first maximum in column-major order among the in-band cells.
 * No positive in-band cell, or a band that misses the matrix: score 0, end 0 / 0, empty strings.  Traceback: the rule above,
 * unchanged; an equality with -infinity never holds, so the walk never leaves the band: every emitted pair and gap letter lies
 * on an in-band cell, and the value of the strings is the score.  A band changes answers: an alignment that leaves it does
 * not count.
 *
 * Effective band: lo_e = max(band_lo, 1 - m), hi_e = min(band_hi, n - 1), W = hi_e - lo_e + 1 diagonals.  lo_e > hi_e: zeros.
 * lo_e == 1 - m and hi_e == n - 1 (the band covers the matrix): the pair IS the unbanded pair, on today's code path with
 * today's bytes.  Every other pair is computed by the band kernel when it has 1..512 rows and W <= 256, under the pair kernel's
 * bounds (integer scores, smax * (rows + 1) < 2^18, gap_open < 2^18, the score table within 32 KiB of LDS) — work in
 * proportion to rows x W — and else by the exact kernel under a band, within that kernel's limits (2^26 cells of rows x
 * columns, about 5 600 rows); one pair beyond those fails the whole call with MI355_SW_ENOTSUP, naming the pair.  A banded
 * pair never falls back to an unbanded kernel.  Option no_affine_band (A/B, tests): every banded pair on the exact kernel.
 *
 * Arguments, their checks and the order of those checks, ownership of the results and "the context stays usable after any
 * error" are those of the _mode calls.  band_lo == NULL and band_hi == NULL: the _mode call itself (same code path, same
 * bytes, same mi355_sw_last_path).  Exactly one of the two NULL, or band_hi[k] < band_lo[k]: MI355_SW_EINVAL.
 * MI355_SW_AFFINE_END_TO_END with bands is not supported yet (the column-0 border inside a band, and pairs whose band reaches
 * no cell of row m, need decisions of their own): MI355_SW_ENOTSUP after the argument checks.
 * mi355_sw_last_timings: [0] includes the band kernel, [4] / [5] count its launches and its cells, rows x W per pair.
 * mi355_sw_last_path: "affine_band[R=..]" once per instance of the band kernel that ran (R registers per lane, 16 R
 * diagonals; R is one of kBandR in csrc/sw_affine_band_kernel.h: 1, 2, 3, 5, 7, 9, 12, 16), "affine_exact_band" when the exact kernel ran under a band, beside the tags above.
 * mi355_sw_last_kernel names the instance ("sw_affine_band_kernel<R=..>") and its ops per cell.  DESIGN.md §3.8, L20. */
int mi355_sw_affine_pairs_run_band(mi355_sw_ctx *ctx, int mode, size_t npairs, const int32_t *query, const int64_t *lefts,
                                   const int64_t *rights, const int64_t *band_lo, const int64_t *band_hi,
                                   const mi355_sw_affine_params *params, float *score, int64_t *end_x, int64_t *end_y);
int mi355_sw_affine_pairs_trace_band(mi355_sw_ctx *ctx, int mode, size_t npairs, const int32_t *query, const int64_t *lefts,
                                     const int64_t *rights, const int64_t *band_lo, const int64_t *band_hi,
                                     const mi355_sw_affine_params *params, mi355_sw_result *outs);

/* ---- lists of pairs, anchored seed extension, forward and backward (BWA-MEM ksw_extend, minimap2 ksw_extz) ----------------
 * A mapper starts AT its seed and extends away from it: the alignment is anchored at the seed's edge and ends where the score
 * peaks (a soft clip) or at the read's end; the mapper picks between the two by comparing the two scores, to the right of the
 * seed and again to the left on both strings reversed.
 *
 * Pair k is the letters [q_lo[k], q_hi[k]) of resident query query[k] against the window [lefts[k], rights[k]) of the resident
 * reference, in direction backward[k].  Call the letters x (m = q_hi - q_lo rows) and the window y (n columns).
 * Forward (backward[k] == 0): x and y as they stand; the anchor is in front of x[1] and y[1].  Backward: x and y both reversed;
 * the anchor is behind the query range's last letter and the window's last column: the left extension of a seed.  It is DEFINED
 * as the forward model on the two reversed strings.  With s = f(x[i], y[j]), o = gap_open, e = gap_extend, o >= e > 0:
 *
 *   E(i,j) = max(E(i,j-1) - e, H(i,j-1) - o)
 *   F(i,j) = max(F(i-1,j) - e, H(i-1,j) - o)
 *   H(i,j) = max(H(i-1,j-1) + s, E(i,j), F(i,j))                          no zero floor
 *   H(0,0) = 0
 *   H(0,j) = E(0,j) = -(o + (j-1) e), F(0,j) = -infinity   for j >= 1     the anchor is fixed: a flank is a gap
 *   H(i,0) = F(i,0) = -(o + (i-1) e), E(i,0) = -infinity   for i >= 1
 *
 * Best extension: score = max of H over 0 <= i <= m, 0 <= j <= n.  It is >= 0, because cell (0,0) competes; score 0 means
 * "extend nothing".  end_x, end_y = the first maximum in column-major order (smallest column, then smallest row), reported as
 * lengths: the letters of x and the columns of y the extension consumes.  A forward extension covers query letters
 * [q_lo, q_lo + end_x) and reference columns [left, left + end_y); a backward extension covers [q_hi - end_x, q_hi) and
 * [right - end_y, right).  Score 0 always comes with end 0 / 0: column 0 wins every tie, and the border cells are negative.
 *
 * To the end: to_end_score = max over 0 <= j <= n of H(m, j), of any sign; to_end_y = the smallest such j, which may be 0: the
 * whole of x as one insertion.  This is what a mapper compares with score + clip penalty; the library does not take that decision.
 *
 * Traceback: the priorities of the other models (diagonal over E over F, opening wins a tie with extending).  The walk starts in
 * state M at the chosen cell — the best extension's by default, (m, to_end_y) where to_end[k] != 0 — and stops at (0,0) and
 * nowhere else; in row 0 only E moves happen, in column 0 only F moves.  The strings run from the far end to the anchor: a forward
 * pair's cons_x / cons_y are reversed, as in every mi355_sw_result, and a backward pair's strings therefore read left to right in
 * the original strings.  The value of the strings under (f, o, e) is the traced cell's score; cons_x without '-' has end_x
 * letters and cons_y without '-' has end_y letters; pos = 1 when the strings hold a letter of y, else 0.  outs[k].score / end_x /
 * end_y describe the traced alignment.
 *
 * Degenerate pairs.  m = 0: everything is 0 and the strings are empty.  n = 0, m >= 1: the best extension is 0 / 0 / 0,
 * to_end_score = -(o + (m-1) e) and to_end_y = 0; its traceback is m letters of x against m '-'; the host fills this in, no
 * kernel runs.
 *
 * Arguments: to_end_score and to_end_y may both be NULL; to_end == NULL: the best extension for every pair; backward == NULL:
 * every pair forward; q_lo == q_hi == NULL: the whole query.  Argument checks and their order follow the pairs calls.
 * MI355_SW_EINVAL: list is NULL; query, lefts or rights is NULL; exactly one of q_lo / q_hi is NULL; q_lo < 0, q_hi < q_lo or
 * q_hi > the query's length; the pairs calls' own checks fail.  npairs == 0 returns 0 and writes nothing.  After any error the
 * context stays usable.
 *
 * Dispatch: the extension instance of the pair kernel for 1..512 rows and 1..2^20 columns while the score table fits 32 KiB of
 * LDS and the admission test holds — every value the kernel forms is an integer below 2^24 in magnitude, and a positive score
 * leaves the winner's key five mantissa bits; with smin (smax) the least (greatest) substitution score, both taken with 0:
 *     3 gap_open + (rows + columns) gap_extend - smin < 2^24,   smax rows + gap_open < 2^24   and   smax (rows + 1) < 2^18
 * (H(i,j) >= -(2o + (i+j-2) e) by the path along row 0 and down column j; H - o, E, F >= -(3o + (m+n-2) e), and one e lower
 * before their maximum; the diagonal term is (H - o) + (s + o) with s + o >= smin + o) — else the exact kernel (2^26 cells,
 * about 5 600 rows; 3 gap_open + (rows + columns) gap_extend < 2^24, 2 gap_open + (rows + columns) gap_extend - smin < 2^24,
 * smax (rows + 1) < 2^24), else MI355_SW_ENOTSUP naming the pair.  The traceback fills the whole rectangle from the anchor to
 * the traced cell: at most 2^30 decision bytes and about 5 600 rows, else MI355_SW_ENOTSUP.  Option no_affine_pairs sends every
 * pair to the exact kernel.  A backward pair runs as the forward pair on window [N - right, N - left) and letters
 * [len - q_hi, len - q_lo) of reversed copies of the reference and the batch, which the context builds on the device at the first
 * backward pair and keeps until the next mi355_sw_set_reference / mi355_sw_batch_upload; calls without a backward pair allocate
 * nothing for them.
 * mi355_sw_last_path: "affine_pair_ext[R=..]" once per instance of the pair kernel that ran, "affine_exact" and "affine_trace" as
 * above.  mi355_sw_last_timings and mi355_sw_last_kernel as for the pairs calls; the kernel's name is
 * "sw_affine_pair_ext_kernel<R=..>", with its ops per cell.  DESIGN.md §3.8, L21. */
typedef struct {
  size_t npairs;
  const int32_t *query;            /* resident query of pair k */
  const int32_t *q_lo, *q_hi;      /* its letters [q_lo, q_hi), 0-based, half open; both NULL: the whole query */
  const int64_t *lefts, *rights;   /* the window, as in mi355_sw_affine_pairs_run */
  const uint8_t *backward;         /* NULL: every pair forward */
} mi355_sw_extend_list;

int mi355_sw_affine_extend_run(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const mi355_sw_affine_params *params,
                               float *score, int64_t *end_x, int64_t *end_y, float *to_end_score, int64_t *to_end_y);
int mi355_sw_affine_extend_trace(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const mi355_sw_affine_params *params,
                                 const uint8_t *to_end /* NULL: best extension for every pair */,
                                 mi355_sw_result *outs, float *to_end_score, int64_t *to_end_y);

/* ---- lists of pairs, anchored seed extension inside a diagonal band (BWA-MEM ksw_extend w, minimap2 ksw_extz -r) ----------
 * A mapper never extends a seed over the full rectangle: it extends inside a band around the seed's diagonal.  Pair k is as in
 * mi355_sw_affine_extend_run — x with m rows, y with n columns, forward or backward — and has a band
 *
 *     band_lo[k] <= j - i <= band_hi[k]          i the letters of x, j the columns of y consumed from the anchor; signed
 *
 * The anchor (0,0) lies on diagonal 0, so band_lo <= 0 <= band_hi is required (ksw_extend's w is [-w, w]).  i and j are counted
 * from the anchor, so the band means the same for a backward pair, which stays the forward model on both strings reversed.
 *
 * Cells outside the band are not part of the matrix: H = E = F = -infinity there — -infinity and not 0, because the model has
 * no floor.  Inside the band the anchored recurrence and its borders hold unchanged: H(0,0) = 0, H(0,j) = E(0,j) =
 * -(o + (j-1) e) for in-band j >= 1, H(i,0) = F(i,0) = -(o + (i-1) e) for in-band i >= 1.  Every in-band cell is finite: it is
 * reachable from the anchor along diagonal 0 and then one gap.
 *
 * Best extension: the maximum of H over the in-band cells, >= 0 because (0,0) competes; the end cell is the first maximum in
 * column-major order, reported as lengths; score 0 comes with 0 / 0.
 * To the end: the maximum of H(m, j) over the in-band j in 0..n, at the smallest such j.  Row m has an in-band cell exactly when
 * band_lo <= n - m.  Otherwise the read's end is unreachable: to_end_score = -INFINITY and to_end_y = -1; no kernel decides
 * this, the host fills it in.  A pair with n = 0 and m >= 1 keeps the host-filled answer of the unbanded call when
 * band_lo <= -m, and is unreachable otherwise.
 * Traceback: the rule of the anchored model, unchanged.  An equality with -infinity never holds, so every emitted pair and gap
 * letter lies on an in-band cell, and the value of the strings is the traced score.  Where to_end[k] != 0 on an unreachable
 * pair: score -INFINITY, end 0 / 0, pos 0 and empty strings.
 *
 * Effective band: lo_e = max(band_lo, -m), hi_e = min(band_hi, n), W = hi_e - lo_e + 1 diagonals.  lo_e == -m and hi_e == n (the
 * band covers the matrix): the pair IS the unbanded pair, on the unbanded code path with its bytes and its mi355_sw_last_path.
 * Columns beyond m + hi_e are out of band in every row: the window is clipped to min(n, m + hi_e) columns before anything is
 * sized or dispatched, so a long window under a narrow band never reaches a cell-count limit.
 *
 * Dispatch: the extension instance of the band kernel for 1..512 rows and W <= 256 while the score table fits 32 KiB of LDS and
 * the admission test holds — every value of a real cell is an integer below 2^24 in magnitude, and a positive score leaves the
 * winner's key five mantissa bits; with smin (smax) the least (greatest) substitution score, both taken with 0, and a = -smin:
 *     a rows + 3 gap_open + (W + 1) gap_extend - smin < 2^24,   smax rows + gap_open < 2^24   and   smax (rows + 1) < 2^18
 * (the cheapest in-band path runs along diagonal 0 and then one gap, not along the borders: H(i,j) >= -(a min(i,j) + o +
 * (|j-i|-1) e); H - o, E, F one o lower, the scan's H - o of an F another o lower, and one e lower before their maximum; the
 * diagonal term is (H - o) + (s + o) with s + o >= smin + o) — work in proportion to rows x W.  Every other banded pair: the
 * exact kernel under the band, within its limits on the CLIPPED window (2^26 cells, about 5 600 rows, a rows + 2 gap_open +
 * W gap_extend - smin < 2^24 and smax (rows + 1) < 2^24); one pair beyond those fails the whole call with MI355_SW_ENOTSUP,
 * naming the pair.  A banded pair never runs on an unbanded kernel.  Option no_affine_band sends every banded extension to the
 * exact kernel; no_affine_pairs does so too.  Backward pairs reuse the reversed copies of the unbanded calls.
 *
 * Arguments, their checks and the order of those checks, ownership of the results and "the context stays usable after any
 * error" are those of mi355_sw_affine_extend_run / _trace; the band checks come last.  band_lo == NULL and band_hi == NULL: the
 * unbanded call itself (same code path, same bytes).  Exactly one of the two NULL, band_lo[k] > 0 or band_hi[k] < 0:
 * MI355_SW_EINVAL.
 * mi355_sw_last_path: "affine_band_ext[R=..]" once per instance of the band kernel that ran (R one of kBandR), "affine_exact_band"
 * when the exact kernel ran under a band, beside the tags above.  mi355_sw_last_timings: [0] includes the band kernel, [4] /
 * [5] count its launches and its cells, rows x W per pair.  mi355_sw_last_kernel names the instance
 * ("sw_affine_band_ext_kernel<R=..>") and its ops per cell.  DESIGN.md §3.8, L22. */
int mi355_sw_affine_extend_run_band(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const int64_t *band_lo,
                                    const int64_t *band_hi, const mi355_sw_affine_params *params, float *score,
                                    int64_t *end_x, int64_t *end_y, float *to_end_score, int64_t *to_end_y);
int mi355_sw_affine_extend_trace_band(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const int64_t *band_lo,
                                      const int64_t *band_hi, const mi355_sw_affine_params *params,
                                      const uint8_t *to_end /* NULL: best extension for every pair */,
                                      mi355_sw_result *outs, float *to_end_score, int64_t *to_end_y);

/* ---- lists of pairs, global alignment between two anchors, plain and banded (BWA-MEM ksw_global, minimap2's gap-filling ksw_extz) ----
 * The alignment BETWEEN two consecutive seeds of a chain: anchored at both ends.  Pair k is as in mi355_sw_affine_extend_run — x, the
 * letters [q_lo, q_hi) of resident query query[k], with m rows; y, the window [lefts[k], rights[k]) of the resident reference, with
 * n columns; backward[k] != 0 runs the pair on both strings reversed and is DEFINED as the forward model on the reversed strings, on
 * the reversed copies of the extension calls.  A gap fill has no direction: backward only chooses toward which side ties of the
 * walk fall.
 *
 * Model: the anchored model of mi355_sw_affine_extend_run, unchanged — the recurrence, o >= e > 0, no zero floor, and the borders
 * H(0,0) = 0, H(0,j) = E(0,j) = -(o + (j-1) e), H(i,0) = F(i,0) = -(o + (i-1) e).
 *
 * Score = H(m, n), of any sign; end_x = m and end_y = n always (lengths, as in the extension calls).
 *
 * Traceback: the anchored model's rule (diagonal over E over F, opening wins a tie with extending).  The walk starts in state M at
 * (m, n) and stops at (0,0) and nowhere else; in row 0 only E moves happen, in column 0 only F moves.  cons_x without '-' is all m
 * letters, cons_y without '-' is all n columns, and the value of the strings under (f, o, e) is the score.  pos = 1 when n >= 1,
 * else 0.  String orientation as in the extension calls: reversed for a forward pair, reading order for a backward pair.
 *
 * Degenerate pairs, filled in by the host (no kernel runs).  m = 0, n = 0: score 0, end 0 / 0, empty strings.  m >= 1, n = 0: score
 * -(o + (m-1) e), the m letters of x against m '-'.  m = 0, n >= 1: score -(o + (n-1) e), n '-' against the n letters of y — a pure
 * deletion between two adjacent seeds.
 *
 * Band (band_lo, band_hi: both NULL, or both given): the in-band cells are band_lo[k] <= j - i <= band_hi[k], i and j counted from
 * the anchor; band_lo[k] > 0 or band_hi[k] < 0: MI355_SW_EINVAL.  Outside the band H = E = F = -infinity.  Effective band: lo_e =
 * max(band_lo, -m), hi_e = min(band_hi, n), W = hi_e - lo_e + 1.  lo_e == -m and hi_e == n: the pair IS the unbanded pair — same
 * path, same bytes, same mi355_sw_last_path.  The corner is reachable exactly when band_lo <= n - m <= band_hi.  Otherwise the run
 * call returns score = -INFINITY, the trace call score -INFINITY, end 0 / 0, pos 0 and empty strings, and no kernel runs for such a
 * pair.  These rules cover the degenerate pairs too: n = 0 needs band_lo <= -m, and m = 0 needs band_hi >= n.  A reachable pair
 * has n <= m + hi_e: no window is clipped.
 *
 * Arguments, their checks and the order of those checks are those of mi355_sw_affine_extend_run_band; the band checks come last.
 * score == NULL (run) or outs == NULL (trace): MI355_SW_EINVAL.  npairs == 0 returns 0 and writes nothing.  After any error the
 * context stays usable.
 *
 * Dispatch.  The kernels form no key, so no value lends mantissa bits and the extension calls' smax (rows + 1)
 * < 2^18 does not apply; every value a kernel forms is an integer below 2^24 in magnitude; smin (smax) the least (greatest)
 * substitution score, both taken with 0, and a = -smin.  Unbanded: the global instance of the pair kernel for 1..512 rows and
 * 1..2^20 columns while the score table fits 32 KiB of LDS and
 *     3 gap_open + (rows + columns) gap_extend - smin < 2^24 and smax rows + gap_open < 2^24
 * Banded: the global instance of the band kernel for 1..512 rows and W <= 256 while the table fits and
 *     a rows + 3 gap_open + (W + 1) gap_extend - smin < 2^24 and smax rows + gap_open < 2^24
 * Every other pair: the exact kernel within the bounds of the extension calls (unbanded and under a band), else MI355_SW_ENOTSUP
 * naming the pair.  A banded pair never runs on an unbanded kernel.  The traceback is the extension calls', started at (m, n).
 * Option no_affine_pairs sends every pair to the exact kernel, no_affine_band every banded pair.
 * mi355_sw_last_path: "affine_pair_glob[R=..]" and "affine_band_glob[R=..]" once per instance that ran, "affine_exact",
 * "affine_exact_band" and "affine_trace" as above; a list of host-filled pairs alone leaves no kernel tag.  mi355_sw_last_timings as
 * for the pairs calls.  mi355_sw_last_kernel names "sw_affine_pair_glob_kernel<R=..>" or "sw_affine_band_glob_kernel<R=..>", with
 * its ops per cell. */
int mi355_sw_affine_global_run(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const int64_t *band_lo, const int64_t *band_hi,
                               const mi355_sw_affine_params *params, float *score);
int mi355_sw_affine_global_trace(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const int64_t *band_lo, const int64_t *band_hi,
                                 const mi355_sw_affine_params *params, mi355_sw_result *outs);

/* ---- lists of pairs, banded extension with a z-drop stop rule (BWA-MEM ksw_extend zdrop, minimap2 ksw_extz zdrop) ----------------
 * A mapper stops an extension that has run into junk: a chimeric read, or a seed at a false position, is not extended over all its
 * rows, and its best extension cannot jump across a stretch of mismatches to an unrelated match further down.  Pair k is a pair of
 * mi355_sw_affine_extend_run_band, unchanged — x with m rows, y with n columns, forward or backward, the band band_lo[k] <= j - i <=
 * band_hi[k] with band_lo <= 0 <= band_hi, the anchored recurrence and its borders, -infinity outside the band.  New is one scalar
 * per call, zdrop >= 0.
 *
 * Stop rule.  It runs over the rows i = 1, 2, ..., m - 1 in order; its running best starts at (B, bi, bj) = (0, 0, 0), the anchor.
 * For row i: r_i = the maximum of H(i, j) over the in-band real columns 0 <= j <= n of row i (column 0 is the border cell where it
 * lies in the band; columns beyond n never count), c_i = the smallest such column; a row with no such column (i + band_lo > n) has
 * r_i = -infinity.  If r_i > B then (B, bi, bj) = (r_i, i, c_i) — strictly greater: the earliest row that attains the running
 * maximum, at its smallest column.  Otherwise let d = |(i - bi) - (c_i - bj)|, the diagonal offset between the two cells; the
 * extension stops after row i when
 *     B - r_i - d gap_extend > zdrop
 * and an r_i of -infinity stops for every finite zdrop.  Row m is never tested: a stop there would leave nothing to skip.
 * rows_done[k] = the stop row s (1 <= s < m), or m when no row stopped; 0 for m = 0.  Rows beyond rows_done are not part of the
 * matrix.
 *
 * Definition by truncation: the results of pair k are those of mi355_sw_affine_extend_run_band on the first
 * rows_done[k] letters of x — for a backward pair, letters of the reversed string — same window, same band.  One exception: when
 * rows_done < m the read's end was not reached, so to_end_score = -INFINITY and to_end_y = -1, and a trace with to_end[k] != 0 on
 * such a pair is the empty alignment of the banded call's unreachable case.  Rows <= s do not depend on later rows, so the cells
 * are those of the full matrix; row s itself cannot hold the best, because r_s < B.  The best extension keeps the tie rule of the
 * extension calls (the first maximum in column-major order); the rule's (bi, bj) is only the stop test's own bookkeeping.
 * This is the library's own statement of the rule, not a port: it differs from BWA-MEM's loop in its tie choices (which row and
 * which column hold a repeated maximum).
 *
 * Degenerate pairs.  n = 0, m >= 1: the same rule on the border column, evaluated by the host (B stays 0 and d = i, so a row in
 * the band stops exactly when gap_open - gap_extend > zdrop, and the first row below the band stops).  m = 0: rows_done = 0.
 * zdrop = +INFINITY: the call IS mi355_sw_affine_extend_run_band / _trace_band — same path, same bytes, same mi355_sw_last_path —
 * and rows_done = m.  With a finite zdrop a band that covers the matrix does not re-route the pair to the pair kernel: every pair
 * with m, n >= 1 is a banded pair.
 *
 * Arguments, their checks and the order of those checks are those of the _band calls; then: band_lo == NULL and band_hi == NULL is
 * MI355_SW_EINVAL (bands are required: an unbanded z-drop has no kernel), and last, zdrop negative or NaN is MI355_SW_EINVAL.
 * rows_done may be NULL.  After any error the context stays usable.
 *
 * Dispatch.  The z-drop instance of the band kernel (a fourth mode of its body; the wavefront leaves its row loop when none of
 * its four pairs is still alive) where the banded extension call dispatches to the band kernel and zdrop < 2^24: the test is
 * formed as r_i + d gap_extend < B - floor(zdrop), both sides integers below 2^24 in magnitude (L24).  Every other pair takes the
 * exact path, which carries out the definition in two steps: the rows instance of the exact kernel under the band writes r_i and
 * c_i of every row, the host runs the rule, and the exact kernel under the band runs on the first rows_done letters.  The rows
 * instance holds at most 4 398 rows (two more words of LDS per row); a pair beyond that fails the call with MI355_SW_ENOTSUP,
 * naming the bound.  Options no_affine_band and no_affine_pairs send every pair to the exact path.
 * mi355_sw_last_path: "affine_band_extz[R=..]" once per instance that ran, "affine_exact_band_rows" and "affine_exact_band" for the
 * exact path's two steps, "affine_trace" as before.  mi355_sw_last_kernel names "sw_affine_band_extz_kernel<R=..>" with its ops
 * per cell.  mi355_sw_last_counter: "zdrop_stopped" = pairs with rows_done < m; "zdrop_rows_run" = the sum over the z-drop
 * instance's wavefronts of the rows their loops ran (four pairs share a wavefront, which leaves when all four are done).
 * Every affine call also counts its launches of the exact kernels: "exact_launches" = launches of any sw_affine_exact_* kernel
 * (at most 65 536 problems each; the rows instance included, which is also cut at 2^24 row words), "trace_launches" = launches of
 * any sw_affine_trace_* kernel (at most 65 536 problems and 2^30 decision bytes each).  Both are 0 where no such kernel ran. */
int mi355_sw_affine_extend_run_zdrop(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const int64_t *band_lo,
                                     const int64_t *band_hi, float zdrop, const mi355_sw_affine_params *params, float *score,
                                     int64_t *end_x, int64_t *end_y, float *to_end_score, int64_t *to_end_y,
                                     int64_t *rows_done /* may be NULL */);
int mi355_sw_affine_extend_trace_zdrop(mi355_sw_ctx *ctx, const mi355_sw_extend_list *list, const int64_t *band_lo,
                                       const int64_t *band_hi, float zdrop, const mi355_sw_affine_params *params,
                                       const uint8_t *to_end /* NULL: best extension for every pair */,
                                       mi355_sw_result *outs, float *to_end_score, int64_t *to_end_y, int64_t *rows_done);

/* Host-only helper: piece ranges [left,right). Returns MI355_SW_ERANGE where the reference asserts. */
int mi355_sw_make_string_range(int npiece, int64_t shortlen, int64_t longlen, float overlap_ratio,
                               int64_t *lefts, int64_t *rights);

/* Host-only helpers: Similarity_Matrix_Skewed::trueindex2rawindex / rawindex2trueindex
 * (similaritymatrix.cpp:330-346, :353-364) for a matrix built from (x of length nx, y of length ny);
 * indices are in the skewed class's INTERNAL coordinates (ti = column of y, tj = row of x). */
void mi355_sw_true2raw(size_t nx, size_t ny, size_t ti, size_t tj, size_t *ri, size_t *rj);
void mi355_sw_raw2true(size_t nx, size_t ny, size_t ri, size_t rj, size_t *ti, size_t *tj);

/* Full matrix on the device, copied out as float, column-major over y:
 * H[j*(nx+1) + i] = matrix(i, j), i = 0..nx, j = 0..ny.  For small problems (tests, operator()). */
int mi355_sw_fill_matrix(mi355_sw_ctx *ctx, const char *x, size_t nx, const char *y, size_t ny,
                         const mi355_sw_params *params, float *H);

/* find_index_of_maximum(): first maximum in the reference's storage order. */
int mi355_sw_argmax(mi355_sw_ctx *ctx, const char *x, size_t nx, const char *y, size_t ny,
                    const mi355_sw_params *params, int64_t *index_x, int64_t *index_y, float *max);

/* Device timings of the last batch/align call, microseconds (HIP events on the library's stream):
 * [0] score kernel(s), [1] argmax rescan, [2] traceback window + walk, [3] whole call (device),
 * [4] number of score-kernel launches, [5] cells swept by the score kernel(s). */
int mi355_sw_last_timings(const mi355_sw_ctx *ctx, double out[6]);

/* What the candidate filters of the last batch / align call did: [0] queries that exceeded their
 * candidate cap and were swept a second time on the exact instances (per-query fallback), [1] times the WHOLE batch was swept
 * again (more than half of it exceeded the cap), [2] candidate sub-chunks re-evaluated exactly, [3] walks of the
 * many-small-alignments batch that left the decision window in front of their argmax and were redone on whole-problem decisions
 * (DESIGN.md §4.3). */
int mi355_sw_last_counters(const mi355_sw_ctx *ctx, uint64_t out[4]);
/* One counter of the last call by name: "requeried", "whole_batch_again", "candidates", "left_window" (= [0..3] above) and
 * "first_settled" — uint8 engine: queries over their candidate cap whose first candidates, evaluated in order, settled them
 * without a second sweep; "saved_locates" / "saved_traces" — finish steps of a lone long query that started from the columns and
 * strip rows its sweep saved, "saved_fallbacks" — those that took the zero-border windows instead; "walk_widened" — times a
 * traceback walk reported that its decision window was too small (the greedy walk left what the window makes exact, DESIGN.md
 * §3.3 L2) and the alignment was run again with four times the column budget: one count per alignment and round;
 * "wait_retries" — launches
 * repeated on a non-waiting instance after a wait between workgroups expired; "early_settled" — uint8 engine: queries settled
 * from the first and last sub-chunks without a sweep; "beyond_f16" — sequences of a many-small-alignments batch whose maximum lay
 * beyond the packed float16 pass's key range and were redone on float32 cells; "prefix_certified" — float engine, short-read
 * batches against a long reference: queries settled by the prefix-row filter, i.e. without a sweep of all
 * their rows (its offenders are swept on all rows and counted by "requeried"; when more than half of a batch offends the whole batch
 * is swept, "whole_batch_again").  Options of the filter (mi355_sw_set_option): "no_prefix" switches it off (the A/B),
 * "prefix_min_cols" = n moves the reference length from which it engages (default 8 Mi columns).  mi355_sw_last_kernel then names the
 * prefix instance and its `cells` are the cells that launch swept (P rows per read), not |x| * |y|.
 * A bucket of at least 512 reads is probed with its first 64, at the next lower prefix height on tiles that fold row P alone; the
 * probe decides the height of the rest.  "no_prefix_low" keeps such a bucket at its own height with the fold over
 * all prefix rows (the A/B).
 * A probed bucket of at least 1024 reads takes its heights as a chain: the probe runs at the lowest eligible height on tiles that fold
 * row P at every step (no slack), the rest of the bucket starts at the lowest height the probe's offender count pays for, and the
 * offenders of that pass take ONE prefix pass at the next height before the sweep of all rows; "prefix_second_pass" counts the reads
 * that took it.  "no_prefix_cascade" gives such buckets the flow of the smaller ones, "no_prefix_step" keeps the chain on the tiles
 * that fold every 4th step (both A/Bs).
 * On those step tiles the flags of a pass are thinned before the locate stage: each flagged sub-chunk is evaluated on the read's first
 * 38 rows, and only the sub-chunks where that row reaches its own threshold go on.  A read over its candidate cap
 * with up to 1024 flags is thinned instead of offending (65 536 flags for all such reads of a pass, the fewest first); "prefix_thinned" counts the reads whose flags took the thin stage,
 * "prefix_thin_items" the (read, sub-chunk) items it evaluated, and "candidates" what reached the locate stage.  "no_prefix_thin"
 * switches the stage off (the A/B); "prefix_thin_min_cols" = n moves the reference length from which it engages (default 4 Mi columns:
 * below the default of "prefix_min_cols").
 * "pooled_loops" — per-item host loops that went to the library's worker threads (big batches: from 49 152 alignments per call, or
 * from 1024 per loop when MI355_SW_POOL_THREADS is set; 0: every loop ran on the calling thread).  Unlike the others it is counted
 * per host thread, not per context: the value is that of the last call the CALLING thread made into the library that does any
 * work on a context (this function and the other mi355_sw_last_* readers leave it alone).
 * MI355_SW_EINVAL for an unknown name. */
int mi355_sw_last_counter(const mi355_sw_ctx *ctx, const char *name, uint64_t *out);

/* Test hook.  After a mi355_sw_score_ranges call of ONE range under mi355_sw_set_option("prefix_rowp", R) — the bucket of the prefix
 * shape swept by the instance of R rows per lane that folds row P = 2 R alone — the value of every sub-chunk of the range as the tiles
 * published it, in score units: values[q * *n_sub + s] for resident query q, -1 for queries the hook did not sweep.  *n_sub = 0 (and
 * nothing written) when the last call left no such values; values may be NULL to ask for *n_sub alone.
 * mi355_sw_set_option("prefix_rowp_step", R) works the same way on the instance that folds row P at every step. */
int mi355_sw_prefix_values(mi355_sw_ctx *ctx, float *values, size_t capacity, size_t *n_sub);

/* Test hook, open only under mi355_sw_set_option("prefix_thin_items", "1").  The thin stage of the prefix filter
 * on a caller's list: items[2 k], items[2 k + 1] = (resident query, sub-chunk of sub_len columns) of the range [left, right) of the
 * resident reference, as a row-P pass (P rows) would flag them; P2 is the taller height (38).  Per item the kernel sweeps the
 * read's first P2 rows over [s sub_len - 64 - warm, (s + 1) sub_len + W12) clipped to the range; values[k * *n_per_item + t] is the
 * maximum of row P2 over the item's own columns — from s sub_len - 63 on — inside sub-chunk s - 1 + t, -1 where there is no such
 * column.  values may be NULL to ask for *n_per_item alone.  MI355_SW_ENOTSUP where the library would not thin (heights, reads of at
 * most P2 rows, sub_len below 64, non-integer scores). */
int mi355_sw_prefix_thin_items(mi355_sw_ctx *ctx, size_t n_items, const uint32_t *items, int P, int P2, int64_t sub_len, int64_t left, int64_t right,
                               const mi355_sw_params *params, float *values, size_t capacity, size_t *n_per_item);

/* The seed stage of the chained prefix filter.  A chained bucket (>= 1024 reads, reference of at least
 * "prefix_seed_min_cols" columns, default 4 Mi) first looks for exact k-letter seeds of its reads in the reference — disjoint seeds at
 * offsets 0, k, 2k, ..., one scan of the reference per call (sw_seed_kernel.h) —, takes B0 of a read from the window of its best seed
 * cluster, and then sweeps every read at the lowest prefix height (16, 20, 26, 32 or 38 rows) that can certify it against this
 * reference's measured background, one pass per height: path tags "prefix_seed[k=..,hits=..]", "prefix_group[R=..,n=..]" per pass,
 * "prefix_calibrated[..]" in the call that measured the background table (once per reference and scoring), "prefix_seed_failed" when
 * more than half of the bucket has no seed B0 (the flow is then the probed chain's, exactly).  Counters (mi355_sw_last_counter):
 * "prefix_seeded" — reads whose B0 came from seed hits, "prefix_seed_hits" — hits the scan reported, "prefix_calibrated" — tables
 * measured in the call.  "no_prefix_seed" gives the probed chain (the A/B).  Results are the same either way.
 *
 * mi355_sw_seed_k: the seed length for reads of at least min_len letters over `letters` distinct letters against n columns — the
 * smallest k with letters^k >= (min_len / k) n that leaves 4 seeds in the shortest read; 0: none.  mi355_sw_seed_hash: the rolling
 * hash of k code bytes.  mi355_sw_seed_cluster: the cluster rule on one read's hits (start = position - offset, offset): for every
 * hit as the anchor the hits with start in [anchor, anchor + width]; most distinct offsets win, then the lowest start.  Returns 1
 * and the cluster's lowest and highest start, 0 without hits.  None of the three needs a device.
 *
 * mi355_sw_seed_hits (test hook): the scan over [left, right) of the resident reference for the resident batch with seeds of k
 * letters (0: the rule above on the batch's shortest read; the k used goes to *k_used).  counts[q] = hits of query q, exact;
 * the first 32 of them, in no particular order, as starts[q * 32 + j] = position - offset relative to `left` (may be negative) and
 * offsets[q * 32 + j].  A seed with a letter the reference does not hold is left out, and so is a seed that repeats itself with a
 * period of at most k / 2 letters (poly-A, a microsatellite).
 *
 * Reads an intact seed must find: a seeded read whose hits are all listed and whose deficit d = smax m - B0
 * satisfies floor(d / min(gap, smax)) < u — u the read's seeds in the table — keeps an intact seed in every alignment of score >= B0,
 * so the windows of all its hits give its result and it takes no pass: path tag "seed_certify[n=..,windows=..]", counter
 * "seed_certified" (apart from "prefix_certified").  "no_seed_certify" gives the flow without it (the A/B), "seed_certify_min_cols"
 * moves its size gate (default 4 Mi columns, independent of "prefix_seed_min_cols"); "seed_ride" = 1 / 2 / 3 picks how a small group
 * of the remaining reads rides with a taller one (cascade / near heights only / not at all).  Results are the same either way.
 * Host functions behind it, none needs a device (test hooks): mi355_sw_seed_usable — u of one read for seeds of k letters, `letters`
 * the bytes the reference holds; mi355_sw_seed_certify_ok — the rule, 1 or 0; mi355_sw_seed_certify_window — the 0-based end columns
 * [*lo, *hi] inside [0, n) of an alignment of score >= B0 through the intact seed of a hit with start = position - offset,
 * start + m - 1 - floor(d / min(gap, smax)) .. start + m - 1 + floor(d / gap); returns 1, or 0 when no column of the range is left. */
int mi355_sw_seed_usable(const uint8_t *read, int32_t len, int k, const uint8_t *letters, size_t n_letters);
int mi355_sw_seed_certify_ok(int64_t d, int64_t smax, int64_t g, int64_t u);
int mi355_sw_seed_certify_window(int64_t start, int64_t m, int64_t d, int64_t smax, int64_t g, int64_t n, int64_t *lo, int64_t *hi);
int mi355_sw_seed_k(int letters, int min_len, int64_t n);
uint32_t mi355_sw_seed_hash(const uint8_t *codes, int k);
int mi355_sw_seed_cluster(size_t n_hits, const int64_t *starts, const int32_t *offsets, int64_t width, int64_t *lo, int64_t *hi, int *distinct);
int mi355_sw_seed_hits(mi355_sw_ctx *ctx, int64_t left, int64_t right, int k, uint32_t *counts, int64_t *starts, int32_t *offsets, int *k_used);

/* The tile length of a pass of the seeded flow by how its launch fills the chip.  The passes of the groups ("prefix_group"
 * tags, their second passes included) on a range of at least "prefix_fill_min_cols" columns (default 4 Mi) take the cheapest tile under
 *   cost(c) = ceil((warm + c + lanes) / 64) x 64 x (workgroups / slots + f0),   f0: the tail of a launch, in rounds,
 * with workgroups = pairs x ceil(ceil(cols / c) / (256 / lanes)) against slots = cus x resident (the resident workgroups per CU of the
 * instance, asked of the runtime), among the multiples of the sub-chunk length from the shortest tile whose warm-up redundancy
 * (warm + lanes) / c stays under `cap` up to old_len, the length of the rule before — and only for a predicted gain of at least 4 %.
 * A launch of more than 2 rounds (workgroups / slots) at old_len keeps old_len: nothing deeper has been measured.
 * "no_prefix_fill" gives the rule before (the A/B, whatever else is set), "prefix_group_chunk" forces the length of these passes alone
 * (tuning aid; whole sub-chunks, at most 64 of them and at most the range).  Results
 * are the same either way; counters that depend on where tiles are cut ("candidates", "prefix_thin_items") may differ; "prefix_fill_moved" counts
 * the passes of the call whose tile the rule shortened, "prefix_fill_resident" is the resident count it took for the largest group.
 * mi355_sw_prefix_group_tile_len (test hook, no device): the rule.  resident <= 0 or any argument out of range: old_len.  f0 <= 0 /
 * cap <= 0: the library's constants, which mi355_sw_prefix_fill_constants returns with the gain threshold. */
int64_t mi355_sw_prefix_group_tile_len(int64_t pairs, int64_t cols, int64_t sub_len, int64_t warm, int lanes, int cus, int resident,
                                       int64_t old_len, double f0, double cap);
void mi355_sw_prefix_fill_constants(double *f0, double *cap, double *gain);

/* Which kernels and pipeline decisions the last call used: space-separated tags, each at most once, e.g.
 * "score[cell=f16,SL=8,R=19,...,sampled=1,...] strip[R=3,mode=max,...] wave[orient=0,...,dirs=1,...] walk_wave" — what the parity
 * tests assert a switch of mi355_sw_set_option ENGAGED with.  A call whose single-alignment chain declined after its launches
 * ("solo[...]") and went on to the general path keeps that tag beside the general path's.  Valid until the next call on the
 * context; never NULL. */
const char *mi355_sw_last_path(const mi355_sw_ctx *ctx);

/* Which sw_score_kernel instance swept the most cells in the last call (what the `iterate` of
 * similaritymatrix.cpp:99-264 / :386-561 became for this input): reporting aid for drivers and bench.py, so
 * that nobody re-derives the library's choice.  cells == 0 when the call did not use the score kernel. */
enum {
  MI355_SW_CELL_I16 = 0,   /* two queries per register, packed 16-bit integers */
  MI355_SW_CELL_U8 = 1,    /* uint8 engine, packed 16-bit integers with explicit saturation */
  MI355_SW_CELL_F32 = 2,   /* one query per register, float32 cells scaled by 2^-k */
  MI355_SW_CELL_F32U8 = 3, /* uint8 engine rule on integer-valued float32 cells, one query per register */
  MI355_SW_CELL_F16 = 4,   /* two queries per register, packed float16 cells holding H / 2048 */
  MI355_SW_CELL_U8H = 5    /* uint8 engine, packed float16 cells holding (H + 1) / 256 */
};
typedef struct {
  int cell;                 /* MI355_SW_CELL_* */
  int lanes;                /* lanes per tile: 8, 16 or 64 */
  int rows_per_lane;        /* R */
  int strips;               /* query swept in strips of lanes * rows_per_lane rows */
  int twin;                 /* two tiles of one query per packed register */
  int64_t chunk_len;        /* own columns per tile */
  int64_t sub_len;          /* columns per reported sub-chunk maximum */
  int64_t warm;             /* warm-up columns in front of a tile */
  double cells;             /* cells this instance swept in the call */
  double valu_ops_per_cell; /* VALU instructions per cell and lane of the inner loop (cost model) */
  char name[160];           /* e.g. "sw_score_kernel<R=19, f16x2, SL=8>" */
} mi355_sw_kernel_info;
int mi355_sw_last_kernel(const mi355_sw_ctx *ctx, mi355_sw_kernel_info *out);

/* ---- several GPUs of one node behind one handle (one process, one engine context + host thread per device) ----
 * The reference spreads the same work over OpenMP threads (pieces, src/aligner/plocalaligner.cpp:110-129) and MPI ranks
 * (independent alignments, src/mpi_sw_solve_uniprot.cpp:95-138).  Results are identical to the single-device calls.
 * devices == NULL or ndev <= 0: all visible devices.  A device may be listed more than once (the contexts are
 * independent), except with MI355_SW_MULTI_RCCL. */
typedef struct mi355_sw_multi mi355_sw_multi;
enum {
  MI355_SW_MULTI_RCCL = 1  /* merge the per-device best keys with ncclAllReduce(ncclMax, ncclUint64) over xGMI (RCCL is
                              loaded at run time) instead of on the host; needs distinct devices */
};
int mi355_sw_multi_create(mi355_sw_multi **m, int ndev, const int *devices, int flags);
void mi355_sw_multi_destroy(mi355_sw_multi *m);
const char *mi355_sw_multi_last_error(const mi355_sw_multi *m);
int mi355_sw_multi_set_option(mi355_sw_multi *m, const char *key, const char *value);   /* mi355_sw_set_option on every device's context */
int mi355_sw_multi_device_count(const mi355_sw_multi *m);
int mi355_sw_multi_rccl_version(const mi355_sw_multi *m);   /* ncclGetVersion code, 0 without MI355_SW_MULTI_RCCL */

/* mi355_sw_align_split with piece p swept by device p mod ndev; the per-device best (score, lowest piece) keys are
 * merged by MAX (serial rule plocalaligner.cpp:122-129), the owner of the winning piece re-aligns it (:132-141).
 * Every device keeps a copy of y resident between calls (same reuse rule as mi355_sw_align). */
int mi355_sw_multi_align_split(mi355_sw_multi *m, const char *x, size_t nx, const char *y, size_t ny,
                               const mi355_sw_params *params, int sm_semantics, int la_semantics,
                               int npiece, float overlap_ratio, mi355_sw_result *out, int *winning_piece);

/* mi355_sw_set_reference / mi355_sw_align_batch with the reference replicated and the alignments dealt to the
 * devices by length; outs[k] belongs to xs[k].  best_index (may be NULL): the alignment with the highest score,
 * lowest index on ties, -1 for an empty batch — the "best over the database" of the UniProt-shaped run. */
int mi355_sw_multi_set_reference(mi355_sw_multi *m, const char *y, size_t ny);
int mi355_sw_multi_align_batch(mi355_sw_multi *m, size_t n, const char *const *xs, const size_t *nxs,
                               const mi355_sw_params *params, int flags, mi355_sw_result *outs, int64_t *best_index);
/* as mi355_sw_last_timings: [0..3] maximum over the devices (they run side by side), [4..5] sums */
int mi355_sw_multi_last_timings(const mi355_sw_multi *m, double out[6]);

void mi355_sw_free_result(mi355_sw_result *r);
void mi355_sw_free_results(mi355_sw_result *r, size_t n);

/* Build information: "gfx950;..." */
const char *mi355_sw_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355_SW_H_ */
