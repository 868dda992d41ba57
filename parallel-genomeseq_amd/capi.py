"""ctypes binding of libmi355_sw.so (include/mi355_sw.h).  There is no CPU fallback: if the HIP
library is missing, or no MI355X is visible, every compute call raises."""
import ctypes as C
import os
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355_sw.so")

F32, U8SAT = 0, 1
SCORE_ONLY = 1

EXPORTS = [
    "mi355_sw_create", "mi355_sw_destroy", "mi355_sw_last_error", "mi355_sw_default_params",
    "mi355_sw_align", "mi355_sw_set_reference", "mi355_sw_align_batch", "mi355_sw_batch_upload",
    "mi355_sw_batch_run", "mi355_sw_score_ranges", "mi355_sw_align_scored_range", "mi355_sw_align_split", "mi355_sw_make_string_range", "mi355_sw_fill_matrix",
    "mi355_sw_argmax", "mi355_sw_true2raw", "mi355_sw_raw2true", "mi355_sw_last_timings", "mi355_sw_free_result", "mi355_sw_free_results",
    "mi355_sw_build_info", "mi355_sw_last_kernel", "mi355_sw_batch_run_view",
    "mi355_sw_multi_create", "mi355_sw_multi_destroy", "mi355_sw_multi_last_error", "mi355_sw_multi_device_count",
    "mi355_sw_multi_rccl_version", "mi355_sw_multi_align_split", "mi355_sw_multi_set_reference",
    "mi355_sw_multi_align_batch", "mi355_sw_multi_last_timings",
    "mi355_sw_set_option", "mi355_sw_option_names", "mi355_sw_multi_set_option", "mi355_sw_last_counters", "mi355_sw_last_counter", "mi355_sw_batch_upload_packed", "mi355_sw_best_range", "mi355_sw_last_path",
    "mi355_sw_default_affine_params", "mi355_sw_affine_align", "mi355_sw_affine_batch_run", "mi355_sw_affine_score_ranges",
    "mi355_sw_affine_align_trace", "mi355_sw_affine_batch_trace", "mi355_sw_affine_pairs_run", "mi355_sw_affine_pairs_trace",
    "mi355_sw_prefix_values", "mi355_sw_prefix_thin_items", "mi355_sw_affine_pairs_run_mode", "mi355_sw_affine_pairs_trace_mode",
    "mi355_sw_affine_pairs_run_band", "mi355_sw_affine_pairs_trace_band",
    "mi355_sw_affine_extend_run", "mi355_sw_affine_extend_trace",
    "mi355_sw_affine_extend_run_band", "mi355_sw_affine_extend_trace_band",
    "mi355_sw_affine_global_run", "mi355_sw_affine_global_trace",
    "mi355_sw_affine_extend_run_zdrop", "mi355_sw_affine_extend_trace_zdrop",
    "mi355_sw_seed_k", "mi355_sw_seed_hash", "mi355_sw_seed_cluster", "mi355_sw_seed_hits",
    "mi355_sw_seed_usable", "mi355_sw_seed_certify_ok", "mi355_sw_seed_certify_window",
    "mi355_sw_prefix_group_tile_len", "mi355_sw_prefix_fill_constants",
]
SEED_HIT_CAP = 32                                       # hits listed per read by the seed scan (kSeedHitCap of sw_seed_kernel.h)
AFFINE_LOCAL, AFFINE_END_TO_END = 0, 1                 # mode of the affine pairs calls (include/mi355_sw.h)
AFFINE_MODES = {"local": AFFINE_LOCAL, "end_to_end": AFFINE_END_TO_END}
MULTI_RCCL = 1


class Params(C.Structure):
    _fields_ = [("lut", C.POINTER(C.c_float)), ("match", C.c_float), ("mismatch", C.c_float),
                ("gap", C.c_float), ("semantics", C.c_int)]


class AffineParams(C.Structure):
    _fields_ = [("lut", C.POINTER(C.c_float)), ("match", C.c_float), ("mismatch", C.c_float),
                ("gap_open", C.c_float), ("gap_extend", C.c_float)]


class ExtendList(C.Structure):
    """mi355_sw_extend_list: the pairs of the extension calls."""
    _fields_ = [("npairs", C.c_size_t), ("query", C.POINTER(C.c_int32)), ("q_lo", C.POINTER(C.c_int32)), ("q_hi", C.POINTER(C.c_int32)),
                ("lefts", C.POINTER(C.c_int64)), ("rights", C.POINTER(C.c_int64)), ("backward", C.POINTER(C.c_uint8))]


class Result(C.Structure):
    _fields_ = [("score", C.c_float), ("pos", C.c_uint32), ("end_x", C.c_int64), ("end_y", C.c_int64),
                ("cons_x", C.c_void_p), ("cons_y", C.c_void_p), ("cons_len", C.c_size_t),
                ("timings_us", C.c_float * 2)]


class BatchView(C.Structure):
    _fields_ = [("n", C.c_size_t), ("score", C.POINTER(C.c_float)), ("pos", C.POINTER(C.c_uint32)),
                ("end_x", C.POINTER(C.c_int64)), ("end_y", C.POINTER(C.c_int64)), ("cons_x", C.POINTER(C.c_void_p)),
                ("cons_y", C.POINTER(C.c_void_p)), ("cons_len", C.POINTER(C.c_uint32)), ("timings_us", C.c_float * 2)]


class KernelInfo(C.Structure):
    _fields_ = [("cell", C.c_int), ("lanes", C.c_int), ("rows_per_lane", C.c_int), ("strips", C.c_int), ("twin", C.c_int),
                ("chunk_len", C.c_int64), ("sub_len", C.c_int64), ("warm", C.c_int64), ("cells", C.c_double),
                ("valu_ops_per_cell", C.c_double), ("name", C.c_char * 160)]


CELL_NAMES = {0: "i16", 1: "u8", 2: "f32", 3: "u8", 4: "f16", 5: "u8"}      # arithmetic type of the cells ("dtype" of bench.py)

_RESULT_DTYPE = np.dtype({"names": ["score", "pos", "end_x", "end_y", "cons_x", "cons_y", "cons_len", "t0", "t1"],
                          "formats": ["<f4", "<u4", "<i8", "<i8", "<u8", "<u8", "<u8", "<f4", "<f4"],
                          "offsets": [Result.score.offset, Result.pos.offset, Result.end_x.offset, Result.end_y.offset,
                                      Result.cons_x.offset, Result.cons_y.offset, Result.cons_len.offset,
                                      Result.timings_us.offset, Result.timings_us.offset + 4],
                          "itemsize": C.sizeof(Result)})


class MI355Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mi355_sw error %d: %s" % (code, msg))
        self.code = code


_LIB = None


def lib():
    """Load the HIP library; fail loudly when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmi355_sw.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C parallel-genomeseq_amd/csrc`")
        L = C.CDLL(LIB_PATH)
        L.mi355_sw_last_error.restype = C.c_char_p
        L.mi355_sw_build_info.restype = C.c_char_p
        L.mi355_sw_multi_last_error.restype = C.c_char_p
        L.mi355_sw_option_names.restype = C.c_char_p
        L.mi355_sw_last_path.restype = C.c_char_p
        L.mi355_sw_seed_hash.restype = C.c_uint32
        L.mi355_sw_prefix_group_tile_len.restype = C.c_int64
        L.mi355_sw_prefix_fill_constants.restype = None
        for name in EXPORTS:
            getattr(L, name)
        _LIB = L
    return _LIB


def make_params(semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None):
    p = Params()
    keep = None
    if lut is not None:
        keep = np.ascontiguousarray(lut, dtype=np.float32).reshape(65536)
        p.lut = keep.ctypes.data_as(C.POINTER(C.c_float))
    p.match, p.mismatch, p.gap, p.semantics = match, mismatch, gap, semantics
    return p, keep


def make_affine_params(match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
    p = AffineParams()
    keep = None
    if lut is not None:
        keep = np.ascontiguousarray(lut, dtype=np.float32).reshape(65536)
        p.lut = keep.ctypes.data_as(C.POINTER(C.c_float))
    p.match, p.mismatch, p.gap_open, p.gap_extend = match, mismatch, gap_open, gap_extend
    return p, keep


def _bytes(s):
    if isinstance(s, (bytes, bytearray)):
        return bytes(s)
    if isinstance(s, np.ndarray):
        return s.astype(np.uint8).tobytes()
    return s.encode("latin-1")


def _take(r):
    cx = C.string_at(r.cons_x, r.cons_len).decode("latin-1") if r.cons_len else ""
    cy = C.string_at(r.cons_y, r.cons_len).decode("latin-1") if r.cons_len else ""
    return dict(score=float(r.score), pos=int(r.pos), end_x=int(r.end_x), end_y=int(r.end_y),
                cons_x=cx, cons_y=cy, timings_us=(float(r.timings_us[0]), float(r.timings_us[1])))


def cigar(cons_x, cons_y):
    """Forward run-length string of an alignment given as the REVERSED consensus pair of a result: M = a letter pair (match or
    mismatch), I = a query letter against '-' (cons_y == '-'), D = a reference letter against '-' (cons_x == '-')."""
    if len(cons_x) != len(cons_y):
        raise ValueError("cigar: consensus strings of different lengths")
    out, last, run = [], "", 0
    for a, b in zip(reversed(cons_x), reversed(cons_y)):
        op = "D" if a == "-" else ("I" if b == "-" else "M")
        if op != last and run:
            out.append("%d%s" % (run, last))
            run = 0
        last, run = op, run + 1
    if run:
        out.append("%d%s" % (run, last))
    return "".join(out)


def _take_affine(r, end_to_end=False):
    """end_to_end: an alignment exists wherever there is an end cell, whatever the sign of its score."""
    cx = C.string_at(r.cons_x, r.cons_len).decode("latin-1") if r.cons_len else ""
    cy = C.string_at(r.cons_y, r.cons_len).decode("latin-1") if r.cons_len else ""
    ex, score = int(r.end_x), float(r.score)
    aligned = ex > 0 if end_to_end else score > 0
    return dict(score=score, end_x=ex, end_y=int(r.end_y), begin_x=(ex + 1 - (len(cx) - cx.count("-"))) if aligned else 0,
                begin_y=int(r.pos), pos=int(r.pos), cons_x=cx, cons_y=cy, cigar=cigar(cx, cy))


class Context:
    """One engine context = one GPU (mi355_sw_create)."""

    def __init__(self, device=0):
        self._L = lib()
        self._ctx = C.c_void_p()
        rc = self._L.mi355_sw_create(C.byref(self._ctx), C.c_int(device))
        if rc:
            raise MI355Error(rc, "mi355_sw_create failed (no usable HIP device %d?)" % device)
        self.device = device
        self._view = None              # struct-of-arrays view of the last batch_run(raw=True): library memory, see consensus()
        self._nbatch = 0
        self.last_call_s = 0.0         # wall time of the last mi355_sw_batch_run_view call itself (batch_run(raw=True))

    def close(self):
        self._view = None
        if self._ctx:
            self._L.mi355_sw_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        self._view = None              # every library call invalidates the memory the last view points into
        if rc:
            raise MI355Error(rc, (self._L.mi355_sw_last_error(self._ctx) or b"").decode())

    def set_option(self, key, value=True):
        """A/B and diagnostic switches of this context (mi355_sw_set_option); none changes a result."""
        v = None if value in (None, False, 0) else ("1" if value is True else str(value))
        self._chk(self._L.mi355_sw_set_option(self._ctx, key.encode(), v.encode() if v is not None else None))

    # -- single alignment ---------------------------------------------------------------------
    def align(self, x, y, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None):
        x, y = _bytes(x), _bytes(y)
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        r = Result()
        self._chk(self._L.mi355_sw_align(self._ctx, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p), C.byref(r)))
        out = _take(r)
        self._L.mi355_sw_free_result(C.byref(r))
        return out

    def argmax(self, x, y, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None):
        x, y = _bytes(x), _bytes(y)
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        ix, iy, mx = C.c_int64(), C.c_int64(), C.c_float()
        self._chk(self._L.mi355_sw_argmax(self._ctx, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p),
                                          C.byref(ix), C.byref(iy), C.byref(mx)))
        return ix.value, iy.value, mx.value

    def fill_matrix(self, x, y, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None):
        x, y = _bytes(x), _bytes(y)
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        H = np.zeros((len(y) + 1, len(x) + 1), dtype=np.float32)
        self._chk(self._L.mi355_sw_fill_matrix(self._ctx, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p),
                                               H.ctypes.data_as(C.POINTER(C.c_float))))
        return H.T

    def align_split(self, x, y, npiece, overlap_ratio, sm_semantics=F32, la_semantics=F32, match=3.0,
                    mismatch=-3.0, gap=2.0, lut=None):
        x, y = _bytes(x), _bytes(y)
        p, keep = make_params(sm_semantics, match, mismatch, gap, lut)
        r = Result()
        piece = C.c_int(0)
        self._chk(self._L.mi355_sw_align_split(self._ctx, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p),
                                               C.c_int(sm_semantics), C.c_int(la_semantics), C.c_int(npiece),
                                               C.c_float(overlap_ratio), C.byref(r), C.byref(piece)))
        out = _take(r)
        out["piece"] = piece.value
        self._L.mi355_sw_free_result(C.byref(r))
        return out

    # -- batches ------------------------------------------------------------------------------
    def set_reference(self, y):
        y = _bytes(y)
        self._chk(self._L.mi355_sw_set_reference(self._ctx, y, C.c_size_t(len(y))))
        self._ref_len = len(y)

    def batch_upload(self, xs):
        xs = [_bytes(x) for x in xs]
        n = len(xs)
        arr = (C.c_char_p * n)(*xs)
        lens = (C.c_size_t * n)(*[len(x) for x in xs])
        self._chk(self._L.mi355_sw_batch_upload(self._ctx, C.c_size_t(n), arr, lens))
        self._nbatch = n

    def batch_upload_packed(self, buf, offsets):
        """The batch as one contiguous buffer (bytes or uint8 array) and n + 1 ascending int64 offsets
        (mi355_sw_batch_upload_packed): no per-sequence Python objects or pointers."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offs) - 1
        if isinstance(buf, np.ndarray):
            arr = np.ascontiguousarray(buf, dtype=np.uint8)
            ptr = arr.ctypes.data_as(C.c_char_p)
        else:
            arr = bytes(buf)
            ptr = C.c_char_p(arr)
        self._chk(self._L.mi355_sw_batch_upload_packed(self._ctx, C.c_size_t(n), ptr, offs.ctypes.data_as(C.POINTER(C.c_int64))))
        self._nbatch = n

    def batch_run(self, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None, flags=0, raw=False):
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        n = self._nbatch
        if raw:
            # struct-of-arrays view in library-owned memory (mi355_sw_batch_run_view): no per-result objects, no
            # per-result allocations on either side; cons=True adds the strings' lengths and addresses
            v = BatchView()
            t0 = time.perf_counter()
            rc = self._L.mi355_sw_batch_run_view(self._ctx, C.byref(p), C.c_int(flags), C.byref(v))
            self.last_call_s = time.perf_counter() - t0            # the C-ABI call alone (what a C / C++ caller waits for)
            self._chk(rc)
            if n == 0:
                return dict(score=np.zeros(0, np.float32), pos=np.zeros(0, np.int64), end_x=np.zeros(0, np.int64),
                            end_y=np.zeros(0, np.int64), cons_len=np.zeros(0, np.int64))
            arr = lambda ptr, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt)   # copies out of library memory
            out = dict(score=arr(v.score, np.float32), pos=arr(v.pos, np.int64), end_x=arr(v.end_x, np.int64),
                       end_y=arr(v.end_y, np.int64), cons_len=arr(v.cons_len, np.int64))
            self._view = v                                             # consensus(k) reads through it until the next call
            return out
        res = (Result * n)()
        self._chk(self._L.mi355_sw_batch_run(self._ctx, C.byref(p), C.c_int(flags), res))
        out = [_take(r) for r in res]
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        return out

    def consensus(self, k):
        """(cons_x, cons_y) of alignment k of the last batch_run(raw=True) (valid until the next call)."""
        v = self._view
        if v is None:
            raise RuntimeError("consensus(k): no batch_run(raw=True) result is current (the view dies with the next call on "
                               "this context, with an empty batch and with close())")
        if not 0 <= k < int(v.n):
            raise IndexError("consensus(%d): the batch has %d alignments" % (k, int(v.n)))
        ln = int(v.cons_len[k])
        if ln == 0:
            return "", ""
        return C.string_at(v.cons_x[k], ln).decode("latin-1"), C.string_at(v.cons_y[k], ln).decode("latin-1")

    def score_ranges(self, ranges, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None):
        """Per-range maxima of every resident query: array [len(ranges), n_queries]."""
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        n = len(ranges)
        lefts = (C.c_int64 * n)(*[r[0] for r in ranges])
        rights = (C.c_int64 * n)(*[r[1] for r in ranges])
        out = np.zeros((n, self._nbatch), dtype=np.float32)
        self._chk(self._L.mi355_sw_score_ranges(self._ctx, C.c_size_t(n), lefts, rights, C.byref(p),
                                                out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def best_range(self, ranges, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None, known_best=0.0, want_exact_above=False):
        """Per resident query the first range with the greatest maximum (mi355_sw_best_range): (best[nq], best_range[nq],
        maxima[len(ranges), nq] — exact for the winners, lower bounds for ranges that cannot win).  want_exact_above=True (the
        multi-rank protocol): a fourth value, the maximum above which this call was exact (-1: everything); the caller merges
        the ranks' bests and calls again with known_best = the merged best when that does not exceed it."""
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        n = len(ranges)
        lefts = (C.c_int64 * max(1, n))(*[r[0] for r in ranges])
        rights = (C.c_int64 * max(1, n))(*[r[1] for r in ranges])
        mx = np.zeros((n, self._nbatch), dtype=np.float32)
        best = np.zeros(self._nbatch, dtype=np.float32)
        which = np.zeros(self._nbatch, dtype=np.int64)
        above = C.c_float(-1.0)
        self._chk(self._L.mi355_sw_best_range(self._ctx, C.c_size_t(n), lefts, rights, C.byref(p), C.c_float(known_best),
                                              mx.ctypes.data_as(C.POINTER(C.c_float)), best.ctypes.data_as(C.POINTER(C.c_float)),
                                              which.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(above) if want_exact_above else None))
        if want_exact_above:
            return best, which, mx, float(above.value)
        return best, which, mx

    def align_scored_range(self, k, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None, flags=0, query=0):
        """Range k of the last score_ranges call finished as a stand-alone problem (argmax + traceback from the sweep's
        keys when the scoring is the same); result of resident query `query`, pos relative to the range start."""
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        n = self._nbatch
        res = (Result * max(1, n))()
        self._chk(self._L.mi355_sw_align_scored_range(self._ctx, C.c_size_t(k), C.byref(p), C.c_int(flags), res))
        out = _take(res[query])
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        return out

    # -- affine gaps: score, end cell, traceback (mi355_sw_affine_*) -------------------------------------
    def affine_align(self, x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
        """One alignment under affine gaps: dict(score, end_x, end_y), the end cell 1-based, 0 / 0 when the score is 0."""
        x, y = _bytes(x), _bytes(y)
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        score, ex, ey = C.c_float(), C.c_int64(), C.c_int64()
        self._chk(self._L.mi355_sw_affine_align(self._ctx, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p),
                                                C.byref(score), C.byref(ex), C.byref(ey)))
        return dict(score=float(score.value), end_x=int(ex.value), end_y=int(ey.value))

    def affine_batch_run(self, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
        """The resident batch against the resident reference under affine gaps: dict of arrays score, end_x, end_y."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        n = self._nbatch
        score = np.zeros(n, dtype=np.float32)
        ex = np.zeros(n, dtype=np.int64)
        ey = np.zeros(n, dtype=np.int64)
        self._chk(self._L.mi355_sw_affine_batch_run(self._ctx, C.byref(p), score.ctypes.data_as(C.POINTER(C.c_float)),
                                                    ex.ctypes.data_as(C.POINTER(C.c_int64)), ey.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(score=score, end_x=ex, end_y=ey)

    def affine_align_trace(self, x, y, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
        """affine_align with the traceback (mi355_sw_affine_align_trace): dict(score, end_x, end_y, begin_x, begin_y, pos, cons_x,
        cons_y, cigar).  cons_x / cons_y are reversed (end cell first), pos == begin_y is the alignment's first column of y,
        begin_x its first row of x (1-based; 0 when the score is 0), cigar the forward run-length string (capi.cigar)."""
        x, y = _bytes(x), _bytes(y)
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        r = Result()
        self._chk(self._L.mi355_sw_affine_align_trace(self._ctx, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p), C.byref(r)))
        out = _take_affine(r)
        self._L.mi355_sw_free_result(C.byref(r))
        return out

    def affine_batch_trace(self, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
        """affine_batch_run with the traceback (mi355_sw_affine_batch_trace): dict of arrays score, end_x, end_y, begin_x, begin_y,
        pos and of lists of strings cons_x, cons_y, cigar, one entry per resident query."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        n = self._nbatch
        res = (Result * max(1, n))()
        self._chk(self._L.mi355_sw_affine_batch_trace(self._ctx, C.byref(p), res))
        rows = [_take_affine(res[k]) for k in range(n)]
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        out = dict(score=np.array([r["score"] for r in rows], dtype=np.float32))
        for k in ("end_x", "end_y", "begin_x", "begin_y", "pos"):
            out[k] = np.array([r[k] for r in rows], dtype=np.int64)
        for k in ("cons_x", "cons_y", "cigar"):
            out[k] = [r[k] for r in rows]
        return out

    def affine_score_ranges(self, ranges, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None):
        """Per-range affine maxima of every resident query: array [len(ranges), n_queries]."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        n = len(ranges)
        lefts = (C.c_int64 * max(1, n))(*[r[0] for r in ranges])
        rights = (C.c_int64 * max(1, n))(*[r[1] for r in ranges])
        out = np.zeros((n, self._nbatch), dtype=np.float32)
        self._chk(self._L.mi355_sw_affine_score_ranges(self._ctx, C.c_size_t(n), lefts, rights, C.byref(p),
                                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    @staticmethod
    def _pair_arrays(query, lefts, rights):
        q = np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        lo = np.ascontiguousarray(lefts, dtype=np.int64).reshape(-1)
        hi = np.ascontiguousarray(rights, dtype=np.int64).reshape(-1)
        if not (len(q) == len(lo) == len(hi)):
            raise ValueError("query, lefts and rights must have the same length")
        return q, lo, hi

    @staticmethod
    def _pair_mode(mode):
        if mode not in AFFINE_MODES:
            raise ValueError("mode must be one of %s" % ", ".join(repr(k) for k in AFFINE_MODES))
        return AFFINE_MODES[mode]

    @staticmethod
    def _pair_bands(band_lo, band_hi, n):
        """(lo, hi) int64 arrays of n bands, or (None, None): each of band_lo / band_hi is an int (every pair) or an array per pair."""
        if band_lo is None and band_hi is None:
            return None, None
        if band_lo is None or band_hi is None:
            raise ValueError("band_lo and band_hi must both be given, or neither")
        out = []
        for b in (band_lo, band_hi):
            a = np.ascontiguousarray(b, dtype=np.int64).reshape(-1)
            if np.ndim(b) == 0:
                a = np.full(n, int(b), dtype=np.int64)
            if len(a) != n:
                raise ValueError("band_lo and band_hi must be ints or hold one value per pair")
            out.append(a)
        return out[0], out[1]

    def _pairs_call(self, name, m, blo, bhi, args):
        """The entry point of a pairs call (name: mi355_sw_affine_pairs_run or _trace; args: npairs, query, lefts, rights, params,
        outputs): `name`_band where bands are given, `name` itself in local mode, `name`_mode otherwise."""
        if blo is not None:
            i64 = C.POINTER(C.c_int64)
            rc = getattr(self._L, name + "_band")(self._ctx, C.c_int(m), *args[:4], blo.ctypes.data_as(i64), bhi.ctypes.data_as(i64), *args[4:])
        elif m == AFFINE_LOCAL:
            rc = getattr(self._L, name)(self._ctx, *args)
        else:
            rc = getattr(self._L, name + "_mode")(self._ctx, C.c_int(m), *args)
        self._chk(rc)

    def affine_pairs_run(self, query, lefts, rights, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mode="local",
                         band_lo=None, band_hi=None):
        """Pair k = resident query query[k] against the window [lefts[k], rights[k]) of the resident reference, each a stand-alone
        problem (mi355_sw_affine_pairs_run): dict of arrays score, end_x, end_y in the caller's order; end_y is relative to the
        window start.  query, lefts, rights: numpy int arrays or lists.  mode="end_to_end" (mi355_sw_affine_pairs_run_mode): the
        whole query against its window, free flanks of the window, a score of any sign; end_x is the query's length.
        band_lo / band_hi (mi355_sw_affine_pairs_run_band; an int or an array per pair): only cells with band_lo <= j - i <= band_hi
        count, i the row and j the column relative to the window start, both 1-based."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        q, lo, hi = self._pair_arrays(query, lefts, rights)
        n = len(q)
        blo, bhi = self._pair_bands(band_lo, band_hi, n)
        score = np.zeros(n, dtype=np.float32)
        ex = np.zeros(n, dtype=np.int64)
        ey = np.zeros(n, dtype=np.int64)
        args = (C.c_size_t(n), q.ctypes.data_as(C.POINTER(C.c_int32)), lo.ctypes.data_as(C.POINTER(C.c_int64)),
                hi.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p), score.ctypes.data_as(C.POINTER(C.c_float)),
                ex.ctypes.data_as(C.POINTER(C.c_int64)), ey.ctypes.data_as(C.POINTER(C.c_int64)))
        self._pairs_call("mi355_sw_affine_pairs_run", self._pair_mode(mode), blo, bhi, args)
        return dict(score=score, end_x=ex, end_y=ey)

    def affine_pairs_trace(self, query, lefts, rights, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, lut=None, mode="local",
                           band_lo=None, band_hi=None):
        """affine_pairs_run with the traceback (mi355_sw_affine_pairs_trace): the dict shape of affine_batch_trace, one entry per pair;
        begin_y / pos are relative to the window start.  mode="end_to_end" (mi355_sw_affine_pairs_trace_mode): begin_x is 1 for
        every pair that has an alignment, whatever the sign of its score.  band_lo / band_hi (mi355_sw_affine_pairs_trace_band): as
        affine_pairs_run; every emitted cell lies in the band."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        q, lo, hi = self._pair_arrays(query, lefts, rights)
        n = len(q)
        blo, bhi = self._pair_bands(band_lo, band_hi, n)
        res = (Result * max(1, n))()
        args = (C.c_size_t(n), q.ctypes.data_as(C.POINTER(C.c_int32)), lo.ctypes.data_as(C.POINTER(C.c_int64)),
                hi.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p), res)
        m = self._pair_mode(mode)
        self._pairs_call("mi355_sw_affine_pairs_trace", m, blo, bhi, args)
        rows = [_take_affine(res[k], m == AFFINE_END_TO_END) for k in range(n)]
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        out = dict(score=np.array([r["score"] for r in rows], dtype=np.float32))
        for k in ("end_x", "end_y", "begin_x", "begin_y", "pos"):
            out[k] = np.array([r[k] for r in rows], dtype=np.int64)
        for k in ("cons_x", "cons_y", "cigar"):
            out[k] = [r[k] for r in rows]
        return out

    @staticmethod
    def _per_pair(v, n, dtype, name):
        """None, or an array of n values of `dtype`: v is a scalar for every pair, or an array per pair."""
        if v is None:
            return None
        a = np.full(n, v, dtype=dtype) if np.ndim(v) == 0 else np.ascontiguousarray(v, dtype=dtype).reshape(-1)
        if len(a) != n:
            raise ValueError("%s must be a scalar or hold one value per pair" % name)
        return a

    def _extend_list(self, query, lefts, rights, q_lo, q_hi, backward):
        """(mi355_sw_extend_list, n, the arrays it points into)."""
        q, lo, hi = self._pair_arrays(query, lefts, rights)
        n = len(q)
        if (q_lo is None) != (q_hi is None):
            raise ValueError("q_lo and q_hi must both be given, or neither")
        ql, qh = self._per_pair(q_lo, n, np.int32, "q_lo"), self._per_pair(q_hi, n, np.int32, "q_hi")
        back = self._per_pair(None if backward is None else np.asarray(backward).astype(bool), n, np.uint8, "backward")
        i32, i64, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        el = ExtendList()
        el.npairs = n
        el.query, el.lefts, el.rights = q.ctypes.data_as(i32), lo.ctypes.data_as(i64), hi.ctypes.data_as(i64)
        if ql is not None:
            el.q_lo, el.q_hi = ql.ctypes.data_as(i32), qh.ctypes.data_as(i32)
        if back is not None:
            el.backward = back.ctypes.data_as(u8)
        return el, n, (q, lo, hi, ql, qh, back)

    def _extend_bands(self, band_lo, band_hi, n):
        """(lo, hi) int64 arrays of n bands, or (None, None): each of band_lo / band_hi is a scalar (every pair) or an array per pair."""
        if (band_lo is None) != (band_hi is None):
            raise ValueError("band_lo and band_hi must both be given, or neither")
        return self._per_pair(band_lo, n, np.int64, "band_lo"), self._per_pair(band_hi, n, np.int64, "band_hi")

    def affine_extend_run(self, query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0,
                          gap_extend=1.0, lut=None, band_lo=None, band_hi=None):
        """Anchored seed extension (mi355_sw_affine_extend_run): pair k = the letters [q_lo[k], q_hi[k]) of resident query query[k]
        (both None: the whole query) against the window [lefts[k], rights[k]) of the resident reference, anchored in front of both;
        backward[k]: anchored behind both, on both strings reversed (the left extension of a seed).  No zero floor, and both flanks
        cost a gap.  Dict of arrays: score (>= 0), end_x, end_y — the best extension, as LENGTHS of query letters and reference
        columns consumed from the anchor — and to_end_score (any sign), to_end_y: the best extension that reaches the query
        range's end.  q_lo, q_hi and backward each take a scalar for every pair, or an array.
        band_lo / band_hi (mi355_sw_affine_extend_run_band; a scalar or an array per pair, band_lo <= 0 <= band_hi): only cells with
        band_lo <= j - i <= band_hi count, i and j the letters and columns consumed from the anchor.  A read end the band cannot
        reach comes back as to_end_score = float("-inf") and to_end_y = -1."""
        return self._extend_run(query, lefts, rights, q_lo, q_hi, backward, match, mismatch, gap_open, gap_extend, lut, band_lo, band_hi)

    def _extend_run(self, query, lefts, rights, q_lo, q_hi, backward, match, mismatch, gap_open, gap_extend, lut, band_lo, band_hi,
                    zdrop=None):
        """affine_extend_run, and with zdrop (not None) affine_extend_zdrop_run: the _zdrop entry point, which also fills rows_done."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        el, n, arrays = self._extend_list(query, lefts, rights, q_lo, q_hi, backward)
        blo, bhi = self._extend_bands(band_lo, band_hi, n)
        score, tscore = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        ex, ey, ty = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        f32, i64 = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        outs = (score.ctypes.data_as(f32), ex.ctypes.data_as(i64), ey.ctypes.data_as(i64), tscore.ctypes.data_as(f32), ty.ctypes.data_as(i64))
        out = dict(score=score, end_x=ex, end_y=ey, to_end_score=tscore, to_end_y=ty)
        if zdrop is not None:
            out["rows_done"] = np.zeros(n, dtype=np.int64)
            self._chk(self._L.mi355_sw_affine_extend_run_zdrop(self._ctx, C.byref(el), None if blo is None else blo.ctypes.data_as(i64),
                                                               None if bhi is None else bhi.ctypes.data_as(i64), C.c_float(zdrop),
                                                               C.byref(p), *outs, out["rows_done"].ctypes.data_as(i64)))
        elif blo is None:
            self._chk(self._L.mi355_sw_affine_extend_run(self._ctx, C.byref(el), C.byref(p), *outs))
        else:
            self._chk(self._L.mi355_sw_affine_extend_run_band(self._ctx, C.byref(el), blo.ctypes.data_as(i64), bhi.ctypes.data_as(i64),
                                                              C.byref(p), *outs))
        return out

    def affine_extend_zdrop_run(self, query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0,
                                gap_extend=1.0, lut=None, band_lo=None, band_hi=None, zdrop=float("inf")):
        """affine_extend_run inside a band under the z-drop stop rule (mi355_sw_affine_extend_run_zdrop): the extension of pair k
        stops after the first row i < m whose in-band maximum r_i falls more than zdrop below the running best B, the gap between
        their diagonals allowed for: B - r_i - d gap_extend > zdrop.  The results are those of affine_extend_run with the same band on
        the first rows_done[k] letters, and a pair that stopped has to_end_score = float("-inf") and to_end_y = -1.  The dict gains
        rows_done (the stop row, or m).  Bands are required; zdrop = inf is affine_extend_run with these bands."""
        return self._extend_run(query, lefts, rights, q_lo, q_hi, backward, match, mismatch, gap_open, gap_extend, lut, band_lo, band_hi,
                                zdrop=float(zdrop))

    def affine_extend_trace(self, query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0,
                            gap_extend=1.0, lut=None, to_end=None, band_lo=None, band_hi=None):
        """affine_extend_run with the traceback (mi355_sw_affine_extend_trace): score, end_x, end_y describe the TRACED alignment —
        the best extension, or where to_end[k] is set (a scalar for every pair, or an array) the one that ends in (m, to_end_y) —
        with pos, cons_x, cons_y and cigar; to_end_score / to_end_y as affine_extend_run.  The strings run from the far end to the
        anchor: reversed for a forward pair, left to right in the original strings for a backward pair.  The CIGAR is in reading
        order for both directions.  band_lo / band_hi (mi355_sw_affine_extend_trace_band): as affine_extend_run; every emitted cell
        lies in the band, and a pair traced to an end the band cannot reach has score float("-inf"), end 0 / 0 and empty strings."""
        return self._extend_trace(query, lefts, rights, q_lo, q_hi, backward, match, mismatch, gap_open, gap_extend, lut, to_end, band_lo, band_hi)

    def affine_extend_zdrop_trace(self, query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0,
                                  gap_extend=1.0, lut=None, to_end=None, band_lo=None, band_hi=None, zdrop=float("inf")):
        """affine_extend_zdrop_run with the traceback (mi355_sw_affine_extend_trace_zdrop): affine_extend_trace's dict and rows_done.
        Every emitted cell lies in the band and in rows <= rows_done; a pair that stopped, traced to_end, is the empty alignment."""
        return self._extend_trace(query, lefts, rights, q_lo, q_hi, backward, match, mismatch, gap_open, gap_extend, lut, to_end, band_lo, band_hi,
                                  zdrop=float(zdrop))

    def _extend_trace(self, query, lefts, rights, q_lo, q_hi, backward, match, mismatch, gap_open, gap_extend, lut, to_end, band_lo, band_hi,
                      zdrop=None):
        """affine_extend_trace, and with zdrop (not None) affine_extend_zdrop_trace."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        el, n, arrays = self._extend_list(query, lefts, rights, q_lo, q_hi, backward)
        blo, bhi = self._extend_bands(band_lo, band_hi, n)
        te = self._per_pair(None if to_end is None else np.asarray(to_end).astype(bool), n, np.uint8, "to_end")
        res = (Result * max(1, n))()
        tscore, ty = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64)
        rows_done = np.zeros(n, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        tail = (te.ctypes.data_as(C.POINTER(C.c_uint8)) if te is not None else None, res,
                tscore.ctypes.data_as(C.POINTER(C.c_float)), ty.ctypes.data_as(i64))
        if zdrop is not None:
            self._chk(self._L.mi355_sw_affine_extend_trace_zdrop(self._ctx, C.byref(el), None if blo is None else blo.ctypes.data_as(i64),
                                                                 None if bhi is None else bhi.ctypes.data_as(i64), C.c_float(zdrop),
                                                                 C.byref(p), *tail, rows_done.ctypes.data_as(i64)))
        elif blo is None:
            self._chk(self._L.mi355_sw_affine_extend_trace(self._ctx, C.byref(el), C.byref(p), *tail))
        else:
            self._chk(self._L.mi355_sw_affine_extend_trace_band(self._ctx, C.byref(el), blo.ctypes.data_as(i64), bhi.ctypes.data_as(i64),
                                                                C.byref(p), *tail))
        back = arrays[5]
        rows = []
        for k in range(n):
            r = _take(res[k])
            b = back is not None and bool(back[k])
            r["cigar"] = cigar(r["cons_x"][::-1], r["cons_y"][::-1]) if b else cigar(r["cons_x"], r["cons_y"])
            rows.append(r)
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        out = dict(score=np.array([r["score"] for r in rows], dtype=np.float32), to_end_score=tscore, to_end_y=ty)
        for k in ("end_x", "end_y", "pos"):
            out[k] = np.array([r[k] for r in rows], dtype=np.int64)
        for k in ("cons_x", "cons_y", "cigar"):
            out[k] = [r[k] for r in rows]
        if zdrop is not None:
            out["rows_done"] = rows_done
        return out

    def affine_global_run(self, query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0,
                          gap_extend=1.0, lut=None, band_lo=None, band_hi=None):
        """Global alignment between two anchors (mi355_sw_affine_global_run): pair k as in affine_extend_run, anchored in front of
        AND behind both strings — the gap fill between two consecutive seeds of a chain.  dict(score=): H(m, n) of the anchored
        model, of any sign.  band_lo / band_hi (a scalar or an array per pair, band_lo <= 0 <= band_hi): only cells with
        band_lo <= j - i <= band_hi count; a band that misses the corner (n - m outside it) gives float("-inf")."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        el, n, arrays = self._extend_list(query, lefts, rights, q_lo, q_hi, backward)
        blo, bhi = self._extend_bands(band_lo, band_hi, n)
        score = np.zeros(n, dtype=np.float32)
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.mi355_sw_affine_global_run(self._ctx, C.byref(el), blo.ctypes.data_as(i64) if blo is not None else None,
                                                     bhi.ctypes.data_as(i64) if bhi is not None else None, C.byref(p),
                                                     score.ctypes.data_as(C.POINTER(C.c_float))))
        return dict(score=score)

    def affine_global_trace(self, query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0,
                            gap_extend=1.0, lut=None, band_lo=None, band_hi=None):
        """affine_global_run with the traceback (mi355_sw_affine_global_trace): score, end_x (= m), end_y (= n), pos, cons_x, cons_y
        and cigar of the walk from (m, n) to the anchor.  The strings hold all of x and all of the window; they run from the far end
        to the anchor, as affine_extend_trace's, and the CIGAR is in reading order for both directions.  A band that misses the
        corner: score float("-inf"), end 0 / 0, pos 0 and empty strings."""
        p, keep = make_affine_params(match, mismatch, gap_open, gap_extend, lut)
        el, n, arrays = self._extend_list(query, lefts, rights, q_lo, q_hi, backward)
        blo, bhi = self._extend_bands(band_lo, band_hi, n)
        res = (Result * max(1, n))()
        i64 = C.POINTER(C.c_int64)
        self._chk(self._L.mi355_sw_affine_global_trace(self._ctx, C.byref(el), blo.ctypes.data_as(i64) if blo is not None else None,
                                                       bhi.ctypes.data_as(i64) if bhi is not None else None, C.byref(p), res))
        back = arrays[5]
        rows = []
        for k in range(n):
            r = _take(res[k])
            b = back is not None and bool(back[k])
            r["cigar"] = cigar(r["cons_x"][::-1], r["cons_y"][::-1]) if b else cigar(r["cons_x"], r["cons_y"])
            rows.append(r)
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        out = dict(score=np.array([r["score"] for r in rows], dtype=np.float32))
        for k in ("end_x", "end_y", "pos"):
            out[k] = np.array([r[k] for r in rows], dtype=np.int64)
        for k in ("cons_x", "cons_y", "cigar"):
            out[k] = [r[k] for r in rows]
        return out

    def align_batch(self, xs, y=None, **kw):
        if y is not None:
            self.set_reference(y)
        self.batch_upload(xs)
        return self.batch_run(**kw)

    def last_timings(self):
        t = (C.c_double * 6)()
        self._L.mi355_sw_last_timings(self._ctx, t)
        return dict(score_us=t[0], locate_us=t[1], trace_us=t[2], total_us=t[3], score_launches=int(t[4]), cells=t[5])


    def last_counters(self):
        """Candidate-filter counters of the last call (mi355_sw_last_counters)."""
        c = (C.c_uint64 * 4)()
        self._L.mi355_sw_last_counters(self._ctx, c)
        out = dict(requeried=int(c[0]), whole_batch_again=int(c[1]), candidates=int(c[2]), left_window=int(c[3]))
        for name in ("first_settled", "saved_locates", "saved_traces", "saved_fallbacks", "walk_widened", "wait_retries", "early_settled", "beyond_f16", "prefix_certified",
                     "prefix_second_pass", "prefix_thinned", "prefix_thin_items", "pooled_loops", "prefix_seeded", "prefix_seed_hits", "prefix_calibrated", "seed_certified",
                     "zdrop_stopped", "zdrop_rows_run", "exact_launches", "trace_launches", "prefix_fill_moved", "prefix_fill_resident"):
            v = C.c_uint64(0)
            rc = self._L.mi355_sw_last_counter(self._ctx, name.encode(), C.byref(v))
            if rc:
                raise MI355Error(rc, "mi355_sw_last_counter(%s)" % name)
            out[name] = int(v.value)
        return out

    def prefix_values(self):
        """Test hook (set_option("prefix_rowp", R), then score_ranges of one range): the sub-chunk values the row-P prefix tiles
        published, array [n_queries, n_sub] in score units, -1 in the rows of queries the hook did not sweep; None without such values."""
        nsub = C.c_size_t(0)
        self._chk(self._L.mi355_sw_prefix_values(self._ctx, None, C.c_size_t(0), C.byref(nsub)))
        if nsub.value == 0:
            return None
        out = np.zeros((self._nbatch, nsub.value), dtype=np.float32)
        self._chk(self._L.mi355_sw_prefix_values(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size), C.byref(nsub)))
        return out

    def prefix_thin_items(self, items, P, left, right, P2=38, sub_len=256, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None):
        """Test hook (set_option("prefix_thin_items", 1)): the thin stage's kernel on items = [(resident query, sub-chunk)] of the range
        [left, right) of the resident reference, as a pass at P rows flags them.  Array [n_items, n_per_item]: the maximum of row P2 over
        the item's own columns inside sub-chunk s - 1 + t, -1 where it has none (mi355_sw_prefix_thin_items)."""
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        flat = np.ascontiguousarray(np.asarray(items, dtype=np.uint32).reshape(-1, 2))
        per = C.c_size_t(0)
        args = (self._ctx, C.c_size_t(len(flat)), flat.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int(P), C.c_int(P2), C.c_int64(sub_len),
                C.c_int64(left), C.c_int64(right), C.byref(p))
        self._chk(self._L.mi355_sw_prefix_thin_items(*args, None, C.c_size_t(0), C.byref(per)))
        out = np.zeros((len(flat), per.value), dtype=np.float32)
        self._chk(self._L.mi355_sw_prefix_thin_items(*args, out.ctypes.data_as(C.POINTER(C.c_float)), C.c_size_t(out.size), C.byref(per)))
        return out

    def seed_hits(self, left, right, k=0):
        """Test hook (mi355_sw_seed_hits): the seed scan over [left, right) of the resident reference for the resident batch, seeds of k
        letters (0: the library's rule).  Returns (k used, counts[n_queries] — exact —, hits): hits[q] = the listed hits of query q, at
        most SEED_HIT_CAP, as sorted (start, offset) pairs with start = position - offset relative to `left`."""
        n = self._nbatch
        counts = np.zeros(n, dtype=np.uint32)
        starts = np.zeros(n * SEED_HIT_CAP, dtype=np.int64)
        offs = np.zeros(n * SEED_HIT_CAP, dtype=np.int32)
        used = C.c_int(0)
        self._chk(self._L.mi355_sw_seed_hits(self._ctx, C.c_int64(left), C.c_int64(right), C.c_int(k), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             starts.ctypes.data_as(C.POINTER(C.c_int64)), offs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(used)))
        hits = []
        for q in range(n):
            c = min(int(counts[q]), SEED_HIT_CAP)
            hits.append(sorted(zip(starts[q * SEED_HIT_CAP:q * SEED_HIT_CAP + c].tolist(), offs[q * SEED_HIT_CAP:q * SEED_HIT_CAP + c].tolist())))
        return used.value, counts, hits

    def last_path(self):
        """Tags of the kernels / pipeline decisions of the last call (mi355_sw_last_path), as a list."""
        return self._L.mi355_sw_last_path(self._ctx).decode().split()

    def last_kernel(self):
        """The sw_score_kernel instance that swept the most cells in the last call (mi355_sw_last_kernel)."""
        k = KernelInfo()
        self._L.mi355_sw_last_kernel(self._ctx, C.byref(k))
        return dict(cell=k.cell, dtype=CELL_NAMES.get(k.cell, "?"), lanes=k.lanes, rows_per_lane=k.rows_per_lane,
                    strips=bool(k.strips), twin=bool(k.twin), chunk_len=k.chunk_len, sub_len=k.sub_len, warm=k.warm,
                    cells=k.cells, valu_ops_per_cell=k.valu_ops_per_cell, name=k.name.decode())


class MultiContext:
    """Several GPUs of one node behind one handle (mi355_sw_multi_*): one engine context and one host thread per
    device inside this process.  devices=None: all visible devices; a device may be listed twice (rehearsal on a
    one-GPU box) unless rccl=True."""

    def __init__(self, devices=None, rccl=False):
        self._L = lib()
        self._m = C.c_void_p()
        n = 0 if devices is None else len(devices)
        arr = (C.c_int * max(1, n))(*(devices or [0]))
        rc = self._L.mi355_sw_multi_create(C.byref(self._m), C.c_int(n), arr if n else None, C.c_int(MULTI_RCCL if rccl else 0))
        if rc:
            raise MI355Error(rc, "mi355_sw_multi_create failed (devices %r, rccl=%r)" % (devices, rccl))
        self.ndev = self._L.mi355_sw_multi_device_count(self._m)
        self.rccl_version = self._L.mi355_sw_multi_rccl_version(self._m)

    def close(self):
        if self._m:
            self._L.mi355_sw_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise MI355Error(rc, (self._L.mi355_sw_multi_last_error(self._m) or b"").decode())

    def set_option(self, key, value=True):
        v = None if value in (None, False, 0) else ("1" if value is True else str(value))
        self._chk(self._L.mi355_sw_multi_set_option(self._m, key.encode(), v.encode() if v is not None else None))

    def align_split(self, x, y, npiece, overlap_ratio, sm_semantics=F32, la_semantics=F32, match=3.0,
                    mismatch=-3.0, gap=2.0, lut=None):
        x, y = _bytes(x), _bytes(y)
        p, keep = make_params(sm_semantics, match, mismatch, gap, lut)
        r = Result()
        piece = C.c_int(0)
        self._chk(self._L.mi355_sw_multi_align_split(self._m, x, C.c_size_t(len(x)), y, C.c_size_t(len(y)), C.byref(p),
                                                     C.c_int(sm_semantics), C.c_int(la_semantics), C.c_int(npiece),
                                                     C.c_float(overlap_ratio), C.byref(r), C.byref(piece)))
        out = _take(r)
        out["piece"] = piece.value
        self._L.mi355_sw_free_result(C.byref(r))
        return out

    def set_reference(self, y):
        y = _bytes(y)
        self._chk(self._L.mi355_sw_multi_set_reference(self._m, y, C.c_size_t(len(y))))

    def align_batch(self, xs, y=None, semantics=F32, match=3.0, mismatch=-3.0, gap=2.0, lut=None, flags=0, raw=False):
        """Returns (results, best_index)."""
        if y is not None:
            self.set_reference(y)
        xs = [_bytes(x) for x in xs]
        n = len(xs)
        arr = (C.c_char_p * max(1, n))(*xs)
        lens = (C.c_size_t * max(1, n))(*[len(x) for x in xs])
        p, keep = make_params(semantics, match, mismatch, gap, lut)
        res = (Result * max(1, n))()
        best = C.c_int64(-1)
        self._chk(self._L.mi355_sw_multi_align_batch(self._m, C.c_size_t(n), arr, lens, C.byref(p), C.c_int(flags), res,
                                                     C.byref(best)))
        if raw:
            v = np.frombuffer(res, dtype=_RESULT_DTYPE, count=n)
            out = dict(score=v["score"].astype(np.float32), pos=v["pos"].astype(np.int64),
                       end_x=v["end_x"].astype(np.int64), end_y=v["end_y"].astype(np.int64))
        else:
            out = [_take(res[k]) for k in range(n)]
        self._L.mi355_sw_free_results(res, C.c_size_t(n))
        return out, best.value

    def last_timings(self):
        t = (C.c_double * 6)()
        self._L.mi355_sw_multi_last_timings(self._m, t)
        return dict(score_us=t[0], locate_us=t[1], trace_us=t[2], total_us=t[3], score_launches=int(t[4]), cells=t[5])


def option_names():
    return lib().mi355_sw_option_names().decode().split(",")


def make_string_range(npiece, shortlen, longlen, ratio):
    lefts = (C.c_int64 * max(1, npiece))()
    rights = (C.c_int64 * max(1, npiece))()
    rc = lib().mi355_sw_make_string_range(C.c_int(npiece), C.c_int64(shortlen), C.c_int64(longlen), C.c_float(ratio),
                                          lefts, rights)
    if rc:
        return None
    return [(int(lefts[k]), int(rights[k])) for k in range(npiece)]


def true2raw(nx, ny, ti, tj):
    ri, rj = C.c_size_t(), C.c_size_t()
    lib().mi355_sw_true2raw(C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(ti), C.c_size_t(tj), C.byref(ri), C.byref(rj))
    return ri.value, rj.value


def raw2true(nx, ny, ri, rj):
    ti, tj = C.c_size_t(), C.c_size_t()
    lib().mi355_sw_raw2true(C.c_size_t(nx), C.c_size_t(ny), C.c_size_t(ri), C.c_size_t(rj), C.byref(ti), C.byref(tj))
    return ti.value, tj.value


def seed_k(letters, min_len, n):
    """mi355_sw_seed_k: the seed length of the seed stage, 0 where it is not used (no device needed)."""
    return int(lib().mi355_sw_seed_k(C.c_int(letters), C.c_int(min_len), C.c_int64(n)))


def seed_hash(codes):
    """mi355_sw_seed_hash: the rolling hash of the code bytes `codes` (no device needed)."""
    a = np.ascontiguousarray(np.frombuffer(bytes(codes), dtype=np.uint8))
    return int(lib().mi355_sw_seed_hash(a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(len(a))))


def seed_usable(read, k, letters=b"ACGT"):
    """mi355_sw_seed_usable: the seeds of `read` (k letters at offsets 0, k, 2k, ...) that enter the seed table — every letter among
    `letters`, not periodic (no device needed)."""
    x = np.ascontiguousarray(np.frombuffer(bytes(read), dtype=np.uint8))
    a = np.ascontiguousarray(np.frombuffer(bytes(letters), dtype=np.uint8))
    rc = lib().mi355_sw_seed_usable(x.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int32(len(x)), C.c_int(k),
                                    a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(len(a)))
    if rc < 0:
        raise MI355Error(rc, "mi355_sw_seed_usable")
    return int(rc)


def seed_certify_ok(d, smax, g, u):
    """mi355_sw_seed_certify_ok: does a read of deficit d with u seeds in the table keep an intact seed in every alignment of score
    >= B0?"""
    return bool(lib().mi355_sw_seed_certify_ok(C.c_int64(d), C.c_int64(smax), C.c_int64(g), C.c_int64(u)))


def seed_certify_window(start, m, d, smax, g, n):
    """mi355_sw_seed_certify_window: (lo, hi), the 0-based end columns inside [0, n) that L21 leaves to the hit `start`, or None."""
    lo, hi = C.c_int64(0), C.c_int64(0)
    rc = lib().mi355_sw_seed_certify_window(C.c_int64(start), C.c_int64(m), C.c_int64(d), C.c_int64(smax), C.c_int64(g), C.c_int64(n),
                                            C.byref(lo), C.byref(hi))
    if rc < 0:
        raise MI355Error(rc, "mi355_sw_seed_certify_window")
    return (lo.value, hi.value) if rc == 1 else None


def prefix_group_tile_len(pairs, cols, sub_len, warm, lanes, cus, resident, old_len, f0=0.0, cap=0.0):
    """mi355_sw_prefix_group_tile_len: the tile length of a seeded group's pass by the launch's fill (no device needed).
    f0 / cap of 0: the library's constants (prefix_fill_constants)."""
    return int(lib().mi355_sw_prefix_group_tile_len(C.c_int64(pairs), C.c_int64(cols), C.c_int64(sub_len), C.c_int64(warm), C.c_int(lanes),
                                                    C.c_int(cus), C.c_int(resident), C.c_int64(old_len), C.c_double(f0), C.c_double(cap)))


def prefix_fill_constants():
    """mi355_sw_prefix_fill_constants: (f0, cap, gain) — what a partly filled round costs, the redundancy cap, the switching threshold."""
    f0, cap, gain = C.c_double(0), C.c_double(0), C.c_double(0)
    lib().mi355_sw_prefix_fill_constants(C.byref(f0), C.byref(cap), C.byref(gain))
    return f0.value, cap.value, gain.value


def seed_cluster(hits, width):
    """mi355_sw_seed_cluster on hits = [(start, offset)]: (lowest start, highest start, distinct offsets) of the winning cluster, or
    None without hits (no device needed)."""
    starts = np.ascontiguousarray([h[0] for h in hits], dtype=np.int64)
    offs = np.ascontiguousarray([h[1] for h in hits], dtype=np.int32)
    lo, hi, d = C.c_int64(0), C.c_int64(0), C.c_int(0)
    rc = lib().mi355_sw_seed_cluster(C.c_size_t(len(starts)), starts.ctypes.data_as(C.POINTER(C.c_int64)), offs.ctypes.data_as(C.POINTER(C.c_int32)),
                                     C.c_int64(width), C.byref(lo), C.byref(hi), C.byref(d))
    if rc < 0:
        raise MI355Error(rc, "mi355_sw_seed_cluster")
    return (lo.value, hi.value, d.value) if rc == 1 else None
