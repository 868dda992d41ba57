"""Host-side mirror of the reference's aligner interface (src/aligner/localaligner.h:7-28,
smithwaterman.h:11-58, plocalaligner.h:6-33) on top of the C-ABI: same class and method names,
same argument meaning, same defaults, same error behaviour where the reference defines one.

    la = SWAligner(first, second)                 # Similarity_Matrix (float32) semantics
    la = SWAligner(first, second, matrix=Similarity_Matrix_Skewed)
    la.calculateScore(); la.getScore(); la.getPos(); la.getConsensus_x(); la.getConsensus_y()

`first` = rows (the read), `second` = columns (the reference); pos indexes `second`, 1-based.
"""
import numpy as np

from . import capi


class Similarity_Matrix:            # tag types mirroring similaritymatrix.h:26-62
    semantics = capi.F32


class Similarity_Matrix_Skewed:     # similaritymatrix.h:64-100
    semantics = capi.U8SAT


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = capi.Context(device)
    return _default_ctx[device]


def _lut_from_function(fn):
    lut = np.empty((256, 256), dtype=np.float32)
    for a in range(256):
        ca = chr(a)
        for b in range(256):
            lut[a, b] = fn(ca, chr(b))
    return lut


class LocalAligner:
    """localaligner.h:7-17"""

    def calculateScore(self): raise NotImplementedError
    def getScore(self): raise NotImplementedError
    def getPos(self): raise NotImplementedError
    def getConsensus_x(self): raise NotImplementedError
    def getConsensus_y(self): raise NotImplementedError
    def getTimings(self): raise NotImplementedError


class SWAligner(LocalAligner):
    """smithwaterman.h:11-58.  `scoring` is either None (3 / -3), a callable f(a, b) -> float (tabulated
    once into a 256x256 table, the way the GPU consumes std::function scoring), or a 256x256 array."""

    def __init__(self, first_sequence, second_sequence, scoring=None, gap_penalty=2.0, matrix=Similarity_Matrix,
                 context=None):
        self.sequence_x, self.sequence_y = first_sequence, second_sequence
        self.gap_penalty = float(gap_penalty)
        self.matrix = matrix
        self._lut = None
        if scoring is not None:
            self._lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        self._ctx = context
        self.pos, self.max_score = 0, -1.0          # smithwaterman.cpp:27-28
        self.consensus_x, self.consensus_y = "", ""
        self._timings = (0.0, 0.0)
        self._end = (0, 0)

    def _context(self):
        return self._ctx if self._ctx is not None else default_context()

    def calculateScore(self):
        r = self._context().align(self.sequence_x, self.sequence_y, self.matrix.semantics, gap=self.gap_penalty,
                                  lut=self._lut)
        self.max_score, self.pos = r["score"], r["pos"]
        self.consensus_x, self.consensus_y = r["cons_x"], r["cons_y"]
        self._timings, self._end = r["timings_us"], (r["end_x"], r["end_y"])
        return self.max_score

    def getScore(self): return self.max_score
    def getPos(self): return self.pos
    def getConsensus_x(self): return self.consensus_x
    def getConsensus_y(self): return self.consensus_y
    def getTimings(self): return self._timings

    def getSimilarity_matrix(self):
        """Matrix accessor (operator()(row, col)): the full matrix recomputed on the device."""
        return self._context().fill_matrix(self.sequence_x, self.sequence_y, self.matrix.semantics,
                                           gap=self.gap_penalty, lut=self._lut)

    def find_index_of_maximum(self):
        return self._context().argmax(self.sequence_x, self.sequence_y, self.matrix.semantics, gap=self.gap_penalty,
                                      lut=self._lut)


class AffineSWAligner:
    """Score and end cell under affine gaps (mi355_sw_affine_align; no counterpart in the reference, whose gap is linear): a gap
    of k letters costs gap_open + (k - 1) * gap_extend.  `scoring` as for SWAligner.  traceback=True: calculateScore also walks
    the alignment back (mi355_sw_affine_align_trace, the rule of include/mi355_sw.h) and getPos / getConsensus_x / getConsensus_y
    (reversed strings, as SWAligner's) / getBegin / getCigar return it."""

    def __init__(self, first_sequence, second_sequence, scoring=None, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0,
                 context=None, traceback=False):
        self.sequence_x, self.sequence_y = first_sequence, second_sequence
        self.match, self.mismatch = float(match), float(mismatch)
        self.gap_open, self.gap_extend = float(gap_open), float(gap_extend)
        self._lut = None
        if scoring is not None:
            self._lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        self._ctx = context
        self.max_score, self._end = -1.0, (0, 0)
        self.traceback = bool(traceback)
        self.pos, self._begin, self._cigar = 0, (0, 0), ""
        self.consensus_x, self.consensus_y = "", ""

    def calculateScore(self):
        ctx = self._ctx if self._ctx is not None else default_context()
        call = ctx.affine_align_trace if self.traceback else ctx.affine_align
        r = call(self.sequence_x, self.sequence_y, match=self.match, mismatch=self.mismatch,
                 gap_open=self.gap_open, gap_extend=self.gap_extend, lut=self._lut)
        self.max_score, self._end = r["score"], (r["end_x"], r["end_y"])
        if self.traceback:
            self.pos, self._begin, self._cigar = r["pos"], (r["begin_x"], r["begin_y"]), r["cigar"]
            self.consensus_x, self.consensus_y = r["cons_x"], r["cons_y"]
        return self.max_score

    def getScore(self): return self.max_score

    def _traced(self):
        if not self.traceback:
            raise RuntimeError("AffineSWAligner was constructed with traceback=False")

    def getPos(self):
        self._traced()
        return self.pos

    def getConsensus_x(self):
        self._traced()
        return self.consensus_x

    def getConsensus_y(self):
        self._traced()
        return self.consensus_y

    def getBegin(self):
        """(row of first_sequence, column of second_sequence) of the alignment's first pair, 1-based; (0, 0) when the score is 0."""
        self._traced()
        return self._begin

    def getCigar(self):
        """Forward run-length string: M letter pair, I letter of first_sequence against a gap, D letter of second_sequence
        against a gap."""
        self._traced()
        return self._cigar

    def getEnd(self):
        """(row of first_sequence, column of second_sequence) of the first maximum in column-major order, 1-based; (0, 0) when
        the score is 0."""
        return self._end

    @staticmethod
    def align_pairs(query, lefts, rights, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0, scoring=None, context=None,
                    traceback=False, end_to_end=False, band=None):
        """The extension stage of a mapper: pair k = query[k] of the context's resident batch against the window
        [lefts[k], rights[k]) of its resident reference, each a stand-alone problem (Context.affine_pairs_run, or
        affine_pairs_trace with traceback=True).  Returns that call's dict of per-pair arrays.  end_to_end=True aligns every
        letter of the query (free flanks of the window, no soft clips, a score of any sign) instead of the best local piece.
        band=(lo, hi), each an int or an array per pair: only cells with lo <= j - i <= hi count (row i, column j relative to the
        window start, 1-based) — the band around a seed's diagonal."""
        ctx = context if context is not None else default_context()
        lut = None
        if scoring is not None:
            lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        call = ctx.affine_pairs_trace if traceback else ctx.affine_pairs_run
        band_lo, band_hi = (None, None) if band is None else band
        return call(query, lefts, rights, match=float(match), mismatch=float(mismatch), gap_open=float(gap_open),
                    gap_extend=float(gap_extend), lut=lut, mode="end_to_end" if end_to_end else "local", band_lo=band_lo, band_hi=band_hi)

    @staticmethod
    def extend_pairs(query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0,
                     scoring=None, context=None, traceback=False, to_end=None, band=None):
        """A mapper's seed extension: pair k = the letters [q_lo[k], q_hi[k]) of query[k] against the window [lefts[k], rights[k]),
        anchored in front of both (backward: behind both, the left extension of a seed, on both strings reversed)
        (Context.affine_extend_run, or affine_extend_trace with traceback=True).  Returns that call's dict: the best extension
        (score >= 0, end_x / end_y as lengths) and the extension to the query's end (to_end_score of any sign, to_end_y).
        q_lo, q_hi, backward and to_end each take a scalar for every pair, or an array; to_end picks the traced alignment.
        band=(lo, hi), lo <= 0 <= hi, each a scalar or an array per pair: extend inside the diagonals lo <= j - i <= hi around the
        anchor's (BWA-MEM's w is (-w, w)); a read end the band cannot reach has to_end_score float("-inf") and to_end_y -1."""
        ctx = context if context is not None else default_context()
        lut = None
        if scoring is not None:
            lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        kw = dict(q_lo=q_lo, q_hi=q_hi, backward=backward, match=float(match), mismatch=float(mismatch), gap_open=float(gap_open),
                  gap_extend=float(gap_extend), lut=lut)
        if band is not None:
            kw["band_lo"], kw["band_hi"] = band
        if traceback:
            return ctx.affine_extend_trace(query, lefts, rights, to_end=to_end, **kw)
        return ctx.affine_extend_run(query, lefts, rights, **kw)

    @staticmethod
    def extend_pairs_zdrop(query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0,
                           scoring=None, context=None, traceback=False, to_end=None, band=None, zdrop=float("inf")):
        """extend_pairs inside a band under a z-drop stop rule (Context.affine_extend_zdrop_run, or affine_extend_zdrop_trace with
        traceback=True): the extension of a pair stops after the first row whose in-band maximum falls more than zdrop below the
        running best (B - r_i - d gap_extend > zdrop, d the distance of the two cells' diagonals), as BWA-MEM's and minimap2's
        extensions do when they run into junk.  band=(lo, hi) is required.  The dict gains rows_done; a pair that stopped has
        to_end_score float("-inf") and to_end_y -1, and its other results are those of extend_pairs on its first rows_done letters."""
        if band is None:
            raise ValueError("extend_pairs_zdrop needs a band: band=(lo, hi)")
        ctx = context if context is not None else default_context()
        lut = None
        if scoring is not None:
            lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        kw = dict(q_lo=q_lo, q_hi=q_hi, backward=backward, match=float(match), mismatch=float(mismatch), gap_open=float(gap_open),
                  gap_extend=float(gap_extend), lut=lut, band_lo=band[0], band_hi=band[1], zdrop=float(zdrop))
        if traceback:
            return ctx.affine_extend_zdrop_trace(query, lefts, rights, to_end=to_end, **kw)
        return ctx.affine_extend_zdrop_run(query, lefts, rights, **kw)

    @staticmethod
    def global_pairs(query, lefts, rights, q_lo=None, q_hi=None, backward=None, match=3.0, mismatch=-3.0, gap_open=5.0, gap_extend=1.0,
                     scoring=None, traceback=False, context=None, band=None):
        """A mapper's gap fill: pair k = the letters [q_lo[k], q_hi[k]) of query[k] against the window [lefts[k], rights[k]), anchored
        at BOTH ends — the alignment between two consecutive seeds of a chain (Context.affine_global_run, or affine_global_trace
        with traceback=True).  Returns that call's dict: score = H(m, n) of any sign, and with traceback end_x = m, end_y = n, pos,
        the strings and the CIGAR.  An empty letter range or an empty window is one gap (or nothing).  band=(lo, hi), lo <= 0 <= hi,
        each a scalar or an array per pair: only the diagonals lo <= j - i <= hi count; a band that does not hold n - m gives score
        float("-inf") and empty strings."""
        ctx = context if context is not None else default_context()
        lut = None
        if scoring is not None:
            lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        kw = dict(q_lo=q_lo, q_hi=q_hi, backward=backward, match=float(match), mismatch=float(mismatch), gap_open=float(gap_open),
                  gap_extend=float(gap_extend), lut=lut)
        if band is not None:
            kw["band_lo"], kw["band_hi"] = band
        if traceback:
            return ctx.affine_global_trace(query, lefts, rights, **kw)
        return ctx.affine_global_run(query, lefts, rights, **kw)


class ParallelLocalAligner:
    """localaligner.h:19-28"""


class OMPParallelLocalAligner(ParallelLocalAligner):
    """plocalaligner.h:6-33: reference split into `npiece` overlapping pieces (overlap =
    overlap_ratio * |first|); the winning piece is re-aligned with DEFAULT scoring by `aligner_matrix`."""

    def __init__(self, first_sequence, second_sequence, npiece, overlap_ratio, scoring=None, gap_penalty=2.0,
                 matrix=Similarity_Matrix, aligner_matrix=None, context=None):
        self.sequence_x, self.sequence_y = first_sequence, second_sequence
        self.npiece, self.overlap_ratio = int(npiece), float(overlap_ratio)
        self.gap_penalty = float(gap_penalty)
        self.matrix = matrix
        self.aligner_matrix = aligner_matrix if aligner_matrix is not None else matrix
        self._lut = None
        if scoring is not None:
            self._lut = _lut_from_function(scoring) if callable(scoring) else np.asarray(scoring, dtype=np.float32)
        self._ctx = context
        self.pos, self.max_score = 0, -1.0          # plocalaligner.cpp:78-79
        self.consensus_x, self.consensus_y = "", ""
        self._timings = (0.0, 0.0)
        self.winning_piece = 0
        # the reference asserts in its constructor (plocalaligner.cpp:52,63,65)
        if capi.make_string_range(self.npiece, len(first_sequence), len(second_sequence), self.overlap_ratio) is None:
            raise AssertionError("_make_string_range: overlaplength <= piecelength / right < longstringlength")

    def calculateScore(self):
        ctx = self._ctx if self._ctx is not None else default_context()
        r = ctx.align_split(self.sequence_x, self.sequence_y, self.npiece, self.overlap_ratio,
                            self.matrix.semantics, self.aligner_matrix.semantics, gap=self.gap_penalty, lut=self._lut)
        self.max_score, self.pos = r["score"], r["pos"]
        self.consensus_x, self.consensus_y = r["cons_x"], r["cons_y"]
        self._timings, self.winning_piece = r["timings_us"], r["piece"]
        return self.max_score

    def getScore(self): return self.max_score
    def getPos(self): return self.pos
    def getConsensus_x(self): return self.consensus_x
    def getConsensus_y(self): return self.consensus_y
    def getTimings(self): return self._timings
