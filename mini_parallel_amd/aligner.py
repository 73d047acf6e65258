"""Host-side mirror of the reference's align/score API over the C ABI.

Reference interface (smith_waterman/src/), same names, argument meaning and
error behaviour (errors raise :class:`MswError`, the ``Err(String)`` analogue):

  gpu.rs:9-10        GPU_WORK_GROUP_SIZE, GPU_MAX_WORK_GROUPS
  gpu.rs:17-30       GpuDevice, GpuAlignmentResult
  gpu.rs:33-94       is_gpu_available, get_gpu_devices
  gpu.rs:97-109      get_opencl_context  -> get_context (one Context per GPU)
  aligner.rs:9-15    get_chunk_size_reads
  aligner.rs:365-373 gpu_align_chunk_self
  aligner.rs:410-532 gpu_align            (legacy kernel semantics, K0)

New batched API (north_star): ``Context.align_batch`` (host arrays, pinned
async staging) and ``Context.align_batch_device`` (HBM-resident batches), both
calling the hand-written gfx950 kernels through include/msw.h.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np

from ._lib import (MSW_E_INVALID, MSW_PILEUP_QSUM, AlnT, BatchT, CallParamsT, CallQParamsT, CandT, DeviceInfoT, IndexInfoT, MapqT, MswError, OutT, PileupSummaryT,
                   ReadBatchT, ScoringT, SeedAltT, SeedOutT, SeedParamsT, StatsT, TraceT, check, lib)

GPU_WORK_GROUP_SIZE = 1024          # gpu.rs:9
GPU_MAX_WORK_GROUPS = 1_000_000     # gpu.rs:10


@dataclass
class GpuDevice:
    """gpu.rs:17-22, plus the HIP ordinal / CU count / arch."""
    name: str
    memory_gb: float
    max_work_group_size: int
    ordinal: int = 0
    cu_count: int = 0
    arch: str = ""


@dataclass
class GpuAlignmentResult:
    """gpu.rs:25-30."""
    score: int
    processing_time_ms: float
    gpu_device: str


@dataclass(frozen=True)
class Scoring:
    """Scoring scheme (include/msw.h msw_scoring_t).

    Reference constants: match +2, mismatch -1, linear gap 2
    (smith_waterman.cl:5-7).  Affine: a gap of length k costs
    gap_open + k * gap_extend."""
    match: int = 2
    mismatch: int = -1
    gap_open: int = 0
    gap_extend: int = 2
    affine: bool = False
    want_coords: bool = False

    def to_c(self) -> ScoringT:
        return ScoringT(self.match, self.mismatch, self.gap_open, self.gap_extend,
                        1 if self.affine else 0, 1 if self.want_coords else 0)


LINEAR = Scoring()                                             # config 2
LINEAR_COORDS = Scoring(want_coords=True)
AFFINE = Scoring(gap_open=3, gap_extend=1, affine=True, want_coords=True)   # config 3


def is_gpu_available() -> bool:
    """gpu.rs:33-45."""
    try:
        n = ctypes.c_int(0)
        return lib().msw_device_count(ctypes.byref(n)) == 0 and n.value > 0
    except MswError:
        return False


def get_gpu_devices() -> list:
    """gpu.rs:48-94 (memory from hipMemGetInfo instead of nvidia-smi)."""
    n = ctypes.c_int(0)
    check(lib().msw_device_count(ctypes.byref(n)))
    out = []
    for i in range(n.value):
        info = DeviceInfoT()
        check(lib().msw_device_info(i, ctypes.byref(info)))
        out.append(GpuDevice(name=info.name.decode(), memory_gb=info.mem_bytes / 2**30,
                             max_work_group_size=int(info.max_wg), ordinal=i,
                             cu_count=int(info.cu_count), arch=info.arch.decode()))
    return out


_PTRS: dict = {}


def _ptr(a) -> int:
    """Data address of a numpy array.  ``a.ctypes.data`` costs ~2 us a call
    (a ctypes view object per call), a sizeable share of a 10k-pair async
    call, so the address is remembered per live array: keyed on id(), checked
    by a weak reference and the shape (an in-place resize changes the shape),
    dropped when the array is freed."""
    if a is None:
        return 0
    k = id(a)
    e = _PTRS.get(k)
    if e is not None and e[0]() is a and e[2] == a.shape:
        return e[1]
    p = a.ctypes.data
    try:
        _PTRS[k] = (weakref.ref(a, lambda _r, k=k: _PTRS.pop(k, None)), p, a.shape)
    except TypeError:  # not weak-referenceable: no caching
        pass
    return p


_SCORING_C: dict = {}


def _scoring_c(scoring: "Scoring"):
    """The C struct of a (frozen, hashable) Scoring, built once."""
    c = _SCORING_C.get(scoring)
    if c is None:
        c = _SCORING_C[scoring] = scoring.to_c()
    return c


def _outputs(n: int, coords: bool):
    """Result arrays of an n-pair call in ONE allocation (score int32, then
    end_i / end_j int16 when coords): one address lookup instead of three.
    Every element is written by the library before the call returns (or
    before wait()), so the buffer is not zeroed."""
    if not coords:
        score = np.empty(n, np.int32)
        return (score, None, None), OutT(_fresh_ptr(score), 0, 0)
    buf = np.empty(8 * n, np.uint8)
    base = _fresh_ptr(buf)
    score, ei, ej = buf[:4 * n].view(np.int32), buf[4 * n:6 * n].view(np.int16), buf[6 * n:].view(np.int16)
    return (score, ei, ej), OutT(base, base + 4 * n, base + 6 * n)


def _fresh_ptr(a) -> int:
    """Address of a just-allocated (writable, contiguous) array: through the
    buffer protocol, ~3x cheaper than a.ctypes.data."""
    return ctypes.addressof(ctypes.c_char.from_buffer(a)) if a.size else 0


# One variant record (msw_variant_t of include/msw.h, "Variants"): 48 bytes, the
# same in memory and in the .var file.
VARIANT_DTYPE = np.dtype([("pos", "<u8"), ("depth", "<u4"), ("ref_count", "<u4"), ("alt_count", "<u4"),
                          ("qual", "<u4"), ("pl", "<u4", (3,)), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"),
                          ("gt", "u1"), ("gq", "u1"), ("pad", "u1", (7,))])
assert VARIANT_DTYPE.itemsize == 48
VAR_SNV, VAR_DEL, VAR_INS = 0, 1, 2


@dataclass(frozen=True)
class CallParams:
    """The caller's thresholds, costs and priors (msw_call_params_t; the
    defaults are msw_call_params_default's)."""
    min_depth: int = 4
    min_alt: int = 2
    min_alt_permille: int = 200
    min_qual: int = 20
    q_hit: int = 4
    q_miss: int = 2477
    q_het: int = 304
    prior_het: int = 3000
    prior_hom: int = 3301

    FIELDS = ("min_depth", "min_alt", "min_alt_permille", "min_qual", "q_hit", "q_miss", "q_het", "prior_het",
              "prior_hom")

    def to_c(self) -> CallParamsT:
        for k in self.FIELDS:
            if not 0 <= int(getattr(self, k)) <= 0xFFFFFFFF:
                raise MswError(MSW_E_INVALID, f"call params: {k} does not fit 32 bits")
        return CallParamsT(*(int(getattr(self, k)) for k in self.FIELDS))


@dataclass(frozen=True)
class QualParams:
    """The weights of the quality-weighted caller (msw_call_qparams_t): an
    observation of Phred value Q costs ``q_scale * Q + q_third`` under the
    other homozygote."""
    q_scale: int = 100
    q_third: int = 477

    FIELDS = ("q_scale", "q_third")

    def to_c(self) -> CallQParamsT:
        for k in self.FIELDS:
            if not 0 <= int(getattr(self, k)) <= 0xFFFFFFFF:
                raise MswError(MSW_E_INVALID, f"call qparams: {k} does not fit 32 bits")
        return CallQParamsT(int(self.q_scale), int(self.q_third))


class Variants(NamedTuple):
    """Variant records as arrays, one entry per record, ordered by pos, then
    kind (0 SNV, 1 DEL, 2 INS).  ``ref`` is the genome byte, ``alt`` the base
    letter of an SNV and 0 otherwise, ``gt`` 1 for 0/1 and 2 for 1/1."""
    pos: np.ndarray        # uint64
    kind: np.ndarray       # uint8
    ref: np.ndarray        # uint8
    alt: np.ndarray        # uint8
    gt: np.ndarray         # uint8
    gq: np.ndarray         # uint8
    qual: np.ndarray       # uint32
    depth: np.ndarray      # uint32
    ref_count: np.ndarray  # uint32
    alt_count: np.ndarray  # uint32
    pl: np.ndarray         # uint32 [n][3]

    @classmethod
    def from_records(cls, rec: np.ndarray) -> "Variants":
        return cls(*(np.ascontiguousarray(rec[k]) for k in cls._fields))

    def to_records(self) -> np.ndarray:
        rec = np.zeros(len(self.pos), VARIANT_DTYPE)
        for k in self._fields:
            rec[k] = getattr(self, k)
        return rec


class Context:
    """One GPU: compute + copy streams and double-buffered pinned staging
    (replaces the (Context, Queue, Device) singleton of gpu.rs:13-14)."""

    def __init__(self, ordinal: int = 0):
        self.ordinal = ordinal
        h = ctypes.c_void_p()
        check(lib().msw_ctx_create(ordinal, ctypes.byref(h)))
        self._h = h

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise MswError(MSW_E_INVALID, "context is closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().msw_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batched scoring from host memory --------------------------------------------
    def align_batch(self, reads: np.ndarray, read_len: np.ndarray, wins: np.ndarray,
                    win_len: np.ndarray, scoring: Scoring = LINEAR, chunk_pairs: int = 0,
                    asynchronous: bool = False):
        """Score a padded SoA batch (uint8 [B, stride] reads / windows, uint16
        lengths).  Returns (score int32[B], end_i int16[B], end_j int16[B]);
        the coordinates are None unless ``scoring.want_coords``.  With
        ``asynchronous`` (msw_align_batch_async) it returns a :class:`Pending`
        whose ``wait()`` gives the same tuple."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        wins = np.ascontiguousarray(wins, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        win_len = np.ascontiguousarray(win_len, dtype=np.uint16)
        B = reads.shape[0]
        if wins.shape[0] != B or read_len.shape[0] != B or win_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of pairs")
        (score, ei, ej), out = _outputs(B, scoring.want_coords)
        batch = BatchT(_ptr(reads), _ptr(wins), _ptr(read_len), _ptr(win_len),
                       reads.shape[1] if reads.ndim == 2 else 0,
                       wins.shape[1] if wins.ndim == 2 else 0, B)
        sc = _scoring_c(scoring)
        if asynchronous:
            t = ctypes.c_uint64(0)
            check(lib().msw_align_batch_async(self.handle, ctypes.byref(sc), ctypes.byref(batch),
                                              ctypes.byref(out), chunk_pairs, ctypes.byref(t)))
            return Pending(self, t.value, (score, ei, ej), (reads, wins, read_len, win_len))
        check(lib().msw_align_batch(self.handle, ctypes.byref(sc), ctypes.byref(batch),
                                    ctypes.byref(out), chunk_pairs))
        return score, ei, ej

    # -- full alignments: traceback ----------------------------------------------------
    def align_batch_trace(self, reads: np.ndarray, read_len: np.ndarray, wins: np.ndarray,
                          win_len: np.ndarray, scoring: Scoring = LINEAR,
                          cigar_stride: Optional[int] = None, chunk_pairs: int = 0):
        """Score a padded SoA batch and trace every pair's canonical alignment
        (msw_align_batch_trace; include/msw.h states the rule).  Returns
        (score int32[B], end_i, end_j, start_i, start_j int16[B], ops): ops[p]
        is a uint32 array of BAM-encoded ops (len << 4 | op, M=0 I=1 D=2) in
        forward order, empty when the score is 0.  Coordinates are always
        computed.  With ``cigar_stride=None`` a stride is picked and the call
        is repeated once with the largest count if a pair overflowed; with a
        given stride an overflowing pair's ops are None.  ``ops.n_cigar``
        holds every pair's op count either way.  Reads over 384 or windows
        over 4096 bases raise :class:`MswError` (MSW_E_RANGE)."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        wins = np.ascontiguousarray(wins, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        win_len = np.ascontiguousarray(win_len, dtype=np.uint16)
        B = reads.shape[0]
        if wins.shape[0] != B or read_len.shape[0] != B or win_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of pairs")
        batch = BatchT(_ptr(reads), _ptr(wins), _ptr(read_len), _ptr(win_len),
                       reads.shape[1] if reads.ndim == 2 else 0,
                       wins.shape[1] if wins.ndim == 2 else 0, B)
        sc = _scoring_c(scoring)
        stride = 32 if cigar_stride is None else int(cigar_stride)
        while True:
            (score, ei, ej), out = _outputs(B, True)
            si, sj = np.empty(B, np.int16), np.empty(B, np.int16)
            nc = np.zeros(B, np.int32)
            cig = np.zeros((B, stride), np.uint32)
            tr = TraceT(_fresh_ptr(si), _fresh_ptr(sj), _fresh_ptr(nc), _fresh_ptr(cig), stride)
            check(lib().msw_align_batch_trace(self.handle, ctypes.byref(sc), ctypes.byref(batch),
                                              ctypes.byref(out), ctypes.byref(tr), chunk_pairs))
            need = int(nc.max()) if B else 0
            if cigar_stride is None and need > stride:
                stride = need  # once: the counts do not depend on the stride
                continue
            break
        ops = CigarList(cig[p, :nc[p]].copy() if nc[p] <= stride else None for p in range(B))
        ops.n_cigar = nc
        return score, ei, ej, si, sj, ops

    def trace_batch_device(self, reads_ptr: int, read_len_ptr: int, wins_ptr: int, win_len_ptr: int,
                           read_stride: int, win_stride: int, n_pairs: int, score_ptr: int,
                           end_i_ptr: int, end_j_ptr: int, start_i_ptr: int, start_j_ptr: int,
                           n_cigar_ptr: int, cigar_ptr: int, cigar_stride: int, max_read_len: int,
                           max_win_len: int, scoring: Scoring = LINEAR, stream: int = 0) -> None:
        """Enqueue one traceback pass over device-resident arrays (raw device
        pointers) on ``stream``: score / end_i / end_j are the outputs of
        :meth:`align_batch_device` with coordinates for the same batch and
        scheme (msw_trace_batch_device)."""
        batch = BatchT(reads_ptr, wins_ptr, read_len_ptr, win_len_ptr, read_stride, win_stride, n_pairs)
        ends = OutT(score_ptr, end_i_ptr, end_j_ptr)
        tr = TraceT(start_i_ptr, start_j_ptr, n_cigar_ptr, cigar_ptr, cigar_stride)
        sc = _scoring_c(scoring)
        check(lib().msw_trace_batch_device(self.handle, ctypes.byref(sc), ctypes.byref(batch),
                                           ctypes.byref(ends), ctypes.byref(tr), max_read_len, max_win_len,
                                           ctypes.c_void_p(stream or None)))

    # -- reads against an HBM-resident genome ------------------------------------------
    def load_genome(self, seq) -> "Genome":
        """Upload a reference genome (bytes / str / uint8 array) once; windows
        are then cut on the GPU (msw_genome_create)."""
        return Genome(self, seq)

    def align_reads(self, genome: "Genome", reads: np.ndarray, read_len: np.ndarray,
                    win_pos: np.ndarray, win_len: np.ndarray, scoring: Scoring = LINEAR,
                    chunk_pairs: int = 0, asynchronous: bool = False):
        """Score read p against genome[win_pos[p] : win_pos[p] + win_len[p]]
        (clipped at the genome end; positions outside it score 0).  Returns
        (score, end_i, end_j) like :meth:`align_batch` (a :class:`Pending`
        with ``asynchronous``, msw_align_reads_async)."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        win_pos = np.ascontiguousarray(win_pos, dtype=np.int64)
        win_len = np.ascontiguousarray(win_len, dtype=np.uint16)
        B = reads.shape[0]
        if read_len.shape[0] != B or win_pos.shape[0] != B or win_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of pairs")
        (score, ei, ej), out = _outputs(B, scoring.want_coords)
        batch = ReadBatchT(_ptr(reads), _ptr(read_len), reads.shape[1] if reads.ndim == 2 else 0,
                           _ptr(win_pos), _ptr(win_len), B)
        sc = _scoring_c(scoring)
        if asynchronous:
            t = ctypes.c_uint64(0)
            check(lib().msw_align_reads_async(self.handle, ctypes.byref(sc), genome.handle,
                                              ctypes.byref(batch), ctypes.byref(out), chunk_pairs,
                                              ctypes.byref(t)))
            return Pending(self, t.value, (score, ei, ej), (reads, read_len, win_pos, win_len, genome))
        check(lib().msw_align_reads(self.handle, ctypes.byref(sc), genome.handle, ctypes.byref(batch),
                                    ctypes.byref(out), chunk_pairs))
        return score, ei, ej

    # -- alignment records: reads against the genome, traced and packed ----------------
    def align_reads_trace(self, genome: "Genome", reads: np.ndarray, read_len: np.ndarray,
                          win_pos: np.ndarray, win_len: np.ndarray, scoring: Scoring = LINEAR,
                          chunk_pairs: int = 0, cigar_cap: Optional[int] = None):
        """Score read p against genome[win_pos[p] : win_pos[p] + win_len[p]]
        like :meth:`align_reads` and trace it (msw_align_reads_trace).  Returns
        (score, end_i, end_j, ref_pos int64[B], nm int32[B], cigars):
        ``ref_pos`` is the genome coordinate of the first aligned base (-1
        when the score is 0), ``nm`` the edit distance, ``cigars[p]`` a uint32
        array of BAM-encoded ops with soft clips (S = 4), so that it consumes
        the whole read; ``cigars.n_cigar`` holds the op counts.  ``cigar_cap``
        is the first guess at the total number of ops (default 4 per read);
        when it is too small the call is repeated once with the exact size."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        win_pos = np.ascontiguousarray(win_pos, dtype=np.int64)
        win_len = np.ascontiguousarray(win_len, dtype=np.uint16)
        B = reads.shape[0]
        if read_len.shape[0] != B or win_pos.shape[0] != B or win_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of pairs")
        batch = ReadBatchT(_ptr(reads), _ptr(read_len), reads.shape[1] if reads.ndim == 2 else 0,
                           _ptr(win_pos), _ptr(win_len), B)
        sc = _scoring_c(scoring)
        cap = 4 * B if cigar_cap is None else int(cigar_cap)
        while True:
            (score, ei, ej), out = _outputs(B, True)
            ref_pos, nm = np.empty(B, np.int64), np.empty(B, np.int32)
            off = np.zeros(B + 1, np.uint32)
            cig = np.zeros(max(cap, 1), np.uint32)
            ovf = np.zeros(1, np.uint32)
            aln = AlnT(_fresh_ptr(ref_pos), _fresh_ptr(nm), _fresh_ptr(off), _fresh_ptr(cig), cap, _fresh_ptr(ovf))
            check(lib().msw_align_reads_trace(self.handle, ctypes.byref(sc), genome.handle, ctypes.byref(batch),
                                              ctypes.byref(out), ctypes.byref(aln), chunk_pairs))
            total = int(off[B])
            if total > cap:
                cap = total  # once: the offsets do not depend on the capacity
                continue
            break
        cigars = CigarList(cig[off[p]:off[p + 1]].copy() for p in range(B))
        cigars.n_cigar = np.diff(off.astype(np.int64)).astype(np.int32)
        return score, ei, ej, ref_pos, nm, cigars

    def trace_reads_device(self, genome: "Genome", reads_ptr: int, read_len_ptr: int, read_stride: int,
                           win_pos_ptr: int, n: int, window: int, max_read_len: int, score_ptr: int,
                           end_i_ptr: int, end_j_ptr: int, start_i_ptr: int, start_j_ptr: int,
                           n_cigar_ptr: int, cigar_ptr: int, cigar_stride: int, scoring: Scoring = LINEAR,
                           stream: int = 0) -> None:
        """Enqueue one traceback pass over device-resident reads against
        windows read straight from the genome (msw_trace_reads_device): the
        arguments of msw_align_reads_device, whose outputs with coordinates
        are score / end_i / end_j."""
        ends = OutT(score_ptr, end_i_ptr, end_j_ptr)
        tr = TraceT(start_i_ptr, start_j_ptr, n_cigar_ptr, cigar_ptr, cigar_stride)
        sc = _scoring_c(scoring)
        check(lib().msw_trace_reads_device(self.handle, ctypes.byref(sc), genome.handle, ctypes.c_void_p(reads_ptr),
                                           ctypes.c_void_p(read_len_ptr), read_stride, ctypes.c_void_p(win_pos_ptr),
                                           n, window, max_read_len, ctypes.byref(ends), ctypes.byref(tr),
                                           ctypes.c_void_p(stream or None)))

    def aln_pack_device(self, genome: "Genome", reads_ptr: int, read_len_ptr: int, read_stride: int,
                        win_pos_ptr: int, n: int, score_ptr: int, end_i_ptr: int, end_j_ptr: int,
                        start_i_ptr: int, start_j_ptr: int, n_cigar_ptr: int, cigar_ptr: int, cigar_stride: int,
                        ref_pos_ptr: int, nm_ptr: int, cigar_off_ptr: int, packed_ptr: int, cigar_cap: int,
                        n_overflow_ptr: int, stream: int = 0) -> None:
        """Enqueue the alignment records of a traced device-resident batch
        (msw_aln_pack_device): ref_pos, nm, the offsets and the packed,
        soft-clipped ops."""
        ends = OutT(score_ptr, end_i_ptr, end_j_ptr)
        tr = TraceT(start_i_ptr, start_j_ptr, n_cigar_ptr, cigar_ptr, cigar_stride)
        aln = AlnT(ref_pos_ptr, nm_ptr, cigar_off_ptr, packed_ptr or None, cigar_cap, n_overflow_ptr)
        check(lib().msw_aln_pack_device(self.handle, genome.handle, ctypes.c_void_p(reads_ptr),
                                        ctypes.c_void_p(read_len_ptr), read_stride, ctypes.c_void_p(win_pos_ptr), n,
                                        ctypes.byref(ends), ctypes.byref(tr), ctypes.byref(aln),
                                        ctypes.c_void_p(stream or None)))

    # -- both strands (include/msw.h, "Both strands") -----------------------------------
    def revcomp_device(self, reads_ptr: int, read_len_ptr: int, read_stride: int, n: int, out_ptr: int,
                       out_stride: int, stream: int = 0) -> None:
        """Enqueue the reverse complement of n device-resident read rows into
        ``out[n][out_stride]``, zero padded (msw_revcomp_device)."""
        check(lib().msw_revcomp_device(self.handle, ctypes.c_void_p(reads_ptr), ctypes.c_void_p(read_len_ptr),
                                       read_stride, n, ctypes.c_void_p(out_ptr), out_stride,
                                       ctypes.c_void_p(stream or None)))

    def align_reads_strands_device(self, genome: "Genome", reads_ptr: int, read_len_ptr: int, read_stride: int,
                                   win_pos_ptr: int, n: int, window: int, max_read_len: int, score_ptr: int,
                                   strand_ptr: int, oriented_ptr: int, oriented_stride: int,
                                   scoring: Scoring = LINEAR, end_i_ptr: int = 0, end_j_ptr: int = 0,
                                   win_len_out_ptr: int = 0, stream: int = 0) -> None:
        """Enqueue both-strand scoring of device-resident reads against their
        genome windows (msw_align_reads_strands_device): the winner's score
        and end cell, the strand byte and the oriented row per read."""
        out = OutT(score_ptr, end_i_ptr or None, end_j_ptr or None)
        sc = _scoring_c(scoring)
        check(lib().msw_align_reads_strands_device(
            self.handle, ctypes.byref(sc), genome.handle, ctypes.c_void_p(reads_ptr), ctypes.c_void_p(read_len_ptr),
            read_stride, ctypes.c_void_p(win_pos_ptr), n, window, max_read_len, ctypes.byref(out),
            ctypes.c_void_p(win_len_out_ptr or None), ctypes.c_void_p(strand_ptr or None),
            ctypes.c_void_p(oriented_ptr or None), oriented_stride, ctypes.c_void_p(stream or None)))

    def align_reads_strands(self, genome: "Genome", reads: np.ndarray, read_len: np.ndarray,
                            win_pos: np.ndarray, win_len: np.ndarray, scoring: Scoring = LINEAR,
                            trace: bool = False, chunk_pairs: int = 0, cigar_cap: Optional[int] = None):
        """:meth:`align_reads` on both strands (msw_align_reads_strands).
        Returns (score, end_i, end_j, strand): the better of the read and its
        reverse complement per read, ``strand`` uint8[B] 1 where the reverse
        complement won (ties: 0); end_i is in the oriented read's coordinates.
        With ``trace`` it also returns ref_pos, nm and cigars as
        :meth:`align_reads_trace` does, for the oriented read (coordinates are
        then always returned), with the same capacity retry."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        win_pos = np.ascontiguousarray(win_pos, dtype=np.int64)
        win_len = np.ascontiguousarray(win_len, dtype=np.uint16)
        B = reads.shape[0]
        if read_len.shape[0] != B or win_pos.shape[0] != B or win_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of pairs")
        batch = ReadBatchT(_ptr(reads), _ptr(read_len), reads.shape[1] if reads.ndim == 2 else 0,
                           _ptr(win_pos), _ptr(win_len), B)
        sc = _scoring_c(scoring)
        strand = np.zeros(B, np.uint8)
        if not trace:
            (score, ei, ej), out = _outputs(B, scoring.want_coords)
            check(lib().msw_align_reads_strands(self.handle, ctypes.byref(sc), genome.handle, ctypes.byref(batch),
                                                ctypes.byref(out), ctypes.c_void_p(_fresh_ptr(strand) or None),
                                                None, chunk_pairs))
            return score, ei, ej, strand
        cap = 4 * B if cigar_cap is None else int(cigar_cap)
        while True:
            (score, ei, ej), out = _outputs(B, True)
            ref_pos, nm = np.empty(B, np.int64), np.empty(B, np.int32)
            off = np.zeros(B + 1, np.uint32)
            cig = np.zeros(max(cap, 1), np.uint32)
            ovf = np.zeros(1, np.uint32)
            aln = AlnT(_fresh_ptr(ref_pos), _fresh_ptr(nm), _fresh_ptr(off), _fresh_ptr(cig), cap, _fresh_ptr(ovf))
            check(lib().msw_align_reads_strands(self.handle, ctypes.byref(sc), genome.handle, ctypes.byref(batch),
                                                ctypes.byref(out), ctypes.c_void_p(_fresh_ptr(strand) or None),
                                                ctypes.byref(aln), chunk_pairs))
            total = int(off[B])
            if total > cap:
                cap = total  # once: the offsets do not depend on the capacity
                continue
            break
        cigars = CigarList(cig[off[p]:off[p + 1]].copy() for p in range(B))
        cigars.n_cigar = np.diff(off.astype(np.int64)).astype(np.int32)
        return score, ei, ej, strand, ref_pos, nm, cigars

    # -- placing reads (include/msw.h, "Placing reads") ---------------------------------
    def build_index(self, genome: "Genome", k: int = 12, max_occ: int = 64) -> "Index":
        """The k-mer index of a resident genome, built on the GPU
        (msw_index_create)."""
        return Index(self, genome, k, max_occ)

    def seed_reads_device(self, index: "Index", reads_ptr: int, read_len_ptr: int, read_stride: int, n: int,
                          max_read_len: int, win_pos_ptr: int, votes_ptr: int, hits_ptr: int, flags_ptr: int,
                          rc_reads_ptr: int = 0, rc_stride: int = 0, band: int = 16, cap: int = 4096,
                          step: int = 1, min_votes: int = 1, window: int = 0, stream: int = 0) -> None:
        """Enqueue the seeding of n device-resident reads (raw device
        pointers) on ``stream`` (msw_seed_reads_device): a window position,
        the votes, the hits and the flags per read.  ``rc_reads_ptr``: the
        reverse complements' rows (:meth:`revcomp_device`), 0 = forward only."""
        sp = SeedParamsT(band, cap, step, min_votes, window)
        out = SeedOutT(win_pos_ptr or None, votes_ptr or None, hits_ptr or None, flags_ptr or None)
        check(lib().msw_seed_reads_device(self.handle, index.handle, ctypes.c_void_p(reads_ptr or None),
                                          ctypes.c_void_p(rc_reads_ptr or None), ctypes.c_void_p(read_len_ptr or None),
                                          read_stride, rc_stride, n, max_read_len, ctypes.byref(sp), ctypes.byref(out),
                                          ctypes.c_void_p(stream or None)))

    def seed_reads(self, index: "Index", reads: np.ndarray, read_len: np.ndarray, both_strands: bool = True,
                   band: int = 16, cap: int = 4096, step: int = 1, min_votes: int = 1, window: int = 0,
                   chunk_reads: int = 0):
        """Place every read of a host batch on the indexed genome
        (msw_seed_reads).  Returns (win_pos int64[B], votes uint32[B], hits
        uint32[B], flags uint8[B]): ``win_pos`` is what the
        reads-against-genome calls take (-1: fewer than ``min_votes`` votes),
        bit 0 of ``flags`` says the reverse complement gathered more votes,
        bit 1 that the read's hits were cut at ``cap``."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        B = reads.shape[0]
        if read_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of reads")
        win_pos, votes = np.empty(B, np.int64), np.empty(B, np.uint32)
        hits, flags = np.empty(B, np.uint32), np.empty(B, np.uint8)
        batch = ReadBatchT(_ptr(reads), _ptr(read_len), reads.shape[1] if reads.ndim == 2 else 0, None, None, B)
        sp = SeedParamsT(band, cap, step, min_votes, window)
        out = SeedOutT(_fresh_ptr(win_pos), _fresh_ptr(votes), _fresh_ptr(hits), _fresh_ptr(flags))
        check(lib().msw_seed_reads(self.handle, index.handle, ctypes.byref(batch), 1 if both_strands else 0,
                                   ctypes.byref(sp), ctypes.byref(out), chunk_reads))
        return win_pos, votes, hits, flags

    def map_reads(self, genome: "Genome", index: "Index", reads: np.ndarray, read_len: np.ndarray,
                  scoring: Scoring = LINEAR, both_strands: bool = True, window: int = 0, band: int = 16,
                  cap: int = 4096, step: int = 1, min_votes: int = 1, chunk_pairs: int = 0, mapq: bool = False,
                  sep: int = 0):
        """Seed, then align with records: :meth:`seed_reads` gives every read
        its window position, and :meth:`align_reads_strands` with ``trace``
        (``both_strands``) or :meth:`align_reads_trace` scores, traces and
        packs it against genome[win_pos : win_pos + W], W = ``window`` or
        twice the read length capped at 4096.  Returns what those return; a
        read that was not placed has score 0 and ref_pos -1.

        ``mapq`` (msw_map_reads): a second candidate locus at least ``sep``
        diagonals away (0 = the window length) is scored too, the better of
        the two becomes the record, and the tuple ends with three more
        arrays: mapq uint8[B] (0..60, an uncalibrated heuristic), sub_score
        int32[B] (the other candidate's score) and cand uint8[B] (1 where the
        second candidate won)."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        if mapq:
            return self._map_reads_mapq(genome, index, reads, read_len, scoring, both_strands, window, band, cap,
                                        step, min_votes, chunk_pairs, sep)
        win_pos, _, _, _ = self.seed_reads(index, reads, read_len, both_strands, band=band, cap=cap, step=step,
                                           min_votes=min_votes, window=window, chunk_reads=chunk_pairs)
        rl = read_len.astype(np.int64)
        win_len = (np.full(rl.shape, window, np.int64) if window else np.minimum(2 * rl, 4096)).astype(np.uint16)
        if both_strands:
            return self.align_reads_strands(genome, reads, read_len, win_pos, win_len, scoring, trace=True,
                                            chunk_pairs=chunk_pairs)
        return self.align_reads_trace(genome, reads, read_len, win_pos, win_len, scoring, chunk_pairs=chunk_pairs)

    # -- pileup (include/msw.h, "Pileup") -----------------------------------------------
    def pileup(self, genome: "Genome", qsum: bool = False) -> "Pileup":
        """An empty pileup over a resident genome (msw_pileup_create): per
        base the allele, deletion, insertion and reverse-strand counts of the
        alignment records added to it.  With ``qsum`` it also carries the
        per-base quality sums (MSW_PILEUP_QSUM): every add then needs
        ``quals``, and :meth:`Pileup.call` can weigh the genotypes by them."""
        return Pileup(self, genome, qsum)

    # -- variants (include/msw.h, "Variants") -------------------------------------------
    def call_variants(self, genome, counts, params: Optional[CallParams] = None, chunk_pos: int = 0, qsums=None,
                      qual_params: Optional[QualParams] = None) -> Variants:
        """Variant calls from any host ``counts[glen][8]`` over the genome bytes
        (msw_call_counts), for example the sum of several pileups.  The rows go
        to the GPU in chunks of ``chunk_pos`` positions (0: about 1 M); the
        records do not depend on it.  With ``qsums[glen][4]`` the genotypes are
        quality-weighted (msw_call_counts_qual; ``qual_params`` None: the
        default weights); ``qual_params`` without ``qsums`` is an error."""
        g = np.frombuffer(bytes(genome), np.uint8) if isinstance(genome, (bytes, bytearray)) else \
            np.ascontiguousarray(genome, dtype=np.uint8)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        if c.ndim != 2 or c.shape[1] != 8 or c.shape[0] != g.shape[0]:
            raise MswError(MSW_E_INVALID, "counts must be [len(genome)][8]")
        q = (params or CallParams()).to_c()
        total = ctypes.c_uint64()
        if qsums is None and qual_params is not None:
            raise MswError(MSW_E_INVALID, "qual_params without qsums")
        if qsums is not None:
            w = np.ascontiguousarray(qsums, dtype=np.uint32)
            if w.ndim != 2 or w.shape[1] != 4 or w.shape[0] != g.shape[0]:
                raise MswError(MSW_E_INVALID, "qsums must be [len(genome)][4]")
            qq = (qual_params or QualParams()).to_c()

        def run(out, cap):
            out_ptr = _fresh_ptr(out) or None if out is not None else None
            if qsums is not None:
                check(lib().msw_call_counts_qual(self.handle, g.ctypes.data if g.size else None, g.shape[0],
                                                 c.ctypes.data if c.size else None, w.ctypes.data if w.size else None,
                                                 ctypes.byref(q), ctypes.byref(qq), chunk_pos, out_ptr, cap,
                                                 ctypes.byref(total)))
            else:
                check(lib().msw_call_counts(self.handle, g.ctypes.data if g.size else None, g.shape[0],
                                            c.ctypes.data if c.size else None, ctypes.byref(q), chunk_pos, out_ptr,
                                            cap, ctypes.byref(total)))
            return int(total.value)

        n = run(None, 0)
        rec = np.zeros(n, VARIANT_DTYPE)
        if n and run(rec, n) != n:
            raise MswError(MSW_E_INVALID, "the counts changed between the two calls")
        return Variants.from_records(rec)

    # -- candidates and mapping quality (include/msw.h) ---------------------------------
    def _map_reads_mapq(self, genome, index, reads, read_len, scoring, both, window, band, cap, step, min_votes,
                        chunk_pairs, sep):
        B = reads.shape[0]
        if read_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of reads")
        batch = ReadBatchT(_ptr(reads), _ptr(read_len), reads.shape[1] if reads.ndim == 2 else 0, None, None, B)
        sc = _scoring_c(scoring)
        sp = SeedParamsT(band, cap, step, min_votes, window)
        strand = np.zeros(B, np.uint8)
        mq, sub, cand = np.zeros(B, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.uint8)
        ccap = 4 * B
        while B:
            (score, ei, ej), out = _outputs(B, True)
            ref_pos, nm = np.empty(B, np.int64), np.empty(B, np.int32)
            off = np.zeros(B + 1, np.uint32)
            cig = np.zeros(max(ccap, 1), np.uint32)
            ovf = np.zeros(1, np.uint32)
            aln = AlnT(_fresh_ptr(ref_pos), _fresh_ptr(nm), _fresh_ptr(off), _fresh_ptr(cig), ccap, _fresh_ptr(ovf))
            mt = MapqT(_fresh_ptr(mq), _fresh_ptr(sub), _fresh_ptr(cand))
            check(lib().msw_map_reads(self.handle, ctypes.byref(sc), genome.handle, index.handle, ctypes.byref(batch),
                                      1 if both else 0, ctypes.byref(sp), sep, ctypes.byref(out),
                                      ctypes.c_void_p(_fresh_ptr(strand) or None), ctypes.byref(aln),
                                      ctypes.byref(mt), chunk_pairs))
            total = int(off[B])
            if total > ccap:
                ccap = total  # once: the offsets do not depend on the capacity
                continue
            break
        if B == 0:  # nothing to call with: every array is empty
            (score, ei, ej), _ = _outputs(0, True)
            ref_pos, nm, off, cig = np.empty(0, np.int64), np.empty(0, np.int32), np.zeros(1, np.uint32), None
        cigars = CigarList(cig[off[p]:off[p + 1]].copy() for p in range(B))
        cigars.n_cigar = np.diff(off.astype(np.int64)).astype(np.int32)
        if both:
            return score, ei, ej, strand, ref_pos, nm, cigars, mq, sub, cand
        return score, ei, ej, ref_pos, nm, cigars, mq, sub, cand

    def seed_candidates_device(self, index: "Index", reads_ptr: int, read_len_ptr: int, read_stride: int, n: int,
                               max_read_len: int, win_pos_ptr: int, votes_ptr: int, hits_ptr: int, flags_ptr: int,
                               win_pos1_ptr: int, votes1_ptr: int, flags1_ptr: int, rc_reads_ptr: int = 0,
                               rc_stride: int = 0, band: int = 16, cap: int = 4096, step: int = 1,
                               min_votes: int = 1, window: int = 0, sep: int = 0, stream: int = 0) -> None:
        """:meth:`seed_reads_device` with the second candidate locus
        (msw_seed_candidates_device): the first four arrays as that call
        writes them, then candidate 1's window position (-1: none), votes and
        flags (bit 0: from the reverse orientation)."""
        sp = SeedParamsT(band, cap, step, min_votes, window)
        out = SeedOutT(win_pos_ptr or None, votes_ptr or None, hits_ptr or None, flags_ptr or None)
        alt = SeedAltT(win_pos1_ptr or None, votes1_ptr or None, flags1_ptr or None)
        check(lib().msw_seed_candidates_device(
            self.handle, index.handle, ctypes.c_void_p(reads_ptr or None), ctypes.c_void_p(rc_reads_ptr or None),
            ctypes.c_void_p(read_len_ptr or None), read_stride, rc_stride, n, max_read_len, ctypes.byref(sp), sep,
            ctypes.byref(out), ctypes.byref(alt), ctypes.c_void_p(stream or None)))

    def seed_candidates(self, index: "Index", reads: np.ndarray, read_len: np.ndarray, both_strands: bool = True,
                        band: int = 16, cap: int = 4096, step: int = 1, min_votes: int = 1, window: int = 0,
                        sep: int = 0, chunk_reads: int = 0):
        """Two candidate loci per read of a host batch (msw_seed_candidates).
        Returns ((win_pos, votes, hits, flags), (win_pos1, votes1, flags1)):
        the first tuple is :meth:`seed_reads`' result, the second the best
        other band at least ``sep`` diagonals away (0 = the window length),
        win_pos1 -1 and votes1 0 where there is none."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        B = reads.shape[0]
        if read_len.shape[0] != B:
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of reads")
        win_pos, votes = np.empty(B, np.int64), np.empty(B, np.uint32)
        hits, flags = np.empty(B, np.uint32), np.empty(B, np.uint8)
        win_pos1, votes1, flags1 = np.empty(B, np.int64), np.empty(B, np.uint32), np.empty(B, np.uint8)
        batch = ReadBatchT(_ptr(reads), _ptr(read_len), reads.shape[1] if reads.ndim == 2 else 0, None, None, B)
        sp = SeedParamsT(band, cap, step, min_votes, window)
        out = SeedOutT(_fresh_ptr(win_pos), _fresh_ptr(votes), _fresh_ptr(hits), _fresh_ptr(flags))
        alt = SeedAltT(_fresh_ptr(win_pos1), _fresh_ptr(votes1), _fresh_ptr(flags1))
        check(lib().msw_seed_candidates(self.handle, index.handle, ctypes.byref(batch), 1 if both_strands else 0,
                                        ctypes.byref(sp), sep, ctypes.byref(out), ctypes.byref(alt), chunk_reads))
        return (win_pos, votes, hits, flags), (win_pos1, votes1, flags1)

    def mapq_select_device(self, primary: dict, alt: dict, read_len_ptr: int, n: int, match: int,
                           sub_score_ptr: int, mapq_ptr: int, cand_ptr: int, oriented_stride: int = 0,
                           stream: int = 0) -> None:
        """Enqueue the choice between two scored candidates per read
        (msw_mapq_select_device).  ``primary`` / ``alt``: raw device pointers
        under the keys score, end_i, end_j, win_len, strand, oriented, win_pos
        (absent or 0 = NULL); the winner lands in the primary's arrays."""
        keys = ("score", "end_i", "end_j", "win_len", "strand", "oriented", "win_pos")
        c0 = CandT(*[primary.get(k) or None for k in keys])
        c1 = CandT(*[alt.get(k) or None for k in keys])
        check(lib().msw_mapq_select_device(self.handle, ctypes.byref(c0), ctypes.byref(c1), oriented_stride,
                                           ctypes.c_void_p(read_len_ptr or None), n, match,
                                           ctypes.c_void_p(sub_score_ptr or None), ctypes.c_void_p(mapq_ptr or None),
                                           ctypes.c_void_p(cand_ptr or None), ctypes.c_void_p(stream or None)))

    # -- HBM-resident batches ----------------------------------------------------------
    def align_batch_device(self, reads_ptr: int, read_len_ptr: int, wins_ptr: int,
                           win_len_ptr: int, read_stride: int, win_stride: int, n_pairs: int,
                           score_ptr: int, max_read_len: int, max_win_len: int,
                           scoring: Scoring = LINEAR, end_i_ptr: int = 0, end_j_ptr: int = 0,
                           stream: int = 0) -> None:
        """Enqueue one scoring pass over device-resident arrays (raw device
        pointers) on ``stream`` (a hipStream_t handle, 0 = context stream)."""
        batch = BatchT(reads_ptr, wins_ptr, read_len_ptr, win_len_ptr, read_stride, win_stride,
                       n_pairs)
        out = OutT(score_ptr, end_i_ptr, end_j_ptr)
        sc = scoring.to_c()
        check(lib().msw_align_batch_device(self.handle, ctypes.byref(sc), ctypes.byref(batch),
                                           ctypes.byref(out), max_read_len, max_win_len,
                                           ctypes.c_void_p(stream or None)))

    def prepare_device_launch(self, reads_ptr: int, read_len_ptr: int, wins_ptr: int,
                              win_len_ptr: int, read_stride: int, win_stride: int, n_pairs: int,
                              score_ptr: int, max_read_len: int, max_win_len: int,
                              scoring: Scoring = LINEAR, end_i_ptr: int = 0, end_j_ptr: int = 0,
                              stream: int = 0):
        """Bind the arguments of align_batch_device once; returns a zero-argument
        callable that enqueues one pass (keeps per-launch host cost minimal)."""
        batch = BatchT(reads_ptr, wins_ptr, read_len_ptr, win_len_ptr, read_stride, win_stride,
                       n_pairs)
        out = OutT(score_ptr, end_i_ptr, end_j_ptr)
        sc = scoring.to_c()
        fn = lib().msw_align_batch_device
        args = (self.handle, ctypes.byref(sc), ctypes.byref(batch), ctypes.byref(out),
                max_read_len, max_win_len, ctypes.c_void_p(stream or None))
        keep = (batch, out, sc)

        def launch() -> None:
            _ = keep
            rc = fn(*args)
            if rc:
                check(rc)
        return launch

    def prepare_planned_launch(self, reads_ptr: int, read_len_ptr: int, wins_ptr: int,
                               win_len_ptr: int, read_stride: int, win_stride: int,
                               read_len, win_len, score_ptr: int, scoring: Scoring = LINEAR,
                               end_i_ptr: int = 0, end_j_ptr: int = 0, stream: int = 0):
        """Mixed-length device batch: build the length-bucketed plan once from the
        host length arrays (msw_plan_create), return a zero-argument callable that
        enqueues one single-launch pass (msw_align_batch_planned).  The plan is
        freed with the callable's ``close()``."""
        rl = np.ascontiguousarray(read_len, dtype=np.uint16)
        wl = np.ascontiguousarray(win_len, dtype=np.uint16)
        if rl.shape != wl.shape:
            raise ValueError("read_len / win_len shapes differ")
        sc = scoring.to_c()
        plan = ctypes.c_void_p()
        check(lib().msw_plan_create(self.handle, ctypes.byref(sc), rl.ctypes.data, wl.ctypes.data,
                                    rl.size, ctypes.byref(plan)))
        batch = BatchT(reads_ptr, wins_ptr, read_len_ptr, win_len_ptr, read_stride, win_stride, rl.size)
        out = OutT(score_ptr, end_i_ptr, end_j_ptr)
        fn = lib().msw_align_batch_planned
        args = (self.handle, plan, ctypes.byref(batch), ctypes.byref(out), ctypes.c_void_p(stream or None))
        keep = (batch, out, sc)

        class _Launch:
            def __call__(self_inner) -> None:
                _ = keep
                rc = fn(*args)
                if rc:
                    check(rc)

            def close(self_inner) -> None:
                if plan.value:
                    lib().msw_plan_destroy(plan)
                    plan.value = None

            def __del__(self_inner):
                try:
                    self_inner.close()
                except Exception:
                    pass
        return _Launch()

    def prepare(self, scoring: Scoring = LINEAR) -> None:
        """msw_ctx_prepare: load every scoring kernel module this scheme may
        use now (HIP loads a module at its first launch), so a short timed
        run does not pay for it."""
        check(lib().msw_ctx_prepare(self.handle, ctypes.byref(_scoring_c(scoring))))

    def synchronize(self) -> None:
        check(lib().msw_synchronize(self.handle))

    def stats(self, reset: bool = False) -> dict:
        """msw_ctx_stats: kernel time, launches, pairs, cells and algorithmic
        bytes of this context's host-batch calls (since creation / last reset)."""
        st = StatsT()
        check(lib().msw_ctx_stats(self.handle, ctypes.byref(st), 1 if reset else 0))
        return {"kernel_ms": st.kernel_ms, "launches": st.launches, "pairs": st.pairs, "cells": st.cells,
                "alg_bytes": st.alg_bytes}

    # -- legacy kernel ------------------------------------------------------------------
    def compat(self, s1: bytes, s2: bytes, wg: int = 0, max_groups: int = 0) -> int:
        """smith_waterman_align semantics (see gpu_align)."""
        res = ctypes.c_int32(0)
        b1 = ctypes.create_string_buffer(s1, len(s1)) if s1 else None
        b2 = ctypes.create_string_buffer(s2, len(s2)) if s2 else None
        check(lib().msw_align_compat(self.handle, b1, len(s1), b2, len(s2), wg, max_groups,
                                     ctypes.byref(res)))
        return int(res.value)


class CigarList(list):
    """Per-pair op arrays of :meth:`Context.align_batch_trace`; ``n_cigar`` holds
    the op count every pair needs (a pair over the stride has ``None`` ops)."""
    n_cigar = None


def cigar_string(ops) -> str:
    """BAM-encoded ops (len << 4 | op, M=0 I=1 D=2 S=4) -> text, e.g.
    ``"3S12M1I30M"``; no ops (score 0) -> ``"*"``."""
    if ops is None or len(ops) == 0:
        return "*"
    return "".join(f"{int(o) >> 4}{_CIGAR_CHARS[int(o) & 15]}" for o in ops)


_CIGAR_CHARS = {0: "M", 1: "I", 2: "D", 4: "S"}


def _comp_table() -> np.ndarray:
    t = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"CG", b"at", b"cg"):
        t[a], t[b] = b, a
    return t


_COMP = _comp_table()


def reverse_complement(seq):
    """The oriented read of a strand-1 record (include/msw.h, "Both
    strands"): ``rc[k] = comp(seq[L-1-k])``, comp mapping A<->T, C<->G, a<->t,
    c<->g and leaving every other byte value, N included.  bytes / str / a
    1-D uint8 array in, the same kind out.  Pure numpy, on the host."""
    if isinstance(seq, str):
        return reverse_complement(seq.encode("latin-1")).decode("latin-1")
    if isinstance(seq, (bytes, bytearray)):
        return _COMP[np.frombuffer(bytes(seq), np.uint8)[::-1]].tobytes()
    a = np.asarray(seq)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise TypeError("reverse_complement takes bytes, str or a 1-D uint8 array")
    return _COMP[a[::-1]]


class Pending:
    """An asynchronous call in flight (msw_*_async ticket).  The input and
    output arrays are held until ``wait()``; ``wait()`` returns (score, end_i,
    end_j).  Waiting on a ticket also completes every earlier one (msw_wait).
    A Pending dropped without ``wait()`` waits in its finaliser: the runtime's
    staging slots still point at its arrays until the ticket drains."""

    def __init__(self, ctx: "Context", ticket: int, outs, keep):
        self.ctx, self.ticket, self._outs, self._keep = ctx, ticket, outs, keep

    def wait(self):
        if self._keep is not None:
            check(lib().msw_wait(self.ctx.handle, self.ticket))
            self._keep = None
        return self._outs

    def __del__(self):
        try:
            if self._keep is not None and getattr(self.ctx, "_h", None) is not None:
                lib().msw_wait(self.ctx._h, self.ticket)
        except Exception:
            pass
        self._keep = None


class Genome:
    """A reference genome resident in HBM on one context (msw_genome_*)."""

    def __init__(self, ctx: Context, seq):
        if isinstance(seq, str):
            seq = seq.encode()
        a = np.ascontiguousarray(np.frombuffer(bytes(seq), np.uint8) if isinstance(seq, (bytes, bytearray))
                                 else seq, dtype=np.uint8)
        h = ctypes.c_void_p()
        check(lib().msw_genome_create(ctx.handle, _ptr(a) if a.size else None, a.size, ctypes.byref(h)))
        self._h = h
        self.ctx = ctx  # keeps the context alive for as long as the genome

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise MswError(MSW_E_INVALID, "genome is closed")
        return self._h

    def __len__(self) -> int:
        return int(lib().msw_genome_length(self.handle))

    def cut_device(self, pos_ptr: int, win_len_ptr: int, n: int, wins_ptr: int, win_stride: int,
                   win_len_out_ptr: int = 0, stream: int = 0) -> None:
        """msw_genome_cut_device: cut n windows (device arrays of positions and
        requested lengths) into a device slab, clipped lengths to
        win_len_out; enqueued on ``stream`` (0 = the context's stream)."""
        check(lib().msw_genome_cut_device(self.ctx.handle, self.handle, ctypes.c_void_p(pos_ptr),
                                          ctypes.c_void_p(win_len_ptr), n, ctypes.c_void_p(wins_ptr),
                                          win_stride, ctypes.c_void_p(win_len_out_ptr or None),
                                          ctypes.c_void_p(stream or None)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().msw_genome_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    """The k-mer index of a resident genome (msw_index_*): for every k-mer
    code the ascending genome positions of its occurrences, buckets over
    ``max_occ`` stored as empty."""

    def __init__(self, ctx: Context, genome: Genome, k: int = 12, max_occ: int = 64):
        h = ctypes.c_void_p()
        check(lib().msw_index_create(ctx.handle, genome.handle, k, max_occ, ctypes.byref(h)))
        self._h = h
        self.ctx = ctx  # keeps the context alive for as long as the index

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise MswError(MSW_E_INVALID, "index is closed")
        return self._h

    def info(self) -> dict:
        """msw_index_info: k, max_occ, the bucket count, the stored positions,
        the masked buckets, the device addresses of ``off`` and ``pos`` and
        the build's GPU time per pass (ms)."""
        i = IndexInfoT()
        check(lib().msw_index_info(self.handle, ctypes.byref(i)))
        return {"k": int(i.k), "max_occ": int(i.max_occ), "n_buckets": int(i.n_buckets), "n_pos": int(i.n_pos),
                "n_masked": int(i.n_masked), "off_ptr": int(i.off or 0), "pos_ptr": int(i.pos or 0),
                "build_ms": dict(zip(("count", "mask", "scan", "fill", "sort"), (float(v) for v in i.build_ms)))}

    def arrays(self):
        """(off uint32[4^k + 1], pos uint32[n_pos]) copied to the host."""
        i = self.info()
        off = np.empty(i["n_buckets"] + 1, np.uint32)
        pos = np.empty(i["n_pos"], np.uint32)
        check(lib().msw_memcpy_d2h(self.ctx.handle, _fresh_ptr(off), i["off_ptr"], off.nbytes))
        if pos.size:
            check(lib().msw_memcpy_d2h(self.ctx.handle, _fresh_ptr(pos), i["pos_ptr"], pos.nbytes))
        return off, pos

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().msw_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pileup:
    """Per-base counts of what aligned reads show (msw_pileup_*; include/msw.h,
    "Pileup"): ``counts()[pos]`` is A, C, G, T, other, deleted, insertions
    after, reverse-strand columns.  Add records, ``finish()`` once, then read
    ``counts()`` and ``summary()``."""

    CHANNELS = 8

    def __init__(self, ctx: Context, genome: Genome, qsum: bool = False):
        h = ctypes.c_void_p()
        if qsum:
            check(lib().msw_pileup_create_ex(ctx.handle, genome.handle, MSW_PILEUP_QSUM, ctypes.byref(h)))
        else:
            check(lib().msw_pileup_create(ctx.handle, genome.handle, ctypes.byref(h)))
        self._h = h
        self.qsum = bool(qsum)
        self.ctx = ctx        # keeps the context and the genome alive for as long as the pileup
        self.genome = genome
        self._glen = len(genome)

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise MswError(MSW_E_INVALID, "pileup is closed")
        return self._h

    def add(self, reads: np.ndarray, read_len: np.ndarray, ref_pos: np.ndarray, nm: np.ndarray, cigars,
            strand=None, mapq=None, min_mapq: int = 0, chunk_reads: int = 0, quals=None,
            min_baseq: int = 0) -> None:
        """Add the records of a host batch (msw_pileup_add): ``reads`` and
        ``read_len`` as they went into :meth:`Context.map_reads`,
        :meth:`Context.align_reads_strands` (``trace=True``) or
        :meth:`Context.align_reads_trace`, and ``ref_pos``, ``nm``, ``cigars``
        (and ``strand``, ``mapq``) as they came back.  With ``strand`` the
        reverse complement of a strand-1 read is taken on the GPU; without it
        the rows are what the CIGARs refer to.  With ``mapq``, reads below
        ``min_mapq`` are skipped.  With ``quals`` (uint8[n, qual_stride], one
        FASTQ quality byte per base of the reads as given) and
        ``min_baseq`` > 0, M columns whose Phred value is below ``min_baseq``
        are dropped (msw_pileup_add_qual; :meth:`lowq_columns` counts them).
        A ``qsum`` pileup needs ``quals`` and takes any ``min_baseq``, 0 too."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_len = np.ascontiguousarray(read_len, dtype=np.uint16)
        ref_pos = np.ascontiguousarray(ref_pos, dtype=np.int64)
        nm = np.ascontiguousarray(nm, dtype=np.int32)
        B = reads.shape[0]
        if not (read_len.shape[0] == ref_pos.shape[0] == nm.shape[0] == len(cigars) == B):
            raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of reads")
        off = np.zeros(B + 1, np.uint32)
        off[1:] = np.cumsum([0 if c is None else len(c) for c in cigars], dtype=np.uint64)
        parts = [np.asarray(c, np.uint32) for c in cigars if c is not None and len(c)]
        cig = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(1, np.uint32), dtype=np.uint32)
        opt = {}
        for name, a in (("strand", strand), ("mapq", mapq)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint8)
                if a.shape[0] != B:
                    raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of reads")
            opt[name] = a
        aln = AlnT(_ptr(ref_pos) or None, _ptr(nm) or None, _ptr(off), _ptr(cig), int(off[B]), None)
        if quals is None and min_baseq == 0:
            check(lib().msw_pileup_add(self.ctx.handle, self.handle, _ptr(reads) if reads.size else None,
                                       _ptr(read_len) if B else None, reads.shape[1] if reads.ndim == 2 else 0, B,
                                       ctypes.byref(aln), _ptr(opt["strand"]) if B else None,
                                       _ptr(opt["mapq"]) if B else None, min_mapq, chunk_reads))
            return
        qs = 0
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            if quals.ndim != 2 or quals.shape[0] != B:
                raise MswError(MSW_E_INVALID, "batch arrays disagree on the number of reads")
            qs = quals.shape[1]
        check(lib().msw_pileup_add_qual(self.ctx.handle, self.handle, _ptr(reads) if reads.size else None,
                                        _ptr(read_len) if B else None, reads.shape[1] if reads.ndim == 2 else 0, B,
                                        ctypes.byref(aln), _ptr(opt["strand"]) if B else None,
                                        _ptr(opt["mapq"]) if B else None, min_mapq,
                                        _ptr(quals) if quals is not None and quals.size else None, qs, min_baseq,
                                        chunk_reads))

    def add_device(self, rows_ptr: int, read_len_ptr: int, row_stride: int, n: int, ref_pos_ptr: int, nm_ptr: int,
                   cigar_off_ptr: int, cigar_ptr: int, cigar_cap: int, strand_ptr: int = 0, mapq_ptr: int = 0,
                   min_mapq: int = 0, stream: int = 0, quals_ptr: int = 0, qual_stride: int = 0,
                   min_baseq: int = 0) -> None:
        """Enqueue the records of n device-resident reads (raw device
        pointers, the arrays msw_aln_pack_device wrote) on ``stream``
        (msw_pileup_add_device).  ``rows_ptr``: the rows the CIGARs refer to.
        ``quals_ptr``: device quality rows in the order of the reads as given
        (``GpuFastqReader(with_qual=True)``), with ``min_baseq`` > 0 the
        threshold of msw_pileup_add_qual_device."""
        aln = AlnT(ref_pos_ptr or None, nm_ptr or None, cigar_off_ptr or None, cigar_ptr or None, cigar_cap, None)
        if quals_ptr or min_baseq:
            check(lib().msw_pileup_add_qual_device(
                self.ctx.handle, self.handle, ctypes.c_void_p(rows_ptr or None), ctypes.c_void_p(read_len_ptr or None),
                row_stride, n, ctypes.byref(aln), ctypes.c_void_p(strand_ptr or None),
                ctypes.c_void_p(mapq_ptr or None), min_mapq, ctypes.c_void_p(quals_ptr or None), qual_stride,
                min_baseq, ctypes.c_void_p(stream or None)))
            return
        check(lib().msw_pileup_add_device(self.ctx.handle, self.handle, ctypes.c_void_p(rows_ptr or None),
                                          ctypes.c_void_p(read_len_ptr or None), row_stride, n, ctypes.byref(aln),
                                          ctypes.c_void_p(strand_ptr or None), ctypes.c_void_p(mapq_ptr or None),
                                          min_mapq, ctypes.c_void_p(stream or None)))

    def finish(self, stream: int = 0) -> None:
        """Fold the state into the counts (msw_pileup_finish); afterwards the
        pileup takes no more reads.  A second call does nothing."""
        check(lib().msw_pileup_finish(self.ctx.handle, self.handle, ctypes.c_void_p(stream or None)))

    def lowq_columns(self) -> int:
        """M columns dropped by ``min_baseq`` so far (msw_pileup_lowq_columns);
        synchronous, before or after finish()."""
        n = ctypes.c_uint64()
        check(lib().msw_pileup_lowq_columns(self.ctx.handle, self.handle, ctypes.byref(n)))
        return int(n.value)

    def counts(self) -> np.ndarray:
        """uint32[glen][8] on the host (msw_pileup_counts); after finish()."""
        out = np.empty((self._glen, self.CHANNELS), np.uint32)
        check(lib().msw_pileup_counts(self.ctx.handle, self.handle, _fresh_ptr(out) or None))
        return out

    def counts_device(self):
        """(device pointer, position stride, channel stride) in uint32 words
        (msw_pileup_counts_device)."""
        ptr, ps, cs = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().msw_pileup_counts_device(self.ctx.handle, self.handle, ctypes.byref(ptr), ctypes.byref(ps),
                                             ctypes.byref(cs)))
        return int(ptr.value or 0), int(ps.value), int(cs.value)

    def qsums(self) -> np.ndarray:
        """uint32[glen][4] on the host (msw_pileup_qsums): per base and allele
        A, C, G, T the summed Phred values of the counted columns; after
        finish(), on a ``qsum`` pileup."""
        out = np.empty((self._glen, 4), np.uint32)
        check(lib().msw_pileup_qsums(self.ctx.handle, self.handle, _fresh_ptr(out) or None))
        return out

    def qsums_device(self):
        """(device pointer, position stride, channel stride) in uint32 words
        (msw_pileup_qsums_device)."""
        ptr, ps, cs = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().msw_pileup_qsums_device(self.ctx.handle, self.handle, ctypes.byref(ptr), ctypes.byref(ps),
                                            ctypes.byref(cs)))
        return int(ptr.value or 0), int(ps.value), int(cs.value)

    def summary(self, min_depth: int = 1) -> dict:
        """covered, depth_sum, max_depth, minority_ref, reads_used and
        reads_skipped of the finished counts (msw_pileup_summary)."""
        s = PileupSummaryT()
        check(lib().msw_pileup_summary(self.ctx.handle, self.handle, min_depth, ctypes.byref(s)))
        return {k: int(getattr(s, k)) for k in ("covered", "depth_sum", "max_depth", "minority_ref", "reads_used",
                                                "reads_skipped")}

    def call_device(self, out_ptr: int, cap: int, n_total_ptr: int, params: Optional[CallParams] = None,
                    stream: int = 0, qual_params: Optional[QualParams] = None) -> None:
        """Enqueue the call on ``stream`` (msw_pileup_call_device): up to
        ``cap`` 48-byte records to the device pointer ``out_ptr`` and the total
        as a u64 to ``n_total_ptr``; ``out_ptr`` 0 with ``cap`` 0 runs the count
        pass alone.  No host synchronisation.  With ``qual_params`` the
        genotypes are quality-weighted (msw_pileup_call_qual_device), as in
        :meth:`call`."""
        q = (params or CallParams()).to_c()
        if qual_params is not None:
            qq = qual_params.to_c()
            check(lib().msw_pileup_call_qual_device(self.ctx.handle, self.handle, ctypes.byref(q), ctypes.byref(qq),
                                                    ctypes.c_void_p(out_ptr or None), cap,
                                                    ctypes.c_void_p(n_total_ptr or None),
                                                    ctypes.c_void_p(stream or None)))
            return
        check(lib().msw_pileup_call_device(self.ctx.handle, self.handle, ctypes.byref(q),
                                           ctypes.c_void_p(out_ptr or None), cap, ctypes.c_void_p(n_total_ptr or None),
                                           ctypes.c_void_p(stream or None)))

    def call(self, params: Optional[CallParams] = None, qual_params: Optional[QualParams] = None) -> Variants:
        """Variant calls from the finished counts (msw_pileup_call): one count
        call, then one call that fills the records.  The genotypes are
        quality-weighted (msw_pileup_call_qual) exactly when ``qual_params`` is
        given -- ``QualParams()`` for the default weights; without it the call
        is the unweighted one on a ``qsum`` pileup too, so the flag alone never
        changes a result.  ``qual_params`` on a pileup without quality sums is
        MSW_E_INVALID."""
        q = (params or CallParams()).to_c()
        total = ctypes.c_uint64()
        if qual_params is not None:
            qq = qual_params.to_c()

            def run(out, cap):
                check(lib().msw_pileup_call_qual(self.ctx.handle, self.handle, ctypes.byref(q), ctypes.byref(qq), out,
                                                 cap, ctypes.byref(total)))
        else:
            def run(out, cap):
                check(lib().msw_pileup_call(self.ctx.handle, self.handle, ctypes.byref(q), out, cap,
                                            ctypes.byref(total)))
        run(None, 0)
        n = int(total.value)
        rec = np.zeros(n, VARIANT_DTYPE)
        if n:
            run(_fresh_ptr(rec), n)
        return Variants.from_records(rec)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().msw_pileup_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pinned_empty(shape, dtype) -> np.ndarray:
    """A numpy array in page-locked host memory (msw_host_alloc): batches held
    in such arrays are copied to the GPU directly, without staging.  The
    memory is freed when the array (and every view of it) is collected."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    p = lib().msw_host_alloc(max(n, 1))
    if not p:
        check(-5)
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=np.uint8, count=n).view(dt).reshape(shape)

    class _Owner:
        def __del__(self_inner):
            lib().msw_host_free(p)
    # numpy keeps `buf` alive through arr.base; hang the owner on the ctypes buffer
    buf._owner = _Owner()
    return arr


_contexts: dict = {}
_ctx_lock = threading.Lock()


def get_context(device=0) -> Context:
    """Process-wide context per GPU (gpu.rs:97-109 get_opencl_context)."""
    ordinal = device.ordinal if isinstance(device, GpuDevice) else int(device)
    with _ctx_lock:
        ctx = _contexts.get(ordinal)
        if ctx is None:
            ctx = _contexts[ordinal] = Context(ordinal)
        return ctx


def gpu_align(seq1: str, seq2: str, device: GpuDevice) -> int:
    """aligner.rs:410-532: the score of the kernel the reference launches
    (smith_waterman_align), with its host geometry W = min(max_wg, 1024),
    G = min(ceil(L/W), 1e6); L == 0 -> 0; oversize -> MswError."""
    b1 = seq1.encode() if isinstance(seq1, str) else bytes(seq1)
    b2 = seq2.encode() if isinstance(seq2, str) else bytes(seq2)
    wg = min(int(device.max_work_group_size), GPU_WORK_GROUP_SIZE)
    return get_context(device).compat(b1, b2, wg, GPU_MAX_WORK_GROUPS)


def gpu_align_chunk_self(chunk: str, device: GpuDevice) -> int:
    """aligner.rs:365-373: chunks under 1000 bases score 0, else self-align."""
    if len(chunk) < 1000:
        return 0
    return gpu_align(chunk, chunk, device)


def get_chunk_size_reads() -> int:
    """aligner.rs:9-15: GPU_CHUNK_SIZE_READS is mandatory."""
    v = os.environ.get("GPU_CHUNK_SIZE_READS")
    if v is None:
        raise MswError(MSW_E_INVALID, "GPU_CHUNK_SIZE_READS not set in .env file")
    try:
        n = int(v)
        if n < 0:
            raise ValueError(v)
        return n
    except ValueError as e:
        raise MswError(MSW_E_INVALID, f"Invalid GPU_CHUNK_SIZE_READS value '{v}': {e}") from None


def pack_batch(reads: Sequence[bytes], wins: Sequence[bytes], read_stride: Optional[int] = None,
               win_stride: Optional[int] = None):
    """Lists of byte strings -> padded SoA arrays (reads, read_len, wins, win_len)."""
    B = len(reads)
    if len(wins) != B:
        raise MswError(MSW_E_INVALID, "reads and windows differ in count")
    rl = np.array([len(r) for r in reads], np.uint16)
    wl = np.array([len(w) for w in wins], np.uint16)
    rs = read_stride or max(16, (int(rl.max()) if B else 0) + 15) // 16 * 16
    ws = win_stride or max(16, (int(wl.max()) if B else 0) + 15) // 16 * 16
    R = np.zeros((B, rs), np.uint8)
    W = np.zeros((B, ws), np.uint8)
    for i, (r, w) in enumerate(zip(reads, wins)):
        R[i, :len(r)] = np.frombuffer(bytes(r), np.uint8)
        W[i, :len(w)] = np.frombuffer(bytes(w), np.uint8)
    return R, rl, W, wl
