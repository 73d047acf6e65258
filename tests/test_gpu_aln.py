"""Alignment records for reads against the genome: the trace that reads its
windows straight from the genome (msw_trace_reads_device), the packed records
(msw_aln_pack_device), the host call and its Python wrapper, and
``rustseq_mini --full-wgs --alignments-out``.

References: tests/traceback_oracle.py (the canonical alignment), tests/aln_oracle.py
(ref_pos, soft clips, NM), and the path that existed before the feature
(msw_genome_cut_device + msw_trace_batch_device).  Every device output array
has sentinel words behind it.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import aln_oracle as ao
import traceback_oracle as tbo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mini_parallel_amd", "rustseq_mini")
LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)
SCHEMES = {"lin": LIN, "aff": AFF}
ACGT = np.frombuffer(b"ACGT", np.uint8)
GUARD = 8
SCAN_TILE = 1024   # kAlnScanTile (msw_kernels.h): offsets one scan block covers


def scoring(scheme, coords=True):
    from mini_parallel_amd import Scoring
    m, x, go, ge, aff = scheme
    return Scoring(match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff, want_coords=coords)


# ---------------------------------------------------------------------------
# device arrays with guard words
# ---------------------------------------------------------------------------
FILL = {np.int16: -21555, np.int32: 0x5EADBEEF, np.int64: 0x5EADBEEF5EADBEEF, np.uint8: 0xA5}


class Guarded:
    """A device array of n elements followed by GUARD sentinel elements; the
    payload starts as the sentinel too (an element the call must write shows)."""

    def __init__(self, n, dtype):
        import torch
        self.n, self.dtype = n, dtype
        tdt = {np.int16: torch.int16, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}[dtype]
        self.t = torch.full((n + GUARD,), FILL[dtype], dtype=tdt, device="cuda:0")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, view=None):
        """Payload on the host; asserts the guard is intact."""
        a = self.t.cpu().numpy()
        assert (a[self.n:] == FILL[self.dtype]).all(), "guard words overwritten"
        a = a[:self.n]
        return a.view(view) if view is not None else a


def to_dev(a, as_type=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(as_type) if as_type is not None else a).to("cuda:0")


class DevReads:
    def __init__(self, R, rl, pos):
        self.R, self.rl, self.pos = R, rl, pos
        self.n, self.stride = R.shape[0], R.shape[1]
        self.d_R, self.d_rl, self.d_pos = to_dev(R), to_dev(rl, np.int16), to_dev(pos)
        self.max_len = max(1, int(rl.max())) if rl.size else 1


def score_reads(ctx, genome, D, window, scheme):
    """msw_align_reads_device with coordinates -> (score, end_i, end_j) device arrays."""
    from mini_parallel_amd._lib import OutT, check, lib
    s, ei, ej = Guarded(D.n, np.int32), Guarded(D.n, np.int16), Guarded(D.n, np.int16)
    out = OutT(s.ptr, ei.ptr, ej.ptr)
    check(lib().msw_align_reads_device(ctx.handle, ctypes.byref(scoring(scheme).to_c()), genome.handle, D.d_R.data_ptr(),
                                       D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), D.n, window, D.max_len,
                                       ctypes.byref(out), None, None))
    ctx.synchronize()
    return s, ei, ej


class Trace:
    def __init__(self, n, stride):
        self.stride = stride
        self.si, self.sj = Guarded(n, np.int16), Guarded(n, np.int16)
        self.nc, self.rows = Guarded(n, np.int32), Guarded(n * stride, np.int32)

    def host(self):
        return self.si.get(), self.sj.get(), self.nc.get(), self.rows.get(np.uint32)


def trace_reads(ctx, genome, D, ends, window, scheme, stride):
    """The new path: windows read from the genome."""
    s, ei, ej = ends
    tr = Trace(D.n, stride)
    ctx.trace_reads_device(genome, D.d_R.data_ptr(), D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), D.n, window,
                           D.max_len, s.ptr, ei.ptr, ej.ptr, tr.si.ptr, tr.sj.ptr, tr.nc.ptr, tr.rows.ptr, stride,
                           scoring(scheme, coords=False))
    ctx.synchronize()
    return tr


def requested(rl, window):
    return (np.minimum(2 * rl.astype(np.int64), 4096) if window == 0 else np.full(rl.size, window)).astype(np.uint16)


def trace_cut_slab(ctx, genome, D, ends, window, scheme, stride):
    """The path that existed before: cut the windows into a slab, trace the padded batch."""
    s, ei, ej = ends
    want = requested(D.rl, window)
    max_win = max(1, int(want.max()))
    ws = max(16, (max_win + 15) // 16 * 16)
    wins = Guarded(D.n * ws, np.uint8)
    wl = Guarded(D.n, np.int16)
    d_want = to_dev(want, np.int16)
    genome.cut_device(D.d_pos.data_ptr(), d_want.data_ptr(), D.n, wins.ptr, ws, wl.ptr)
    tr = Trace(D.n, stride)
    ctx.trace_batch_device(D.d_R.data_ptr(), D.d_rl.data_ptr(), wins.ptr, wl.ptr, D.stride, ws, D.n, s.ptr, ei.ptr,
                           ej.ptr, tr.si.ptr, tr.sj.ptr, tr.nc.ptr, tr.rows.ptr, stride, D.max_len, max_win,
                           scoring(scheme, coords=False))
    ctx.synchronize()
    return tr


class Packed:
    def __init__(self, n, cap):
        self.n, self.cap = n, cap
        self.ref, self.nm = Guarded(n, np.int64), Guarded(n, np.int32)
        self.off, self.ops, self.ovf = Guarded(n + 1, np.int32), Guarded(cap, np.int32), Guarded(1, np.int32)

    def host(self):
        return self.ref.get(), self.nm.get(), self.off.get(np.uint32), self.ops.get(np.uint32), int(self.ovf.get()[0])


def pack(ctx, genome, D, ends, tr, cap):
    s, ei, ej = ends
    pk = Packed(D.n, cap)
    ctx.aln_pack_device(genome, D.d_R.data_ptr(), D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), D.n, s.ptr, ei.ptr,
                        ej.ptr, tr.si.ptr, tr.sj.ptr, tr.nc.ptr, tr.rows.ptr, tr.stride, pk.ref.ptr, pk.nm.ptr,
                        pk.off.ptr, pk.ops.ptr, cap, pk.ovf.ptr)
    ctx.synchronize()
    return pk


def pad_reads(reads, stride=None):
    rl = np.array([len(r) for r in reads], np.uint16)
    stride = stride or max(16, (int(rl.max()) + 15) // 16 * 16)
    R = np.zeros((len(reads), stride), np.uint8)
    for k, r in enumerate(reads):
        R[k, :len(r)] = r
    return R, rl


# ---------------------------------------------------------------------------
# 1. trace straight from the genome
# ---------------------------------------------------------------------------
GENOME_LEN = 20011
READ_LENS = [1, 63, 64, 65, 150, 384]
WINDOWS = [0, 1, 8, 9, 300, 4096]


def the_genome():
    return np.random.default_rng(2024).choice(ACGT, GENOME_LEN).astype(np.uint8)


def mutated(rng, src, m):
    """m bases from src with a few substitutions and short indels."""
    r = [int(x) for x in src[:m]] or [int(ACGT[0])]
    for _ in range(1 + m // 40):
        k = int(rng.integers(0, len(r)))
        what = int(rng.integers(0, 3))
        if what == 0:
            r[k] = int(rng.choice(ACGT))
        elif what == 1:
            r[k:k] = [int(x) for x in rng.choice(ACGT, int(rng.integers(1, 3)))]
        elif len(r) > 4:
            del r[k:k + int(rng.integers(1, 3))]
    while len(r) < m:
        r.append(int(rng.choice(ACGT)))
    return np.array(r[:m], np.uint8)


def trace_case(window):
    """Five pairs per read length: one inside the genome at a position that is
    1, 2, 3 or 3 mod 4 (two of them odd: win_pos has no alignment), rotating
    over the lengths, then a negative position, one >= the genome length, one
    within W of the genome end (a clipped window) and the last base (a window
    of length 1)."""
    g = the_genome()
    rng = np.random.default_rng(100 + window)
    reads, pos = [], []
    for li, m in enumerate(READ_LENS):
        W = window or min(2 * m, 4096)
        kinds = [1001 + 4 * li, 2002 + 4 * li, 3003 + 4 * li, 7007 + 4 * li,      # 1, 2, 3, 3 mod 4; two are odd
                 -1 - li, GENOME_LEN + 5 * li, GENOME_LEN - max(1, W // 2), GENOME_LEN - 1]
        for p in [kinds[li % 4]] + kinds[4:]:
            pos.append(p)
            a = min(max(p, 0), GENOME_LEN - 1)
            # the read comes from inside its window, so that it aligns there
            src = g[a + min(W // 3, 40):a + W + m] if W > 2 else g[a:a + m]
            reads.append(mutated(rng, src, m) if len(src) >= 1 else rng.choice(ACGT, m).astype(np.uint8))
    return g, reads, np.array(pos, np.int64)


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("window", WINDOWS)
def test_trace_from_genome(gpu_ctx, window, scheme):
    """msw_trace_reads_device == msw_genome_cut_device + msw_trace_batch_device on
    the same ends, array for array, == the full-matrix restatement.  Read
    lengths 1 .. 384 under every window rule; at window 4096 the 384-base
    reads' rectangles (384 x 4096) go to the global slab beside LDS pairs."""
    sch = SCHEMES[scheme]
    g, reads, pos = trace_case(window)
    inside = [int(p) for p in pos if 0 <= p < GENOME_LEN - 4096]
    assert {p % 4 for p in inside} >= {1, 2, 3} and any(p % 2 for p in inside)
    assert (pos < 0).any() and (pos >= GENOME_LEN).any() and (pos == GENOME_LEN - 1).any()
    R, rl = pad_reads(reads, 384)
    D = DevReads(R, rl, pos)
    genome = gpu_ctx.load_genome(g)
    ends = score_reads(gpu_ctx, genome, D, window, sch)
    stride = 96
    new = trace_reads(gpu_ctx, genome, D, ends, window, sch, stride).host()
    old = trace_cut_slab(gpu_ctx, genome, D, ends, window, sch, stride).host()
    for a, b, name in zip(new, old, ("start_i", "start_j", "n_cigar", "cigar")):
        assert np.array_equal(a, b), name
    s, ei, ej = (x.get() for x in ends)
    si, sj, nc, rows = new
    rows = rows.reshape(D.n, stride)
    want = requested(rl, window)
    slab_pairs = 0
    for p in range(D.n):
        w = ao.window_of(g, int(pos[p]), int(want[p]))
        exp = tbo.align(reads[p], w, *sch)
        tag = f"pair {p}: read {rl[p]} pos {pos[p]} window {len(w)}"
        assert (int(s[p]), (int(ei[p]), int(ej[p])), (int(si[p]), int(sj[p]))) == exp[:3], tag
        assert int(nc[p]) == len(exp[3]) <= stride, tag
        assert [int(o) for o in rows[p, :nc[p]]] == exp[3], tag
        assert (rows[p, nc[p]:] == 0x5EADBEEF).all(), tag          # nothing past the ops of the row
        words = (int(ei[p]) + 1) * -(-(int(ej[p]) + 1) // (8 if sch[4] else 16))
        slab_pairs += words > 8192
    if window == 4096:
        assert slab_pairs >= 1 and slab_pairs < D.n      # slab and LDS pairs in one launch
    assert len(ao.window_of(g, GENOME_LEN - 1, 300)) == 1
    genome.close()


def test_trace_reads_range(gpu_ctx):
    """Past 384 x 4096 the genome trace is MSW_E_RANGE, like the padded one."""
    import mini_parallel_amd as mpa
    g = the_genome()
    genome = gpu_ctx.load_genome(g)
    R, rl = pad_reads([g[:100].copy()], 400)
    D = DevReads(R, rl, np.array([0], np.int64))
    ends = score_reads(gpu_ctx, genome, D, 300, LIN)
    tr = Trace(1, 8)
    args = lambda window, max_len: (genome, D.d_R.data_ptr(), D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), 1,
                                    window, max_len, ends[0].ptr, ends[1].ptr, ends[2].ptr, tr.si.ptr, tr.sj.ptr,
                                    tr.nc.ptr, tr.rows.ptr, 8, scoring(LIN))
    for window, max_len in ((300, 385), (4097, 100)):
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.trace_reads_device(*args(window, max_len))
        assert e.value.code == -2
    gpu_ctx.trace_reads_device(*args(4096, 384))
    gpu_ctx.synchronize()
    assert int(tr.nc.get()[0]) == 1
    genome.close()


# ---------------------------------------------------------------------------
# 2. pack against aln_oracle
# ---------------------------------------------------------------------------
POOL_WINDOW = 120
_POOL = {}


def pool(scheme):
    """257 reads against 120-base windows: no clip, leading clip, trailing
    clip, both; score 0 and empty reads between aligned ones; non-ACGT bytes;
    runs of mismatches inside M; indels.  With the oracle's records."""
    if scheme in _POOL:
        return _POOL[scheme]
    g = the_genome()
    rng = np.random.default_rng(77)
    junk = lambda n: np.frombuffer(b"Nn*-RYKM"[:8], np.uint8)[rng.integers(0, 8, n)]   # never equals a genome byte
    reads, pos = [], []
    for k in range(257):
        p = int(rng.integers(0, GENOME_LEN - 200)) | 1 if k % 3 else int(rng.integers(0, GENOME_LEN - 200))
        a = p + int(rng.integers(0, 50))
        core = g[a:a + int(rng.integers(20, 50))].copy()
        kind = k % 8
        if kind == 0:
            r = core
        elif kind == 1:
            r = np.concatenate([junk(int(rng.integers(1, 9))), core])
        elif kind == 2:
            r = np.concatenate([core, junk(int(rng.integers(1, 9)))])
        elif kind == 3:
            r = np.concatenate([junk(int(rng.integers(1, 9))), core, junk(int(rng.integers(1, 9)))])
        elif kind == 4:
            r = junk(int(rng.integers(1, 40)))                       # score 0
        elif kind == 5:
            r = core if k % 16 == 5 else core[:0]                    # an empty window (below) or an empty read
            p = -3 if k % 16 == 5 else p
        elif kind == 6:
            r = np.concatenate([g[a:a + 25], junk(3), g[a + 28:a + 55]])   # three mismatches in a row inside M
            r[5] = ord("N")
        else:
            r = mutated(rng, g[a:a + 60], 50)
        reads.append(np.asarray(r, np.uint8))
        pos.append(p)
    pos = np.array(pos, np.int64)
    recs = [ao.record(reads[k], ao.window_of(g, int(pos[k]), POOL_WINDOW), int(pos[k]), *SCHEMES[scheme])
            for k in range(257)]
    text = [ao.cigar_text(r.ops) for r in recs]
    lead = [t != "*" and t.split("S")[0].isdigit() and "S" in t for t in text]
    trail = [t.endswith("S") for t in text]
    # the mix is what the docstring says
    assert any(l and not t for l, t in zip(lead, trail)) and any(t and not l for l, t in zip(lead, trail))
    assert any(l and t for l, t in zip(lead, trail)) and any(x != "*" and "S" not in x for x in text)
    assert sum(x == "*" for x in text) >= 60 and any("I" in x or "D" in x for x in text)
    assert any(r.nm >= 3 and ao.cigar_text(r.ops).count("M") == 1 for r in recs)
    _POOL[scheme] = (g, reads, pos, recs)
    return _POOL[scheme]


def pool_batch(scheme, B):
    g, reads, pos, recs = pool(scheme)
    sel = [3] if B == 1 else list(range(B))
    return g, [reads[k] for k in sel], pos[sel], [recs[k] for k in sel]


def run_pack(ctx, g, reads, pos, scheme, stride, cap=None, window=POOL_WINDOW):
    R, rl = pad_reads(reads, 80)
    D = DevReads(R, rl, pos)
    genome = ctx.load_genome(g)
    ends = score_reads(ctx, genome, D, window, SCHEMES[scheme])
    tr = trace_reads(ctx, genome, D, ends, window, SCHEMES[scheme], stride)
    if cap is None:       # enough for everything
        cap = D.n * (stride + 2)
    pk = pack(ctx, genome, D, ends, tr, cap)
    out = (tuple(x.get() for x in ends), tr.host(), pk.host())
    genome.close()
    return out


def check_records(ends, packed, recs, rl):
    s, ei, ej = ends
    ref, nm, off, ops, ovf = packed
    assert ovf == 0
    assert [int(x) for x in s] == [r.score for r in recs]
    assert [(int(a), int(b)) for a, b in zip(ei, ej)] == [(r.end_i, r.end_j) for r in recs]
    assert [int(x) for x in ref] == [r.ref_pos for r in recs]
    assert [int(x) for x in nm] == [r.nm for r in recs]
    assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), [len(r.ops) for r in recs])
    for p, r in enumerate(recs):
        got = [int(o) for o in ops[off[p]:off[p + 1]]]
        assert got == r.ops, (p, ao.cigar_text(got), ao.cigar_text(r.ops))
        assert ao.read_bases(got) == (int(rl[p]) if got else 0), p        # the CIGAR covers the whole read
    assert (ops[off[-1]:] == 0x5EADBEEF).all()


@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_pack_against_oracle(gpu_ctx, B, scheme):
    g, reads, pos, recs = pool_batch(scheme, B)
    ends, _, packed = run_pack(gpu_ctx, g, reads, pos, scheme, stride=24)
    check_records(ends, packed, recs, [len(r) for r in reads])


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_pack_trace_overflow(gpu_ctx, scheme):
    """cigar_stride = 1: a read with more than one traced op has nm -1 and no
    ops and is counted; one-op reads keep their records and clips."""
    g, reads, pos, recs = pool_batch(scheme, 65)
    ends, tr, (ref, nm, off, ops, ovf) = run_pack(gpu_ctx, g, reads, pos, scheme, stride=1)
    traced = [[o for o in r.ops if (o & 15) != ao.S] for r in recs]
    over = [len(t) > 1 for t in traced]
    assert any(over) and ovf == sum(over)
    assert np.array_equal(tr[2], [len(t) for t in traced])                       # n_cigar still says what is needed
    for p, r in enumerate(recs):
        got = [int(o) for o in ops[off[p]:off[p + 1]]]
        assert int(ref[p]) == r.ref_pos, p                                     # the start cell is valid either way
        assert (int(nm[p]), got) == ((-1, []) if over[p] else (r.nm, r.ops)), p
    assert (ops[off[-1]:] == 0x5EADBEEF).all()


def test_pack_cap_one_short(gpu_ctx):
    """cigar_cap one below the total: the offsets are complete, the ops below
    the cap are the right ones, nothing is written at or past the cap."""
    g, reads, pos, recs = pool_batch("aff", 65)
    total = sum(len(r.ops) for r in recs)
    _, _, (ref, nm, off, ops, ovf) = run_pack(gpu_ctx, g, reads, pos, "aff", stride=24, cap=total - 1)
    assert len(ops) == total - 1 and ovf == 0                 # Guarded.get() has checked the words at the cap
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(r.ops) for r in recs])]))
    assert [int(o) for o in ops] == [o for r in recs for o in r.ops][:total - 1]
    assert [int(x) for x in nm] == [r.nm for r in recs]
    # and no ops at all
    _, _, (_, _, off0, ops0, _) = run_pack(gpu_ctx, g, reads, pos, "aff", stride=24, cap=0)
    assert np.array_equal(off0, off) and len(ops0) == 0


# ---------------------------------------------------------------------------
# 3. the scan's levels, without an oracle
# ---------------------------------------------------------------------------
MENU = [[], [8 << 4], [3 << 4, 1 << 4 | 1, 4 << 4], [2 << 4, 2 << 4 | 2, 6 << 4]]
# read index / genome offset of every M column of the item, and its I + D bases
MENU_COLS = [([], [], 0), (list(range(8)), list(range(8)), 0), ([0, 1, 2, 4, 5, 6, 7], list(range(7)), 1),
             (list(range(8)), [0, 1, 4, 5, 6, 7, 8, 9], 2)]


@pytest.mark.parametrize("n", [1, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1,
                               SCAN_TILE ** 2 - 2, SCAN_TILE ** 2 - 1, SCAN_TILE ** 2, SCAN_TILE ** 2 + 1])
def test_scan_levels(gpu_ctx, n):
    """The prefix sum runs over n + 1 offsets in tiles of 1024: one level up to
    n + 1 = 1024, two up to 1024^2 = 2^20, three beyond (the last four sizes;
    2^20 and 2^20 + 1 reads are past 2^20 offsets).  n + 1 just below, at and
    just above each boundary.  The next boundary, 2^30 offsets, is out of a
    test's reach (> 60 GB of inputs); the levels are one recursive routine, so
    the third level runs the code the second does.  Inputs are synthetic but
    consistent: 8-base reads, each with one of four traces (none, 8M, 3M1I4M,
    2M2D6M) at any genome position; checked against numpy.cumsum and a
    vectorised NM."""
    g = the_genome()
    rng = np.random.default_rng(n)
    item = rng.integers(0, 4, n)
    pos = rng.integers(0, GENOME_LEN - 10, n).astype(np.int64)
    sj = rng.integers(0, 3, n).astype(np.int16)               # window-relative start: ref_pos = pos + sj
    pos -= sj
    R = g[(pos + sj)[:, None] + np.arange(8)[None, :]]
    R = np.where(rng.random((n, 8)) < 0.2, rng.choice(ACGT, (n, 8)), R).astype(np.uint8)
    rl = np.full(n, 8, np.uint16)
    score = np.where(item > 0, 5, 0).astype(np.int32)
    ei = np.where(item > 0, 7, -1).astype(np.int16)
    si = np.where(item > 0, 0, -1).astype(np.int16)
    sj = np.where(item > 0, sj, -1).astype(np.int16)
    nc = np.array([len(m) for m in MENU], np.int32)[item]
    rows = np.zeros((n, 3), np.uint32)
    for k, m in enumerate(MENU):
        rows[item == k, :len(m)] = m
    nm = np.zeros(n, np.int64)
    for k, (ri, gj, gaps) in enumerate(MENU_COLS):
        sel = item == k
        if ri:
            nm[sel] = (R[sel][:, ri] != g[(pos[sel] + sj[sel])[:, None] + np.array(gj)[None, :]]).sum(axis=1) + gaps
    D = DevReads(R, rl, pos)
    genome = gpu_ctx.load_genome(g)
    ends = (Guarded(n, np.int32), Guarded(n, np.int16), Guarded(n, np.int16))
    tr = Trace(n, 3)
    for dst, src in ((ends[0], score), (ends[1], ei), (tr.si, si), (tr.sj, sj), (tr.nc, nc),
                     (tr.rows, rows.view(np.int32).ravel())):
        dst.t[:src.size] = to_dev(src)
    total = int(nc.sum())
    ref, got_nm, off, ops, ovf = pack(gpu_ctx, genome, D, ends, tr, total).host()
    assert ovf == 0
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(nc, dtype=np.int64)]).astype(np.uint32))
    assert np.array_equal(ops, rows[np.arange(3)[None, :] < nc[:, None]])
    assert np.array_equal(got_nm, nm) and np.array_equal(ref, np.where(item > 0, pos + sj, -1))
    genome.close()


# ---------------------------------------------------------------------------
# 4. the host call and its wrapper
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_host_call_and_wrapper(gpu_ctx, scheme):
    """Context.align_reads_trace in chunks smaller than the batch == the device
    calls == the oracle; a first capacity that is too small is retried once;
    the raw call with too small a capacity still completes the offsets."""
    from mini_parallel_amd import _lib, cigar_string
    g, reads, pos, recs = pool_batch(scheme, 65)
    R, rl = pad_reads(reads, 80)
    want = np.full(65, POOL_WINDOW, np.uint16)
    genome = gpu_ctx.load_genome(g)
    _, _, (d_ref, d_nm, d_off, d_ops, _) = run_pack(gpu_ctx, g, reads, pos, scheme, stride=24)
    for kw in ({"chunk_pairs": 7}, {"chunk_pairs": 7, "cigar_cap": 1}, {}):
        s, ei, ej, ref, nm, cigars = gpu_ctx.align_reads_trace(genome, R, rl, pos, want, scoring(SCHEMES[scheme], False), **kw)
        assert np.array_equal(ref, d_ref) and np.array_equal(nm, d_nm)
        assert np.array_equal(cigars.n_cigar, np.diff(d_off.astype(np.int64)))
        assert np.array_equal(np.concatenate(list(cigars)), d_ops[:d_off[-1]])
        for p, r in enumerate(recs):
            assert (int(s[p]), int(ei[p]), int(ej[p]), int(ref[p]), int(nm[p])) == (r.score, r.end_i, r.end_j, r.ref_pos,
                                                                                   r.nm), p
            assert cigar_string(cigars[p]) == ao.cigar_text(r.ops), p
    # raw: cigar_cap below the total
    n = 65
    s, ei, ej = np.zeros(n, np.int32), np.zeros(n, np.int16), np.zeros(n, np.int16)
    ref, nm, off = np.zeros(n, np.int64), np.zeros(n, np.int32), np.full(n + 1, 7, np.uint32)
    cig = np.full(5 + GUARD, 0xDEADBEEF, np.uint32)
    ovf = np.full(1, 9, np.uint32)
    batch = _lib.ReadBatchT(R.ctypes.data, rl.ctypes.data, R.shape[1], pos.ctypes.data, want.ctypes.data, n)
    out = _lib.OutT(s.ctypes.data, ei.ctypes.data, ej.ctypes.data)
    aln = _lib.AlnT(ref.ctypes.data, nm.ctypes.data, off.ctypes.data, cig.ctypes.data, 5, ovf.ctypes.data)
    _lib.check(_lib.lib().msw_align_reads_trace(gpu_ctx.handle, ctypes.byref(scoring(SCHEMES[scheme]).to_c()), genome.handle,
                                                ctypes.byref(batch), ctypes.byref(out), ctypes.byref(aln), 16))
    assert np.array_equal(off, d_off) and int(ovf[0]) == 0 and (cig[5:] == 0xDEADBEEF).all()
    assert np.array_equal(ref, d_ref) and np.array_equal(nm, d_nm)
    genome.close()


# ---------------------------------------------------------------------------
# 5. rustseq_mini --full-wgs --alignments-out
# ---------------------------------------------------------------------------
def run_cli(args, env, cwd):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, env=e, cwd=cwd, timeout=300)


def wgs_env(root, run_id, **extra):
    env = {"WGS_DATA_DIR": str(root / "wgs"), "WGS_SAMPLE_ID": "SYN", "WGS_LANES": "1", "WGS_READS_PER_LANE": "2",
           "GPU_CHUNK_SIZE_READS": "100", "WGS_RUN_ID": run_id, "MSW_GFASTQ_BATCH": "100", "MSW_GFASTQ_SPAN_MB": "1"}
    env.update(extra)
    return env


def wgs_args(root, ds, scheme, run_id):
    gap = ["--gap-model", "affine", "--gap-open", "3", "--gap-extend", "1"] if SCHEMES[scheme][4] else []
    (root / run_id).mkdir()
    return ["--full-wgs", "--gpu", "--score-mode", "sw", "--reference", ds["reference"], "--window", "300",
            "--checkpoint-dir", root / run_id] + gap


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_cli_alignments_out(tmp_path, scheme):
    """Two BGZF lane files of 300 reads in batches of 100: every .aln equals
    the oracle read for read; MSW_CLI_CIGAR_STRIDE=1 (every multi-op read is
    traced again at the exact stride) writes the same alignments; --scores-out
    beside it is byte-identical to a run without --alignments-out."""
    from mini_parallel_amd import read_alignments
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=300, bgzf=True)
    names = [os.path.basename(f) for f in ds["files"]]
    for d in ("aln", "aln1", "scores", "scores_only"):
        (tmp_path / d).mkdir()
    r = run_cli(wgs_args(tmp_path, ds, scheme, "both") + ["--alignments-out", tmp_path / "aln", "--scores-out",
                                                          tmp_path / "scores"], wgs_env(tmp_path, "both"), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    r = run_cli(wgs_args(tmp_path, ds, scheme, "plain") + ["--scores-out", tmp_path / "scores_only"],
                wgs_env(tmp_path, "plain"), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    r = run_cli(wgs_args(tmp_path, ds, scheme, "s1") + ["--alignments-out", tmp_path / "aln1"],
                wgs_env(tmp_path, "s1", MSW_CLI_CIGAR_STRIDE="1"), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    multi_op = 0
    for name, b in zip(names, ds["batches"]):
        assert (tmp_path / "scores" / (name + ".scores")).read_bytes() == \
            (tmp_path / "scores_only" / (name + ".scores")).read_bytes()
        got, got1 = read_alignments(tmp_path / "aln" / (name + ".aln")), read_alignments(tmp_path / "aln1" / (name + ".aln"))
        assert len(got.score) == b.n_pairs == 300
        for p in range(b.n_pairs):
            read, win = b.reads[p, :b.read_len[p]], b.wins[p, :b.win_len[p]]
            want = ao.record(read, win, int(b.pos[p]), *SCHEMES[scheme])
            for x in (got, got1):
                have = (int(x.score[p]), int(x.end_i[p]), int(x.end_j[p]), int(x.ref_pos[p]), int(x.nm[p]),
                        [int(o) for o in x.cigars[p]])
                assert have == tuple(want), (name, p, ao.cigar_text(have[5]), ao.cigar_text(want.ops))
            multi_op += sum((o & 15) != ao.S for o in want.ops) > 1
    assert multi_op > 0      # the stride-1 run did trace reads again


def test_cli_alignments_out_file_switch(tmp_path):
    """Four BGZF lane files of 250 reads over the two workers of one GPU, in
    batches of 100 (two full, one of 50): a worker goes from one file to the
    next while a result set still holds the first file's last batch, and at
    MSW_CLI_CIGAR_STRIDE=1 that batch is traced again before it settles.
    Every .aln equals the oracle read for read, every .scores file equals its
    .aln's scores and end cells, and the checkpoint completes all four files."""
    import json
    from mini_parallel_amd import read_alignments
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=2, reads_per_lane=2, reads_per_file=250, bgzf=True)
    assert len(ds["files"]) == 4
    for d in ("aln", "scores"):
        (tmp_path / d).mkdir()
    r = run_cli(wgs_args(tmp_path, ds, "lin", "sw4") + ["--alignments-out", tmp_path / "aln", "--scores-out",
                                                        tmp_path / "scores"],
                wgs_env(tmp_path, "sw4", WGS_LANES="2", MSW_GFASTQ_BATCH="100", MSW_CLI_CIGAR_STRIDE="1"), tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    rec_t = np.dtype([("score", "<i4"), ("end_i", "<i2"), ("end_j", "<i2")])
    for f, b in zip(ds["files"], ds["batches"]):
        name = os.path.basename(f)
        got = read_alignments(tmp_path / "aln" / (name + ".aln"))
        assert len(got.score) == b.n_pairs == 250
        for p in range(b.n_pairs):
            want = ao.record(b.reads[p, :b.read_len[p]], b.wins[p, :b.win_len[p]], int(b.pos[p]), *LIN)
            have = (int(got.score[p]), int(got.end_i[p]), int(got.end_j[p]), int(got.ref_pos[p]), int(got.nm[p]),
                    [int(o) for o in got.cigars[p]])
            assert have == tuple(want), (name, p, ao.cigar_text(have[5]), ao.cigar_text(want.ops))
        scores = np.fromfile(tmp_path / "scores" / (name + ".scores"), dtype=rec_t)
        assert np.array_equal(scores["score"], got.score) and np.array_equal(scores["end_i"], got.end_i)
        assert np.array_equal(scores["end_j"], got.end_j)
    ck = json.load(open(tmp_path / "sw4" / "checkpoint_sw4.json"))
    assert ck["completed_files"] == ck["total_files"] == 4
    assert sorted(f["file_path"] for f in ck["files"] if f["completed"]) == sorted(ds["files"])
    assert all(f["total_reads"] == 250 for f in ck["files"])


def test_cli_alignments_out_refused(tmp_path):
    """The host reader, reads over 384 and windows over 4096 are refused with
    status 1 and one line, and no .aln appears."""
    from mini_parallel_amd.synthetic import write_wgs_dataset
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=True)
    (tmp_path / "aln").mkdir()
    base = wgs_args(tmp_path, ds, "lin", "r") + ["--alignments-out", tmp_path / "aln"]
    cases = [(base, {"MSW_GPU_INFLATE": "0"}, "host reader"),
             (base, {"MSW_MAX_READ_LEN": "385"}, "384"),
             (base[:base.index("--window") + 1] + ["4097"] + base[base.index("--window") + 2:], {}, "4096")]
    for args, extra, word in cases:
        r = run_cli(args, wgs_env(tmp_path, "r", **extra), tmp_path)
        assert r.returncode == 1 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert os.listdir(tmp_path / "aln") == []
    # gzip lane files go to the host reader as well
    ds = write_wgs_dataset(str(tmp_path / "wgs"), lanes=1, reads_per_lane=2, reads_per_file=20, bgzf=False)
    r = run_cli(base, wgs_env(tmp_path, "r"), tmp_path)
    assert r.returncode == 1 and "host reader" in r.stderr and os.listdir(tmp_path / "aln") == []
