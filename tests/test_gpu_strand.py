"""Both strands on the GPU (include/msw.h, "Both strands"): the reverse
complement kernel, both-strand scoring with its strand byte and oriented slab,
and the records of the oriented reads -- each bit-exact against
tests/strand_oracle.py.  Device outputs carry sentinel bytes around them.
"""
import ctypes

import numpy as np
import pytest

import aln_oracle as ao
import strand_oracle as so

pytestmark = pytest.mark.gpu

LIN = (2, -1, 0, 2, False)
AFF = (2, -1, 3, 1, True)
SCHEMES = {"lin": LIN, "aff": AFF}
ACGT = np.frombuffer(b"ACGT", np.uint8)
GUARD = 256
FILL = {np.int16: -21555, np.int32: 0x5EADBEEF, np.int64: 0x5EADBEEF5EADBEEF, np.uint8: 0xA5}


def scoring(scheme, coords=True):
    from mini_parallel_amd import Scoring
    m, x, go, ge, aff = scheme
    return Scoring(match=m, mismatch=x, gap_open=go, gap_extend=ge, affine=aff, want_coords=coords)


class Guarded:
    """A device array of n elements with GUARD sentinel elements before and
    after it; the payload starts as the sentinel too.  GUARD elements keep the
    payload 16-byte aligned.  The fill runs on torch's stream and the library
    on non-blocking streams of its own, which do not wait for it: the fill is
    finished here, before any library call can write the array."""

    def __init__(self, n, dtype):
        import torch
        self.n, self.dtype = n, dtype
        tdt = {np.int16: torch.int16, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}[dtype]
        self.t = torch.full((n + 2 * GUARD,), FILL[dtype], dtype=tdt, device="cuda:0")
        torch.cuda.synchronize()

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def get(self, view=None):
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == FILL[self.dtype]).all() and (a[GUARD + self.n:] == FILL[self.dtype]).all(), \
            "sentinels overwritten"
        a = a[GUARD:GUARD + self.n]
        return a.view(view) if view is not None else a

    def untouched(self):
        return (self.t.cpu().numpy() == FILL[self.dtype]).all()


def to_dev(a, as_type=None):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(as_type) if as_type is not None else a).to("cuda:0")


def round16(x):
    return max(16, (x + 15) // 16 * 16)


# ---------------------------------------------------------------------------
# 1. the reverse complement kernel
# ---------------------------------------------------------------------------
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 384, 1000]


def revcomp_case(n, stride):
    """n rows of `stride` bytes whose lengths run through LENS (those that
    fit), starting at 17 so that a single row is not the empty one.  Even rows
    are ACGT, odd rows run through all 256 byte values; bytes past a read are
    0xEE, which the kernel must not copy."""
    lens = [l for l in LENS if l <= stride]
    rl = np.array([lens[(k + 10) % len(lens)] for k in range(n)], np.uint16)
    rng = np.random.default_rng(1000 * n + stride)
    R = np.full((n, stride), 0xEE, np.uint8)
    nxt = 0          # odd rows continue one run through 0..255
    for k in range(n):
        L = int(rl[k])
        if k % 2 == 0:
            R[k, :L] = rng.choice(ACGT, L)
        else:
            R[k, :L] = (nxt + np.arange(L)) % 256
            nxt += L
    return R, rl


def revcomp_expected(R, rl, out_stride):
    out = np.zeros((R.shape[0], out_stride), np.uint8)
    for k in range(R.shape[0]):
        L = int(rl[k])
        out[k, :L] = np.frombuffer(so.revcomp(R[k, :L].tobytes()), np.uint8)
    return out


@pytest.mark.parametrize("stride", [1000, 160, 161, 256])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_revcomp_rows(gpu_ctx, n, stride):
    """Whole output slab against the table, padding included, for the input
    at base offsets 0..3 (dword and byte load arms both run; only the result
    is asserted)."""
    import torch
    R, rl = revcomp_case(n, stride)
    if n >= 63:
        assert len(set(R[np.arange(stride)[None, :] < rl[:, None]].tolist())) == 256
        assert {int(x) for x in rl} == {l for l in LENS if l <= stride}
    out_stride = round16(stride)
    want = revcomp_expected(R, rl, out_stride)
    d_rl = to_dev(rl, np.int16)
    for off in range(4):
        src = torch.zeros(off + R.size + 64, dtype=torch.uint8, device="cuda:0")
        src[off:off + R.size] = to_dev(R.ravel())
        out = Guarded(n * out_stride, np.uint8)
        gpu_ctx.revcomp_device(src.data_ptr() + off, d_rl.data_ptr(), stride, n, out.ptr, out_stride)
        gpu_ctx.synchronize()
        got = out.get().reshape(n, out_stride)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (off, bad[:4].tolist())


def test_revcomp_rejects_misaligned_output(gpu_ctx):
    import mini_parallel_amd as mpa
    R, rl = revcomp_case(4, 160)
    d_R, d_rl = to_dev(R), to_dev(rl, np.int16)
    out = Guarded(4 * 160 + 16, np.uint8)
    for ptr, ostride in ((out.ptr + 1, 160), (out.ptr + 8, 160), (out.ptr, 24), (out.ptr, 0)):
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.revcomp_device(d_R.data_ptr(), d_rl.data_ptr(), 160, 4, ptr, ostride)
        assert e.value.code == -1
    gpu_ctx.synchronize()
    assert out.untouched()          # nothing was launched
    gpu_ctx.revcomp_device(d_R.data_ptr(), d_rl.data_ptr(), 160, 0, 0, 160)      # n == 0: nothing to do


# ---------------------------------------------------------------------------
# 2. both-strand scoring
# ---------------------------------------------------------------------------
GENOME_LEN = 30011
TIE_POS, PAL_POS = 5000, 7000
_rng0 = np.random.default_rng(99)
TIE_X = _rng0.choice(ACGT, 75).astype(np.uint8).tobytes()             # genome[5000:5150] = X + rc(X)
_Y = _rng0.choice(ACGT, 40).astype(np.uint8).tobytes()
PAL = _Y + so.revcomp(_Y)                                             # its own reverse complement, at 7000


def the_genome():
    g = np.random.default_rng(2025).choice(ACGT, GENOME_LEN).astype(np.uint8)
    g[TIE_POS:TIE_POS + 150] = np.frombuffer(TIE_X + so.revcomp(TIE_X), np.uint8)
    g[PAL_POS:PAL_POS + 80] = np.frombuffer(PAL, np.uint8)
    return g


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
    return bytes(r[:m])


KINDS = ("fwd", "rev", "unrelated", "palindrome", "tie", "all_n", "empty", "edge", "rev")


def mixed_reads(B, seed, kinds=KINDS):
    """Reads of 75-250 bases against the window rule 2 x read length: forward
    and reverse reads with substitutions and indels, unrelated reads, the
    palindrome and the X + rc(X) tie, all-N and empty reads, and positions
    that are negative, past the end, or clipped at the genome end."""
    g = the_genome()
    rng = np.random.default_rng(seed)
    reads, pos, tags = [], [], []
    for k in range(B):
        kind = kinds[(k + 1) % len(kinds)] if B == 1 else kinds[k % len(kinds)]
        m = int(rng.integers(75, 251))
        p = int(rng.integers(0, GENOME_LEN - 600))
        src = g[p + int(rng.integers(0, m // 2)):][:m + 10]
        if kind == "fwd":
            r = mutated(rng, src, m)
        elif kind == "rev":
            r = so.revcomp(mutated(rng, src, m))
        elif kind == "unrelated":
            r = rng.choice(ACGT, m).astype(np.uint8).tobytes()
        elif kind == "palindrome":
            r, p = PAL, PAL_POS - 10
        elif kind == "tie":
            r, p = TIE_X, TIE_POS
        elif kind == "all_n":
            r = b"N" * m
        elif kind == "empty":
            r = b""
        else:
            sub = (k // len(kinds)) % 3
            p = (-1 - k, GENOME_LEN + k, GENOME_LEN - m)[sub]
            r = mutated(rng, g[max(0, min(p, GENOME_LEN - 1)) + 3:][:m + 10], m)
            r = so.revcomp(r) if k % 2 else r
        reads.append(r)
        pos.append(p)
        tags.append(kind)
    return g, reads, np.array(pos, np.int64), tags


class DevReads:
    def __init__(self, reads, pos, stride):
        self.rl = np.array([len(r) for r in reads], np.uint16)
        self.n, self.stride = len(reads), stride
        self.R = np.full((self.n, stride), 0xEE, np.uint8)      # bytes past a read are not the read
        for k, r in enumerate(reads):
            self.R[k, :len(r)] = np.frombuffer(r, np.uint8)
        self.pos = pos
        self.d_R, self.d_rl, self.d_pos = to_dev(self.R), to_dev(self.rl, np.int16), to_dev(pos)
        self.max_len = max(1, int(self.rl.max()))
        self.want = np.minimum(2 * self.rl.astype(np.int64), 4096).astype(np.uint16)     # window = 0


class StrandOut:
    def __init__(self, n, ostride, coords=True):
        self.n, self.ostride, self.coords = n, ostride, coords
        self.s, self.strand, self.oriented = Guarded(n, np.int32), Guarded(n, np.uint8), Guarded(n * ostride, np.uint8)
        self.ei = Guarded(n, np.int16) if coords else None
        self.ej = Guarded(n, np.int16) if coords else None

    def host(self):
        return (self.s.get(), self.ei.get() if self.coords else None, self.ej.get() if self.coords else None,
                self.strand.get(), self.oriented.get().reshape(self.n, self.ostride))


def enqueue_strands(ctx, genome, D, scheme, coords, ostride, stream=0):
    o = StrandOut(D.n, ostride, coords)
    ctx.align_reads_strands_device(genome, D.d_R.data_ptr(), D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), D.n, 0,
                                   D.max_len, o.s.ptr, o.strand.ptr, o.oriented.ptr, ostride, scoring(scheme, coords),
                                   o.ei.ptr if coords else 0, o.ej.ptr if coords else 0, 0, stream)
    return o


def oracle_scores(g, reads, D, scheme):
    wins = [ao.window_of(g, int(p), int(w)).tobytes() for p, w in zip(D.pos, D.want)]
    return so.score_batch(reads, wins, scheme), wins


def check_scores(o, exp, reads, tags, ostride, coords):
    s, ei, ej, strand, oriented = o.host()
    es, eei, eej, estrand = exp
    assert np.array_equal(strand, estrand), [(k, tags[k]) for k in np.flatnonzero(strand != estrand)[:5]]
    assert np.array_equal(s, es), [(k, tags[k]) for k in np.flatnonzero(s != es)[:5]]
    if coords:
        assert np.array_equal(ei, eei) and np.array_equal(ej, eej)
    want = np.zeros((len(reads), ostride), np.uint8)
    for k, r in enumerate(reads):
        want[k, :len(r)] = np.frombuffer(so.oriented(r, int(estrand[k])), np.uint8)
    bad = np.argwhere(oriented != want)
    assert bad.size == 0, bad[:4].tolist()
    for k, t in enumerate(tags):      # the contract's special cases, spelled out
        if t in ("palindrome", "tie"):
            assert strand[k] == 0 and s[k] == 2 * len(reads[k])
            if coords and t == "tie":
                assert ej[k] == len(reads[k]) - 1          # in the first half of X + rc(X)
        if t in ("all_n", "empty"):
            assert strand[k] == 0 and s[k] == 0 and (not coords or (ei[k], ej[k]) == (-1, -1))


# read stride per batch size: 16-byte rows, rows at no alignment, dword rows
STRIDES = {1: 256, 9: 251, 65: 252, 600: 256}


@pytest.mark.parametrize("coords", [False, True])
@pytest.mark.parametrize("scheme", ["lin", "aff"])
@pytest.mark.parametrize("B", [1, 9, 65, 600])
def test_strands_scoring(gpu_ctx, B, scheme, coords):
    g, reads, pos, tags = mixed_reads(B, 40 + B)
    if B >= 9:
        assert set(tags) == set(KINDS)
    D = DevReads(reads, pos, STRIDES[B])
    genome = gpu_ctx.load_genome(g)
    o = enqueue_strands(gpu_ctx, genome, D, SCHEMES[scheme], coords, 256)       # coords False: NULL end arrays
    gpu_ctx.synchronize()
    exp, _ = oracle_scores(g, reads, D, SCHEMES[scheme])
    if B >= 9:
        assert 0 < int(exp[3].sum()) < B
        assert (pos < 0).any() and (B < 27 or ((pos >= GENOME_LEN).any() and (pos + D.want > GENOME_LEN).any()))
    check_scores(o, exp, reads, tags, 256, coords)
    genome.close()


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_strands_long_pair(gpu_ctx, scheme):
    """A 1000-base reverse read in the batch: both passes run the long-pair kernel."""
    g, reads, pos, tags = mixed_reads(9, 77)
    rng = np.random.default_rng(5)
    reads.append(so.revcomp(mutated(rng, g[12000:13100], 1000)))
    pos = np.append(pos, 11900)
    tags.append("rev")
    D = DevReads(reads, pos, 1000)
    genome = gpu_ctx.load_genome(g)
    o = enqueue_strands(gpu_ctx, genome, D, SCHEMES[scheme], True, 1008)
    gpu_ctx.synchronize()
    exp, _ = oracle_scores(g, reads, D, SCHEMES[scheme])
    assert exp[3][-1] == 1 and exp[0][-1] > 1500
    check_scores(o, exp, reads, tags, 1008, True)
    genome.close()


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_forward_reads_equal_the_one_strand_call(gpu_ctx, scheme):
    from mini_parallel_amd._lib import OutT, check, lib
    g, reads, pos, tags = mixed_reads(65, 11, kinds=("fwd",))
    D = DevReads(reads, pos, 256)
    genome = gpu_ctx.load_genome(g)
    o = enqueue_strands(gpu_ctx, genome, D, SCHEMES[scheme], True, 256)
    s, ei, ej = Guarded(D.n, np.int32), Guarded(D.n, np.int16), Guarded(D.n, np.int16)
    out = OutT(s.ptr, ei.ptr, ej.ptr)
    check(lib().msw_align_reads_device(gpu_ctx.handle, ctypes.byref(scoring(SCHEMES[scheme]).to_c()), genome.handle,
                                       D.d_R.data_ptr(), D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), D.n, 0,
                                       D.max_len, ctypes.byref(out), None, None))
    gpu_ctx.synchronize()
    gs, gi, gj, strand, oriented = o.host()
    assert not strand.any()
    assert np.array_equal(gs, s.get()) and np.array_equal(gi, ei.get()) and np.array_equal(gj, ej.get())
    assert np.array_equal(oriented, np.where(np.arange(256)[None, :] < D.rl[:, None], D.R, 0))
    genome.close()


def test_two_streams_in_flight(gpu_ctx):
    from mini_parallel_amd._lib import check, lib
    streams = [ctypes.c_void_p() for _ in range(2)]
    for st in streams:
        check(lib().msw_stream_create(gpu_ctx.handle, ctypes.byref(st)))
    cases = [mixed_reads(600, 640), mixed_reads(65, 105)]
    genome = gpu_ctx.load_genome(cases[0][0])
    Ds = [DevReads(c[1], c[2], 256) for c in cases]
    outs = [enqueue_strands(gpu_ctx, genome, D, sch, True, 256, stream=st.value)
            for D, sch, st in zip(Ds, (AFF, LIN), streams)]
    gpu_ctx.synchronize()
    for (g, reads, pos, tags), D, o, sch in zip(cases, Ds, outs, (AFF, LIN)):
        check_scores(o, oracle_scores(g, reads, D, sch)[0], reads, tags, 256, True)
    for st in streams:
        check(lib().msw_stream_destroy(gpu_ctx.handle, st))
    genome.close()


def test_strands_argument_errors(gpu_ctx):
    import mini_parallel_amd as mpa
    g, reads, pos, tags = mixed_reads(9, 3)
    D = DevReads(reads, pos, 256)
    genome = gpu_ctx.load_genome(g)
    o = StrandOut(D.n, 256)
    call = lambda strand, oriented, ostride, n=D.n: gpu_ctx.align_reads_strands_device(
        genome, D.d_R.data_ptr(), D.d_rl.data_ptr(), D.stride, D.d_pos.data_ptr(), n, 0, D.max_len, o.s.ptr, strand,
        oriented, ostride, scoring(LIN), o.ei.ptr, o.ej.ptr)
    for args in ((0, o.oriented.ptr, 256), (o.strand.ptr, 0, 256), (o.strand.ptr, o.oriented.ptr + 4, 256),
                 (o.strand.ptr, o.oriented.ptr, 64), (o.strand.ptr, o.oriented.ptr, 264)):       # below max_read_len; not x16
        with pytest.raises(mpa.MswError) as e:
            call(*args)
        assert e.value.code == -1, args
    call(0, 0, 0, n=0)                      # n == 0 is fine
    gpu_ctx.synchronize()
    assert all(x.untouched() for x in (o.s, o.ei, o.ej, o.strand, o.oriented))
    genome.close()


# ---------------------------------------------------------------------------
# 3. records of the oriented reads
# ---------------------------------------------------------------------------
_RECS = {}


def record_case(scheme):
    if scheme not in _RECS:
        g, reads, pos, tags = mixed_reads(65, 4242)
        want = np.minimum(2 * np.array([len(r) for r in reads]), 4096)
        wins = [ao.window_of(g, int(p), int(w)).tobytes() for p, w in zip(pos, want)]
        recs = so.records(reads, wins, pos, SCHEMES[scheme])
        assert 10 < sum(r.strand for r in recs) < 55
        assert any(r.strand and any((o & 15) in (1, 2) for o in r.ops) for r in recs)     # a reverse read with an indel
        _RECS[scheme] = (g, reads, pos, tags, recs)
    return _RECS[scheme]


def check_record(p, rec, have):
    want = (rec.score, rec.end_i, rec.end_j, rec.strand, rec.ref_pos, rec.nm, rec.ops)
    assert have == want, (p, ao.cigar_text(have[6]), ao.cigar_text(rec.ops))


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_host_records(gpu_ctx, scheme):
    """msw_align_reads_strands with aln through its wrapper: chunks of 7, one
    chunk, and a first capacity of 1 that forces the retry."""
    g, reads, pos, tags, recs = record_case(scheme)
    D = DevReads(reads, pos, 256)
    genome = gpu_ctx.load_genome(g)
    for kw in ({"chunk_pairs": 7}, {}, {"chunk_pairs": 7, "cigar_cap": 1}):
        s, ei, ej, strand, ref, nm, cigars = gpu_ctx.align_reads_strands(genome, D.R, D.rl, pos, D.want,
                                                                         scoring(SCHEMES[scheme], False), trace=True, **kw)
        for p, r in enumerate(recs):
            check_record(p, r, (int(s[p]), int(ei[p]), int(ej[p]), int(strand[p]), int(ref[p]), int(nm[p]),
                                [int(o) for o in cigars[p]]))
            assert ao.read_bases(r.ops) == (len(reads[p]) if r.ops else 0)
    # scores only: coordinates as the scoring says
    s, ei, ej, strand = gpu_ctx.align_reads_strands(genome, D.R, D.rl, pos, D.want, scoring(SCHEMES[scheme], False),
                                                    chunk_pairs=16)
    assert ei is None and ej is None
    assert [int(x) for x in s] == [r.score for r in recs] and [int(x) for x in strand] == [r.strand for r in recs]
    s, ei, ej, strand = gpu_ctx.align_reads_strands(genome, D.R, D.rl, pos, D.want, scoring(SCHEMES[scheme], True))
    assert [(int(a), int(b)) for a, b in zip(ei, ej)] == [(r.end_i, r.end_j) for r in recs]
    genome.close()


@pytest.mark.parametrize("scheme", ["lin", "aff"])
def test_device_sequence_records(gpu_ctx, scheme):
    """strands -> msw_trace_reads_device -> msw_aln_pack_device, the last two on `oriented`."""
    g, reads, pos, tags, recs = record_case(scheme)
    D = DevReads(reads, pos, 252)
    n, ostride, cstride = D.n, 256, D.max_len + int(D.want.max())      # exact: no alignment has more ops
    genome = gpu_ctx.load_genome(g)
    o = enqueue_strands(gpu_ctx, genome, D, SCHEMES[scheme], True, ostride)
    si, sj, nc = Guarded(n, np.int16), Guarded(n, np.int16), Guarded(n, np.int32)
    rows = Guarded(n * cstride, np.int32)
    gpu_ctx.trace_reads_device(genome, o.oriented.ptr, D.d_rl.data_ptr(), ostride, D.d_pos.data_ptr(), n, 0, D.max_len,
                               o.s.ptr, o.ei.ptr, o.ej.ptr, si.ptr, sj.ptr, nc.ptr, rows.ptr, cstride,
                               scoring(SCHEMES[scheme]))
    cap = n * (cstride + 2)
    ref, nm, off = Guarded(n, np.int64), Guarded(n, np.int32), Guarded(n + 1, np.int32)
    ops, ovf = Guarded(cap, np.int32), Guarded(1, np.int32)
    gpu_ctx.aln_pack_device(genome, o.oriented.ptr, D.d_rl.data_ptr(), ostride, D.d_pos.data_ptr(), n, o.s.ptr,
                            o.ei.ptr, o.ej.ptr, si.ptr, sj.ptr, nc.ptr, rows.ptr, cstride, ref.ptr, nm.ptr, off.ptr,
                            ops.ptr, cap, ovf.ptr)
    gpu_ctx.synchronize()
    s, ei, ej, strand, _ = o.host()
    ref, nm, off, ops = ref.get(), nm.get(), off.get(np.uint32), ops.get(np.uint32)
    assert int(ovf.get()[0]) == 0
    for p, r in enumerate(recs):
        check_record(p, r, (int(s[p]), int(ei[p]), int(ej[p]), int(strand[p]), int(ref[p]), int(nm[p]),
                            [int(x) for x in ops[off[p]:off[p + 1]]]))
    genome.close()


def test_records_range_errors(gpu_ctx):
    import mini_parallel_amd as mpa
    g = the_genome()
    genome = gpu_ctx.load_genome(g)
    R = np.zeros((1, 400), np.uint8)
    R[0, :385] = g[100:485]
    one = lambda x, t: np.array([x], t)
    for rl, want in ((385, 300), (100, 4097)):
        with pytest.raises(mpa.MswError) as e:
            gpu_ctx.align_reads_strands(genome, R, one(rl, np.uint16), one(90, np.int64), one(want, np.uint16),
                                        scoring(LIN), trace=True)
        assert e.value.code == -2
    # the same read scores without records (the long-pair kernel), as in the one-strand call
    s, _, _, strand = gpu_ctx.align_reads_strands(genome, R, one(385, np.uint16), one(90, np.int64),
                                                  one(800, np.uint16), scoring(LIN, False))
    assert (int(s[0]), int(strand[0])) == (770, 0)
    genome.close()
