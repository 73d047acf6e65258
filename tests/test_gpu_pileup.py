"""Pileup on the GPU (msw_pileup_*; include/msw.h, "Pileup"): the device form
with hand-built records, the host form, the Python wrapper over map_reads and
align_reads_trace output -- all bit-exact against tests/pileup_oracle.py, the
column-by-column restatement (the kernels use the difference form)."""
import ctypes

import numpy as np
import pytest

import pileup_oracle as po
import strand_oracle as so

pytestmark = pytest.mark.gpu

ALPHABET = np.frombuffer(b"ACGTACGTACGTNacgtn\x00", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
SUMMARY_KEYS = ("covered", "depth_sum", "max_depth", "minority_ref")


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


class Records:
    """A batch of hand-built records: rows[n][stride] (the bytes the CIGARs
    refer to), lengths, positions, nm, cigars, optional strand and mapq."""

    def __init__(self, rows, rl, ref, nm, cigars, strand=None, mapq=None):
        self.rows = np.ascontiguousarray(rows, np.uint8)
        self.rl = np.asarray(rl, np.uint16)
        self.ref = np.asarray(ref, np.int64)
        self.nm = np.asarray(nm, np.int32)
        self.cigars = list(cigars)
        self.strand = None if strand is None else np.asarray(strand, np.uint8)
        self.mapq = None if mapq is None else np.asarray(mapq, np.uint8)
        self.n = len(self.cigars)

    def __add__(self, o):
        assert self.rows.shape[1] == o.rows.shape[1]
        cat = lambda a, b: None if a is None else np.concatenate([a, b])  # noqa: E731
        return Records(np.concatenate([self.rows, o.rows]), cat(self.rl, o.rl), cat(self.ref, o.ref),
                       cat(self.nm, o.nm), self.cigars + o.cigars, cat(self.strand, o.strand), cat(self.mapq, o.mapq))

    def packed(self):
        off = np.zeros(self.n + 1, np.uint32)
        off[1:] = np.cumsum([len(c) for c in self.cigars])
        ops = np.concatenate([np.asarray(c, np.uint32) for c in self.cigars] + [np.zeros(0, np.uint32)])
        return off, ops.astype(np.uint32)

    def oracle(self, counts, min_mapq=0):
        return po.add(counts, self.rows, self.rl, self.ref, self.nm, self.cigars, self.strand, self.mapq, min_mapq)


def add_device(pile, rec, min_mapq=0, stream=0, cap=None, shift=0):
    """One msw_pileup_add_device call on a fresh upload; returns what must
    stay alive until the stream has drained.  shift: the rows start that many
    bytes into their allocation (odd-aligned reads)."""
    import torch
    off, ops = rec.packed()
    flat = np.concatenate([np.zeros(shift, np.uint8), rec.rows.reshape(-1)])
    d_rows = to_dev(flat)
    keep = [d_rows, to_dev(rec.rl), to_dev(rec.ref), to_dev(rec.nm), to_dev(off),
            to_dev(np.concatenate([ops, np.zeros(4, np.uint32)])),
            None if rec.strand is None else to_dev(rec.strand), None if rec.mapq is None else to_dev(rec.mapq)]
    assert all(k is None or isinstance(k, torch.Tensor) for k in keep)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    pile.add_device(d_rows.data_ptr() + shift, ptr(keep[1]), rec.rows.shape[1], rec.n, ptr(keep[2]), ptr(keep[3]),
                    ptr(keep[4]), ptr(keep[5]), int(off[-1]) if cap is None else cap, ptr(keep[6]), ptr(keep[7]),
                    min_mapq, stream)
    return keep


def check(ctx, genome, batches, min_mapq=0, min_depth=1, **kw):
    """The pileup of `batches` on the device against the oracle: counts,
    summary, the read counters."""
    g = ctx.load_genome(genome)
    pile = ctx.pileup(g)
    want = po.new_counts(len(genome))
    used = skipped = 0
    keep = []
    for rec in batches:
        keep.append(add_device(pile, rec, min_mapq, **kw))
        u, s = rec.oracle(want, min_mapq)
        used, skipped = used + u, skipped + s
    pile.finish()
    got = pile.counts()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8, 0]].tolist(), want[bad[:8, 0]].tolist())
    s = pile.summary(min_depth)
    ws = po.summary(want, genome, min_depth)
    assert {k: s[k] for k in SUMMARY_KEYS} == ws
    assert (s["reads_used"], s["reads_skipped"]) == (used, skipped)
    pile.close()
    g.close()
    return got


def rand_genome(rng, glen, noisy=True):
    g = ACGT[rng.integers(0, 4, glen)].copy()
    if noisy and glen >= 8:
        for b in (ord("N"), ord("a"), ord("n"), ord("t")):
            g[rng.integers(0, glen, max(1, glen // 30))] = b
    return g.tobytes()


def read_over(rng, genome, ref, cig, rate=0.04):
    """Row bytes for a CIGAR at ref: the genome's own bytes over M columns
    (random where the column is outside), with substitutions -- some of them
    to the same code as the reference byte (N <-> n, a <-> N)."""
    g = np.frombuffer(genome, np.uint8)
    out, at = [], ref
    for word in cig:
        ln, kind = int(word) >> 4, int(word) & 15
        if kind == po.OP_M:
            idx = np.arange(at, at + ln)
            ok = (idx >= 0) & (idx < len(g))
            seg = ALPHABET[rng.integers(0, len(ALPHABET), ln)].copy()
            seg[ok] = g[idx[ok]]
            hit = rng.random(ln) < rate
            seg[hit] = ALPHABET[rng.integers(0, len(ALPHABET), int(hit.sum()))]
            out.append(seg)
            at += ln
        elif kind == po.OP_D:
            at += ln
        elif kind in (po.OP_I, po.OP_S):
            out.append(ALPHABET[rng.integers(0, len(ALPHABET), ln)])
    return np.concatenate(out + [np.zeros(0, np.uint8)])


def build(rng, genome, specs, stride=None, strand=False, mapq=False):
    """specs: (ref_pos, cigar text or ops, read_len or None = what the CIGAR consumes, nm)"""
    rows, rl, ref, nm, cigars = [], [], [], [], []
    for r, cig, length, m in specs:
        ops = po.cigar(cig) if isinstance(cig, str) else np.asarray(cig, np.uint32)
        row = read_over(rng, genome, r, ops)
        rows.append(row)
        rl.append(len(row) if length is None else length)
        ref.append(r)
        nm.append(m)
        cigars.append(ops)
    stride = stride or max(16, max(max(len(r) for r in rows), max(rl)))
    R = np.zeros((len(rows), stride), np.uint8)
    for p, row in enumerate(rows):
        R[p, :min(len(row), stride)] = row[:stride]
    n = len(rows)
    return Records(R, rl, ref, nm, cigars, rng.integers(0, 2, n) if strand else None,
                   rng.integers(0, 61, n) if mapq else None)


# ---------------------------------------------------------------------------
# 1. the device form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("glen", [1, 63, 64, 65, 300])
def test_read_and_run_lengths_at_every_edge(gpu_ctx, glen):
    """Reads of 1 .. 384 bases as one M run: starting at 0, ending exactly at
    glen (the difference array's last entry), crossing it, past it; D runs of
    1, 64, 65, 200 and an I mark at every edge."""
    rng = np.random.default_rng(glen)
    genome = rand_genome(rng, glen)
    specs = []
    for L in (1, 63, 64, 65, 150, 384):
        for ref in {0, max(0, glen - L), max(0, glen - L + 1), glen - 1, glen, glen + 5, glen // 2}:
            specs.append((ref, "%dM" % L, None, 0))
    for run in (1, 64, 65, 200):
        for ref in (0, max(0, glen - run - 2), glen // 3):
            specs.append((ref, "1M%dD1M" % run, None, run))
            specs.append((ref, "2S%dM3I%dM%dD2M1S" % (run, run, run), None, 3 + run))
            specs.append((ref, "%dM" % run, max(1, run - 1), 0))        # read_len one short of the CIGAR
    specs.append((0, "3I2M", None, 3))                                   # the mark would sit at -1
    specs.append((glen, "2I", None, 2))                                  # g == glen marks glen - 1
    specs.append((glen - 1, "1M1I1D1M", None, 2))
    specs.append((0, [po.op(1, "M"), po.op(5, 3), po.op(2, 9), po.op(1, "M")], None, 0))  # op codes that are skipped
    rec = build(rng, genome, specs, strand=True)
    got = check(gpu_ctx, genome, [rec])
    assert got[glen - 1].any()


def test_skipped_reads_and_min_mapq(gpu_ctx):
    rng = np.random.default_rng(5)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 200)), "4S60M2D30M", None, 2) for _ in range(40)]
    rec = build(rng, genome, specs, strand=True, mapq=True)
    rec.ref[3], rec.ref[4] = -1, -7
    rec.nm[5] = -1
    rec.cigars[6] = np.zeros(0, np.uint32)
    rec.mapq[7], rec.mapq[8], rec.mapq[9] = 29, 30, 0
    for min_mapq in (0, 30, 61):
        check(gpu_ctx, genome, [rec], min_mapq=min_mapq)
    # no mapq array: min_mapq is not looked at
    rec.mapq = None
    check(gpu_ctx, genome, [rec], min_mapq=50)
    # reads whose ops end past cigar_cap are skipped (the oracle: they have no ops)
    off, _ = rec.packed()
    cap = int(off[20])
    cut = Records(rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars[:20] + [np.zeros(0, np.uint32)] * 20, rec.strand)
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g)
    keep = add_device(pile, rec, cap=cap)
    pile.finish()
    want = po.new_counts(300)
    used, skipped = cut.oracle(want)
    assert np.array_equal(pile.counts(), want)
    s = pile.summary()
    assert (s["reads_used"], s["reads_skipped"]) == (used, skipped) and skipped >= 23
    del keep


def test_contention_600_identical_reads(gpu_ctx):
    rng = np.random.default_rng(6)
    genome = rand_genome(rng, 300, noisy=False)
    one = build(rng, genome, [(70, "3S70M2I40M5D35M", None, 9)], stride=150)
    # mismatches at fixed columns, so every read adds to the same words
    one.rows[0, 10] = ord("N")
    one.rows[0, 90] ^= 6
    rec = Records(np.repeat(one.rows, 600, 0), np.repeat(one.rl, 600), np.repeat(one.ref, 600), np.repeat(one.nm, 600),
                  one.cigars * 600, np.arange(600) % 3 == 0)
    got = check(gpu_ctx, genome, [rec], min_depth=4)
    assert got[:, :6].sum(axis=1).max() == 600 and got[100, 7] == 200


@pytest.mark.parametrize("n", [0, 1, 65, 600])
def test_batch_sizes_strides_and_alignment(gpu_ctx, n):
    rng = np.random.default_rng(n)
    genome = rand_genome(rng, 300)
    # stride 16 (short reads) and an odd stride with the rows starting at an odd address
    for stride, shift, L in ((16, 0, 16), (151, 1, 150), (151, 3, 97)):
        specs = [(int(rng.integers(0, 300)), "%dM" % L if p % 3 else "1S%dM1I%dM" % (L // 2 - 1, L - L // 2 - 1), None, 1)
                 for p in range(n)]
        if n == 0:
            rec = Records(np.zeros((0, stride), np.uint8), [], [], [], [])
        else:
            rec = build(rng, genome, specs, stride=stride, strand=True)
        check(gpu_ctx, genome, [rec], shift=shift)


def test_two_adds_equal_one_and_two_streams(gpu_ctx):
    from mini_parallel_amd._lib import check as ok, lib
    rng = np.random.default_rng(8)
    genome = rand_genome(rng, 300)
    mk = lambda n: build(rng, genome, [(int(rng.integers(0, 280)), "2S50M1D30M4I20M", None, 5) for _ in range(n)],  # noqa: E731
                         stride=112, strand=True, mapq=True)
    a, b = mk(70), mk(131)
    one = check(gpu_ctx, genome, [a + b], min_mapq=20)
    two = check(gpu_ctx, genome, [a, b], min_mapq=20)
    assert np.array_equal(one, two)
    # the two adds in flight on two streams
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        ok(lib().msw_stream_create(gpu_ctx.handle, ctypes.byref(s)))
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g)
    keep = [add_device(pile, r, 20, stream=s.value) for r, s in zip((a, b), streams)]
    gpu_ctx.synchronize()
    pile.finish()
    assert np.array_equal(pile.counts(), one)
    for s in streams:
        ok(lib().msw_stream_destroy(gpu_ctx.handle, s))
    del keep


def test_planes_layout(fresh_ctx, monkeypatch):
    """MSW_PILEUP_PLANES=1: the device counts as eight planes; everything public is unchanged."""
    monkeypatch.setenv("MSW_PILEUP_PLANES", "1")
    rng = np.random.default_rng(9)
    genome = rand_genome(rng, 301)
    rec = build(rng, genome, [(int(rng.integers(0, 290)), "1S40M3D20M2I30M", None, 5) for _ in range(90)], strand=True)
    g = fresh_ctx.load_genome(genome)
    pile = fresh_ctx.pileup(g)
    assert pile.counts_device()[1:] == (1, 301)
    pile.close()
    g.close()
    check(fresh_ctx, genome, [rec], min_depth=3)


def test_finish_order_and_errors(gpu_ctx, fresh_ctx):
    import mini_parallel_amd as mpa
    from mini_parallel_amd._lib import MSW_E_INVALID, MSW_E_RANGE, AlnT, PileupSummaryT, lib
    rng = np.random.default_rng(10)
    genome = rand_genome(rng, 100)
    rec = build(rng, genome, [(10, "50M", None, 0)] * 3, strand=True)
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g)
    ptr, ps, cs = pile.counts_device()
    assert ptr and (ps, cs) == (8, 1)

    def code(fn, *a, **k):
        with pytest.raises(mpa.MswError) as e:
            fn(*a, **k)
        return e.value.code

    assert code(pile.counts) == MSW_E_INVALID            # before finish
    assert code(pile.summary) == MSW_E_INVALID
    keep = add_device(pile, rec)
    # argument errors of the add forms
    off, ops = rec.packed()
    assert code(pile.add_device, 0, keep[1].data_ptr(), 64, 3, keep[2].data_ptr(), keep[3].data_ptr(),
                keep[4].data_ptr(), keep[5].data_ptr(), 3) == MSW_E_INVALID                       # rows NULL
    assert code(pile.add_device, keep[0].data_ptr(), keep[1].data_ptr(), 64, 3, 0, keep[3].data_ptr(),
                keep[4].data_ptr(), keep[5].data_ptr(), 3) == MSW_E_INVALID                       # ref_pos NULL
    assert code(pile.add_device, keep[0].data_ptr(), keep[1].data_ptr(), 64, 3, keep[2].data_ptr(), keep[3].data_ptr(),
                keep[4].data_ptr(), 0, 3) == MSW_E_INVALID                                        # cigar NULL, cap > 0
    assert code(pile.add_device, keep[0].data_ptr(), keep[1].data_ptr(), 0, 3, keep[2].data_ptr(), keep[3].data_ptr(),
                keep[4].data_ptr(), keep[5].data_ptr(), 3) == MSW_E_INVALID                       # stride 0
    assert code(pile.add_device, keep[0].data_ptr(), keep[1].data_ptr(), 64, 1 << 31, keep[2].data_ptr(),
                keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), 3) == MSW_E_RANGE
    assert code(pile.add_device, keep[0].data_ptr(), keep[1].data_ptr(), 64, 3, keep[2].data_ptr(), keep[3].data_ptr(),
                keep[4].data_ptr(), keep[5].data_ptr(), 3, min_mapq=256) == MSW_E_RANGE
    L = lib()
    assert L.msw_pileup_add_device(gpu_ctx.handle, pile.handle, keep[0].data_ptr(), keep[1].data_ptr(), 64, 3, None,
                                   None, None, 0, None) == MSW_E_INVALID                          # aln NULL
    assert L.msw_pileup_add_device(None, pile.handle, None, None, 64, 0, None, None, None, 0, None) == MSW_E_INVALID
    assert L.msw_pileup_add_device(gpu_ctx.handle, None, None, None, 64, 0, None, None, None, 0, None) == MSW_E_INVALID
    assert L.msw_pileup_finish(gpu_ctx.handle, None, None) == MSW_E_INVALID
    assert L.msw_pileup_counts(None, pile.handle, None) == MSW_E_INVALID
    assert L.msw_pileup_create(gpu_ctx.handle, g.handle, None) == MSW_E_INVALID
    h = ctypes.c_void_p()
    assert L.msw_pileup_create(gpu_ctx.handle, None, ctypes.byref(h)) == MSW_E_INVALID
    # the host form: offsets that decrease, ops past the capacity, a length past the stride
    bad_off = off.copy()
    bad_off[2] = 0
    nm, ref = rec.nm.copy(), rec.ref.copy()

    def host_add(off_, cap, rl=rec.rl, stride=rec.rows.shape[1]):
        aln = AlnT(ref.ctypes.data, nm.ctypes.data, off_.ctypes.data, ops.ctypes.data, cap, None)
        rl = np.ascontiguousarray(rl, np.uint16)
        return L.msw_pileup_add(gpu_ctx.handle, pile.handle, rec.rows.ctypes.data, rl.ctypes.data, stride, 3,
                                ctypes.byref(aln), None, None, 0, 0)

    assert host_add(bad_off, 3) == MSW_E_INVALID
    assert host_add(off, 2) == MSW_E_INVALID
    assert host_add(off, 3, rl=[50, 50, 65]) == MSW_E_INVALID
    # another context's genome, and a pileup used with another context
    other_g = fresh_ctx.load_genome(genome)
    assert L.msw_pileup_create(gpu_ctx.handle, other_g.handle, ctypes.byref(h)) == MSW_E_INVALID
    assert L.msw_pileup_finish(fresh_ctx.handle, pile.handle, None) == MSW_E_INVALID
    assert L.msw_pileup_summary(fresh_ctx.handle, pile.handle, 1, ctypes.byref(PileupSummaryT())) == MSW_E_INVALID
    other_g.close()
    # none of the refused calls added anything
    pile.finish()
    want = po.new_counts(100)
    rec.oracle(want)
    first = pile.counts()
    assert np.array_equal(first, want)
    pile.finish()                                        # a no-op
    assert np.array_equal(pile.counts(), first)
    assert code(add_device, pile, rec) == MSW_E_INVALID  # after finish
    assert code(pile.add, rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars) == MSW_E_INVALID
    assert code(pile.summary, 0) == MSW_E_INVALID        # min_depth 0
    assert L.msw_pileup_summary(gpu_ctx.handle, pile.handle, 1, None) == MSW_E_INVALID
    assert pile.summary(1)["reads_used"] == 3
    pile.close()
    g.close()
    # an empty genome
    g0 = gpu_ctx.load_genome(b"")
    p0 = gpu_ctx.pileup(g0)
    keep = add_device(p0, rec)
    p0.finish()
    assert p0.counts().shape == (0, 8)
    assert p0.summary() == {"covered": 0, "depth_sum": 0, "max_depth": 0, "minority_ref": 0, "reads_used": 3,
                            "reads_skipped": 0}
    p0.close()
    g0.close()


# ---------------------------------------------------------------------------
# 2. the host form and the Python wrapper
# ---------------------------------------------------------------------------
def test_host_form_against_device_form(gpu_ctx):
    """Reads as given plus strand bytes: the GPU takes the reverse complement
    of a strand-1 read; chunks of 7 and one chunk."""
    rng = np.random.default_rng(11)
    genome = rand_genome(rng, 400)
    specs = [(int(rng.integers(0, 380)), "3S40M2I30M4D20M5S" if p % 2 else "100M", None, 6) for p in range(45)]
    rec = build(rng, genome, specs, stride=112, strand=True, mapq=True)      # oriented rows
    dev = check(gpu_ctx, genome, [rec], min_mapq=10)
    given = rec.rows.copy()
    for p in range(rec.n):
        if rec.strand[p]:
            L = int(rec.rl[p])
            given[p, :L] = np.frombuffer(so.revcomp(rec.rows[p, :L].tobytes()), np.uint8)
    g = gpu_ctx.load_genome(genome)
    for chunk in (7, 0):
        pile = gpu_ctx.pileup(g)
        pile.add(given, rec.rl, rec.ref, rec.nm, rec.cigars, strand=rec.strand, mapq=rec.mapq, min_mapq=10,
                 chunk_reads=chunk)
        pile.finish()
        assert np.array_equal(pile.counts(), dev)
        pile.close()
    # without strand bytes the rows are taken as they are
    pile = gpu_ctx.pileup(g)
    pile.add(rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars, chunk_reads=16)
    pile.add(rec.rows[:0], rec.rl[:0], rec.ref[:0], rec.nm[:0], [])
    pile.finish()
    want = po.new_counts(400)
    po.add(want, rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars)
    assert np.array_equal(pile.counts(), want)
    pile.close()
    g.close()


def planted():
    """A 20 kbase genome with a planted exact repeat (reads inside it map
    ambiguously: mapq 0) and a diverged one, and reads of 1 .. 256 bases drawn
    from anywhere with 3 % substitutions, every other one reverse-complemented,
    plus an unrelated and an empty read."""
    rng = np.random.default_rng(12)
    g = bytearray(ACGT[rng.integers(0, 4, 20000)].tobytes())
    g[5000:5120] = g[12000:12120]
    g[7000:7150] = g[15000:15150]
    for p in range(7005, 7150, 15):
        g[p] = ACGT[(int(np.searchsorted(ACGT, g[p])) + 1) % 4]
    g = bytes(g)
    batch = [g[12010:12100], so.revcomp(g[5005:5110]), g[15000:15150], g[7000:7150], b"",
             ACGT[rng.integers(0, 4, 150)].tobytes(), g[:1], g[19999:], g[19900:], g[:40]]
    while len(batch) < 160:
        L = int(rng.integers(30, 257))
        at = int(rng.integers(0, len(g) - L))
        a = np.frombuffer(g[at:at + L], np.uint8).copy()
        hit = rng.random(L) < 0.03
        a[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        if len(batch) % 5 == 0:                     # a deletion and an insertion against the genome
            a = np.concatenate([a[:L // 3], a[L // 3 + 4:2 * L // 3], ACGT[rng.integers(0, 4, 3)], a[2 * L // 3:]])
        batch.append(so.revcomp(a.tobytes()) if len(batch) % 2 else a.tobytes())
    R = np.zeros((len(batch), 256), np.uint8)
    for p, r in enumerate(batch):
        R[p, :len(r)] = np.frombuffer(r, np.uint8)
    return g, batch, R, np.array([len(r) for r in batch], np.uint16)


def test_python_pileup_over_map_reads_and_trace(gpu_ctx):
    from mini_parallel_amd import Scoring
    g, batch, R, rl = planted()
    assert len(g) == 20000
    genome = gpu_ctx.load_genome(g)
    index = gpu_ctx.build_index(genome, 8)
    sc = Scoring(2, -1, 0, 2, False, True)
    s, ei, ej, strand, ref, nm, cigars, mq, sub, cand = gpu_ctx.map_reads(genome, index, R, rl, sc, mapq=True)
    assert strand.any() and (ref >= 0).sum() > 100 and (mq >= 30).any() and (mq < 30).any()
    oriented = [so.revcomp(r) if st else r for r, st in zip(batch, strand)]
    for min_mapq in (0, 30):
        pile = gpu_ctx.pileup(genome)
        pile.add(R, rl, ref, nm, cigars, strand=strand, mapq=mq, min_mapq=min_mapq, chunk_reads=64)
        pile.finish()
        want, used, skipped = po.pileup(g, oriented, rl, ref, nm, cigars, strand, mq, min_mapq)
        assert np.array_equal(pile.counts(), want)
        summ = pile.summary(2)
        assert {k: summ[k] for k in SUMMARY_KEYS} == po.summary(want, g, 2)
        assert (summ["reads_used"], summ["reads_skipped"]) == (used, skipped) and used > 50
        pile.close()
    # one strand: align_reads_trace at the mapped windows, rows as they are
    wp = np.where(ref >= 0, np.maximum(ref - 20, 0), -1).astype(np.int64)
    wl = np.full(len(batch), 300, np.uint16)
    s, ei, ej, ref1, nm1, cig1 = gpu_ctx.align_reads_trace(genome, R, rl, wp, wl, sc)
    pile = gpu_ctx.pileup(genome)
    pile.add(R, rl, ref1, nm1, cig1)
    pile.finish()
    want, used, skipped = po.pileup(g, batch, rl, ref1, nm1, cig1)
    assert np.array_equal(pile.counts(), want) and used > 50
    pile.close()
    index.close()
    genome.close()
