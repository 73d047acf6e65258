"""Quality sums of a MSW_PILEUP_QSUM pileup on the GPU (msw_pileup_create_ex,
msw_pileup_add_qual[_device], msw_pileup_qsums*; include/msw.h, "Quality sums
and weighted genotypes"): counts, lowq_columns and qsums bit-exact against
tests/pileup_qsum_oracle.py, the column-by-column restatement (the kernel adds
quality differences along a run and folds them after a scan).

An M run cannot enter at g < 0: a read counts only with ref_pos >= 0 and g only
grows; reads with ref_pos < 0 are in the batches and are skipped."""
import ctypes

import numpy as np
import pytest

import pileup_oracle as po
import pileup_qsum_oracle as pqs
import strand_oracle as so
from test_gpu_pileup import Records, build, rand_genome, to_dev

pytestmark = pytest.mark.gpu

RUNS = (1, 63, 64, 65, 200)
PATTERNS = ("constant", "every", "seam", "ends")


def pattern_quals(rng, name, n, stride):
    """Quality rows whose changes fall where the pattern says, counted along the
    read as given; Phred 2 .. 41, so that a threshold of 30 drops some."""
    q = np.empty((n, stride), np.uint8)
    for p in range(n):
        a, b = (33 + int(v) for v in rng.choice(np.arange(2, 42), 2, replace=False))
        if name == "constant":
            q[p] = a
        elif name == "every":
            q[p] = 33 + 2 * rng.integers(1, 21, stride) + np.arange(stride) % 2      # neighbours differ in parity
        elif name == "seam":
            q[p, :64], q[p, 64:] = a, b            # between columns 63 and 64 of a run that starts at offset 0
        else:
            q[p] = a
            q[p, 0] = b
    return q


def upload(rec):
    off, ops = rec.packed()
    return {"rows": to_dev(rec.rows.reshape(-1)), "rl": to_dev(rec.rl), "ref": to_dev(rec.ref), "nm": to_dev(rec.nm),
            "off": to_dev(off), "ops": to_dev(np.concatenate([ops, np.zeros(4, np.uint32)])),
            "strand": None if rec.strand is None else to_dev(rec.strand),
            "mapq": None if rec.mapq is None else to_dev(rec.mapq), "cap": int(off[-1])}


def add_device(pile, rec, d, quals_dev, qual_stride, min_baseq, min_mapq=0, stream=0, n=None):
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    pile.add_device(d["rows"].data_ptr(), d["rl"].data_ptr(), rec.rows.shape[1], rec.n if n is None else n,
                    d["ref"].data_ptr(), d["nm"].data_ptr(), d["off"].data_ptr(), d["ops"].data_ptr(), d["cap"],
                    ptr(d["strand"]), ptr(d["mapq"]), min_mapq, stream, ptr(quals_dev), qual_stride, min_baseq)


def oracle(genome, rec, quals, qual_stride, min_baseq, min_mapq=0):
    return pqs.pileup(genome, rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars, quals[:, :qual_stride], rec.strand, rec.mapq,
                      min_mapq, qual_stride, min_baseq)


def compare(pile, want):
    counts, qsums, used, skipped, lowq = want
    assert pile.lowq_columns() == lowq
    pile.finish()
    got, gq = pile.counts(), pile.qsums()
    bad = np.argwhere(got != counts)
    assert bad.size == 0, ("counts", bad[:8].tolist(), got[bad[:8, 0]].tolist(), counts[bad[:8, 0]].tolist())
    bad = np.argwhere(gq != qsums)
    assert bad.size == 0, ("qsums", bad[:8].tolist(), gq[bad[:8, 0]].tolist(), qsums[bad[:8, 0]].tolist())
    s = pile.summary()
    assert (s["reads_used"], s["reads_skipped"]) == (used, skipped)
    return got, gq


def run_device(ctx, genome, rec, quals, qual_stride, min_baseq, min_mapq=0, plain_too=True):
    """The device form on a flagged pileup against the oracle; an unflagged
    pileup fed the same records gives the same counts."""
    g = ctx.load_genome(genome)
    pile = ctx.pileup(g, qsum=True)
    d = upload(rec)
    q = to_dev(np.ascontiguousarray(quals[:, :qual_stride]).reshape(-1))
    add_device(pile, rec, d, q, qual_stride, min_baseq, min_mapq)
    want = oracle(genome, rec, quals, qual_stride, min_baseq, min_mapq)
    got, gq = compare(pile, want)
    pile.close()
    # min_baseq 0 on an unflagged pileup is the plain add, which knows no qual_stride rule
    if plain_too and (min_baseq > 0 or qual_stride >= int(rec.rl.max())):
        plain = ctx.pileup(g)
        add_device(plain, rec, d, q, qual_stride, min_baseq, min_mapq)
        plain.finish()
        assert np.array_equal(plain.counts(), got)
        plain.close()
    g.close()
    return want


def run_specs(glen):
    specs = []
    for L in RUNS:
        for ref in {0, max(0, glen - L), max(0, glen - L // 2 - 1), glen // 3}:
            specs.append((ref, "%dM" % L, None, 0))                       # whole, ending at glen, cut by glen
        specs.append((0, "%dM" % L, max(1, L - 1), 0))                    # cut by read_len
        specs.append((1, "%dM" % L, max(1, L // 2), 0))
        specs.append((2, "3S%dM2I%dM1D%dM2S" % (L, L, L), None, 3))       # runs that start at read offsets 3, L + 5, ...
    specs.append((-1, "20M", None, 0))
    specs.append((-300, "20M", None, 0))
    return specs


@pytest.mark.parametrize("name", PATTERNS)
def test_quality_patterns_over_run_lengths(gpu_ctx, name):
    rng = np.random.default_rng(PATTERNS.index(name))
    glen = 300
    genome = rand_genome(rng, glen)
    rec = build(rng, genome, run_specs(glen) * 2, stride=640, strand=True)
    rec.strand[:len(rec.strand) // 2], rec.strand[len(rec.strand) // 2:] = 0, 1    # every spec on both strands
    quals = pattern_quals(rng, name, rec.n, 640)
    if name == "ends":
        for p in range(rec.n):
            quals[p, int(rec.rl[p]) - 1] = quals[p, 0]
    for min_baseq in (0, 30):
        want = run_device(gpu_ctx, genome, rec, quals, 640, min_baseq)
        assert want[1].any() and want[3] == 4 and (min_baseq == 0) == (want[4] == 0)


@pytest.mark.parametrize("glen", [1, 2, 63, 65, 257])
def test_small_genomes_and_reads_of_1_to_384(gpu_ctx, glen):
    rng = np.random.default_rng(100 + glen)
    genome = rand_genome(rng, glen)
    specs = []
    for L in (1, 2, 63, 64, 65, 150, 384):
        for ref in {0, max(0, glen - L), glen - 1, glen, glen // 2}:
            specs.append((ref, "%dM" % L, None, 0))
    specs.append((glen - 1, "1M1I1D1M", None, 2))
    rec = build(rng, genome, specs, stride=384, strand=True)
    quals = (33 + rng.integers(0, 42, (rec.n, 384))).astype(np.uint8)
    want = run_device(gpu_ctx, genome, rec, quals, 384, 20)
    assert want[1][glen - 1].any()


def dropped_quals(rng, rec, stride):
    """High everywhere, then low (Phred 5) columns: the first, the last, two
    adjacent ones, every second, and all of a read, by read index."""
    q = np.full((rec.n, stride), 33 + 40, np.uint8)
    for p in range(rec.n):
        L, kind = int(rec.rl[p]), p % 6
        if kind == 0:
            q[p, 0] = 38
        elif kind == 1:
            q[p, L - 1] = 38
        elif kind == 2:
            q[p, L // 2:L // 2 + 2] = 38
        elif kind == 3:
            q[p, 0:L:2] = 38
        elif kind == 4:
            q[p] = 38
        else:
            q[p, :L] = 33 + rng.integers(0, 94, L)         # bytes up to 126
    q[0, :4] = (0, 32, 33, 126)
    return q


@pytest.mark.parametrize("min_baseq", [0, 30, 93])
def test_dropped_columns_first_last_adjacent_all(gpu_ctx, min_baseq):
    rng = np.random.default_rng(7)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 280)), c, None, 1) for c in ("70M", "5M", "2S30M3I64M2D40M1S", "130M") for _ in range(12)]
    rec = build(rng, genome, specs, stride=160, strand=True, mapq=True)
    quals = dropped_quals(rng, rec, 160)
    want = run_device(gpu_ctx, genome, rec, quals, 160, min_baseq, min_mapq=10)
    assert (want[4] > 0) == (min_baseq > 0) and want[3] > 0
    if min_baseq == 93:
        assert 0 < int(want[1].sum()) and int(want[1].max()) % 93 == 0      # only bytes of 126 pass


@pytest.mark.parametrize("qual_stride", [101, 64, 1])
def test_qual_stride_shorter_than_the_reads_and_odd(gpu_ctx, qual_stride):
    rng = np.random.default_rng(8)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 200)), c, None, 1) for c in ("150M", "3S100M2D47M", "64M") for _ in range(10)]
    rec = build(rng, genome, specs, stride=152, strand=True)
    quals = (33 + rng.integers(10, 42, (rec.n, 152))).astype(np.uint8)
    for min_baseq in (0, 25):
        want = run_device(gpu_ctx, genome, rec, quals, qual_stride, min_baseq)
        assert want[4] > 0                                   # the columns past the stride are dropped at threshold 0 too


def test_host_form_with_strand_1_reads_as_given(gpu_ctx):
    rng = np.random.default_rng(9)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 260)), c, None, 1) for c in ("70M", "2S30M3I64M2D40M1S", "130M") for _ in range(20)]
    rec = build(rng, genome, specs, stride=160, strand=True, mapq=True)
    quals = (33 + rng.integers(0, 42, (rec.n, 160))).astype(np.uint8)
    given = rec.rows.copy()
    for p in range(rec.n):
        if rec.strand[p]:
            L = int(rec.rl[p])
            given[p, :L] = np.frombuffer(so.revcomp(rec.rows[p, :L].tobytes()), np.uint8)
    g = gpu_ctx.load_genome(genome)
    for min_baseq, qual_stride, chunk in ((0, 160, 0), (20, 160, 7), (20, 99, 0)):
        pile = gpu_ctx.pileup(g, qsum=True)
        pile.add(given, rec.rl, rec.ref, rec.nm, rec.cigars, strand=rec.strand, mapq=rec.mapq, min_mapq=10,
                 chunk_reads=chunk, quals=quals[:, :qual_stride], min_baseq=min_baseq)
        compare(pile, oracle(genome, rec, quals, qual_stride, min_baseq, 10))
        pile.close()
    g.close()
    # the device form over the oriented rows gives the same
    run_device(gpu_ctx, genome, rec, quals, 160, 20, min_mapq=10)


def test_600_reads_on_one_locus_and_n_from_0_to_600(gpu_ctx):
    rng = np.random.default_rng(10)
    genome = rand_genome(rng, 300)
    one = build(rng, genome, [(40, "5S100M2D45M", None, 2)], stride=152, strand=True)
    rec = Records(np.repeat(one.rows, 600, 0), np.repeat(one.rl, 600), np.repeat(one.ref, 600), np.repeat(one.nm, 600),
                  one.cigars * 600, rng.integers(0, 2, 600))
    quals = (33 + rng.integers(0, 42, (600, 152))).astype(np.uint8)
    want = run_device(gpu_ctx, genome, rec, quals, 152, 15)
    assert int(want[0][:, :6].sum(axis=1).max()) > 400
    g = gpu_ctx.load_genome(genome)
    d = upload(rec)
    q = to_dev(quals.reshape(-1))
    for n in (0, 1, 3, 4, 5, 255, 257):
        pile = gpu_ctx.pileup(g, qsum=True)
        add_device(pile, rec, d, q, 152, 15, n=n)
        part = Records(rec.rows[:n], rec.rl[:n], rec.ref[:n], rec.nm[:n], rec.cigars[:n], rec.strand[:n])
        compare(pile, oracle(genome, part, quals[:n], 152, 15))
        pile.close()
    g.close()


def test_two_adds_on_two_streams_equal_one_and_finish_twice(gpu_ctx):
    from mini_parallel_amd._lib import check as ok, lib
    rng = np.random.default_rng(11)
    genome = rand_genome(rng, 300)
    specs = [(int(rng.integers(0, 260)), c, None, 1) for c in ("70M", "2S30M3I64M2D40M1S", "130M") for _ in range(30)]
    a = build(rng, genome, specs, stride=160, strand=True)
    b = build(rng, genome, specs, stride=160, strand=True)
    qa = (33 + rng.integers(0, 42, (a.n, 160))).astype(np.uint8)
    qb = (33 + rng.integers(0, 42, (b.n, 160))).astype(np.uint8)
    want = run_device(gpu_ctx, genome, a + b, np.concatenate([qa, qb]), 160, 12)
    g = gpu_ctx.load_genome(genome)
    pile = gpu_ctx.pileup(g, qsum=True)
    streams = [ctypes.c_void_p() for _ in range(2)]
    for s in streams:
        ok(lib().msw_stream_create(gpu_ctx.handle, ctypes.byref(s)))
    keep = []
    for r, q, s in zip((a, b), (qa, qb), streams):
        keep.append((upload(r), to_dev(q.reshape(-1))))
        add_device(pile, r, keep[-1][0], keep[-1][1], 160, 12, stream=s.value)
    ok(lib().msw_synchronize(gpu_ctx.handle))
    got, gq = compare(pile, want)
    pile.finish()                                            # a second finish is a no-op
    assert np.array_equal(pile.counts(), got) and np.array_equal(pile.qsums(), gq)
    ptr, ps, cs = pile.qsums_device()
    assert ptr and (ps, cs) == (4, 1)
    for s in streams:
        ok(lib().msw_stream_destroy(gpu_ctx.handle, s))
    pile.close()
    g.close()


def test_error_paths(gpu_ctx):
    import mini_parallel_amd as mpa
    from mini_parallel_amd._lib import MSW_E_INVALID, MSW_E_RANGE, lib
    L = lib()
    rng = np.random.default_rng(12)
    genome = rand_genome(rng, 100)
    rec = build(rng, genome, [(3, "40M", None, 0), (20, "40M", None, 0)], stride=48, strand=True)
    quals = np.full((2, 48), 70, np.uint8)
    g = gpu_ctx.load_genome(genome)
    h = ctypes.c_void_p()
    for flags in (2, 3, 0x80000000):
        assert L.msw_pileup_create_ex(gpu_ctx.handle, g.handle, flags, ctypes.byref(h)) == MSW_E_INVALID and not h.value
    assert L.msw_pileup_create_ex(gpu_ctx.handle, g.handle, 1, None) == MSW_E_INVALID
    assert L.msw_pileup_create_ex(gpu_ctx.handle, g.handle, 0, ctypes.byref(h)) == 0 and h.value     # msw_pileup_create
    L.msw_pileup_destroy(h)
    d = upload(rec)
    q = to_dev(quals.reshape(-1))
    pile = gpu_ctx.pileup(g, qsum=True)
    assert pile.qsum
    for kw in (dict(), dict(min_baseq=20)):                  # the plain add, and an add without qualities
        with pytest.raises(mpa.MswError) as e:
            pile.add(rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars, **kw)
        assert e.value.code == MSW_E_INVALID and "quals" in str(e.value)
        with pytest.raises(mpa.MswError) as e:
            add_device(pile, rec, d, None, 48, kw.get("min_baseq", 0))
        assert e.value.code == MSW_E_INVALID
    with pytest.raises(mpa.MswError) as e:
        add_device(pile, rec, d, q, 48, 94)
    assert e.value.code == MSW_E_RANGE
    with pytest.raises(mpa.MswError) as e:                   # before the finish
        pile.qsums()
    assert e.value.code == MSW_E_INVALID and "finish" in str(e.value)
    assert pile.qsums_device()[0]                            # valid at any time
    add_device(pile, rec, d, q, 48, 0)
    compare(pile, oracle(genome, rec, quals, 48, 0))
    assert L.msw_pileup_qsums(gpu_ctx.handle, pile.handle, None) == MSW_E_INVALID
    with pytest.raises(mpa.MswError):                        # finished: no more reads
        add_device(pile, rec, d, q, 48, 0)
    pile.close()
    # an unflagged pileup has no sums, before or after its finish, and still takes the plain add
    plain = gpu_ctx.pileup(g)
    assert not plain.qsum
    plain.add(rec.rows, rec.rl, rec.ref, rec.nm, rec.cigars)
    for finished in (False, True):
        for f in (plain.qsums, plain.qsums_device):
            with pytest.raises(mpa.MswError) as e:
                f()
            assert e.value.code == MSW_E_INVALID and "MSW_PILEUP_QSUM" in str(e.value)
        plain.finish()
    plain.close()
    empty = gpu_ctx.load_genome(b"")
    pile = gpu_ctx.pileup(empty, qsum=True)
    pile.finish()
    assert pile.qsums().shape == (0, 4)
    pile.close()
    empty.close()
    g.close()
