"""The base-quality threshold of the pileup on the GPU
(msw_pileup_add_qual[_device], msw_pileup_lowq_columns; include/msw.h,
"Pileup", "Base qualities"): the device form and the host form, each value
for value against tests/pileup_qual_oracle.py.

One batch of about 2000 hand-built records over a genome of 4096 bases is
built once and shared: read lengths at the lane split of a run (64 columns),
runs that end past the genome, soft clips in front, I and D runs between M
runs, about half the reads on strand 1, rows shorter than the stride, and
quality bytes at every edge of the Phred rule.  (An M run cannot start at a
negative coordinate: g starts at ref_pos >= 0 and only grows; reads with
ref_pos < 0 are in the batch and are skipped.)"""
import ctypes

import numpy as np
import pytest

import pileup_oracle as po
import pileup_qual_oracle as pq
import strand_oracle as so
from test_gpu_pileup import Records, build, rand_genome, to_dev

pytestmark = pytest.mark.gpu

GLEN = 4096
N = 20                                    # the threshold of the shared batch
STRIDE = 160
LENGTHS = (1, 63, 64, 65, 128, 129, 150)
QBYTES = np.array([0, 32, 33, 33 + N - 1, 33 + N, 74, 126, 255], np.uint8)


def cigar_for(L, kind):
    """A CIGAR that consumes exactly L read bases."""
    if kind == 0 or L < 12:
        return "%dM" % L
    if kind == 1:
        return "3S%dM" % (L - 3)
    if kind == 2:
        a = (L - 5) // 2
        return "2S%dM3I%dM" % (a, L - 5 - a)
    a = (L - 4) // 3
    return "1S%dM4D%dM3I%dM" % (a, a, L - 4 - 2 * a)


class Batch:
    pass


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(2024)
    b = Batch()
    b.genome = rand_genome(rng, GLEN)
    specs = []
    for p in range(2000):
        L = LENGTHS[p % len(LENGTHS)]
        where = p % 9
        if where == 0:
            ref = GLEN - L // 2 - 1           # the M runs end past glen
        elif where == 1:
            ref = max(0, GLEN - L)            # ... or exactly at it
        elif where == 2:
            ref = int(rng.integers(0, 4))
        else:
            ref = int(rng.integers(0, GLEN - 100))
        specs.append((ref, cigar_for(L, p % 4), None, 1))
    rec = build(rng, b.genome, specs, stride=STRIDE, strand=True, mapq=True)
    assert rec.rows.shape == (2000, STRIDE) and set(np.unique(rec.rl)) == set(LENGTHS)
    assert 800 < int(rec.strand.sum()) < 1200
    rec.ref[7], rec.ref[8], rec.nm[9] = -1, -40, -1     # skipped reads
    q = QBYTES[rng.integers(0, len(QBYTES), rec.rows.shape)]
    q[20] = 33 + N - 1                                   # a read that is all low quality (strand 0 and 1)
    q[21] = 33
    q[22] = 33 + N                                       # ... and reads that are all high
    q[23] = 126
    b.rec, b.quals = rec, q
    # the reads as given, for the host form: a strand-1 row is the reverse complement of the oriented one
    b.given = rec.rows.copy()
    for p in range(rec.n):
        if rec.strand[p]:
            L = int(rec.rl[p])
            b.given[p, :L] = np.frombuffer(so.revcomp(rec.rows[p, :L].tobytes()), np.uint8)
    b.want = {}
    return b


def oracle(b, qual_stride, min_baseq, min_mapq=10):
    """(counts, used, skipped, lowq) of the shared batch, computed once per (stride, threshold)."""
    key = (qual_stride, min_baseq, min_mapq)
    if key not in b.want:
        r = b.rec
        out = pq.pileup(b.genome, r.rows, r.rl, r.ref, r.nm, r.cigars, r.strand, r.mapq, min_mapq,
                        b.quals[:, :qual_stride], qual_stride, min_baseq)
        out[0].setflags(write=False)
        b.want[key] = out
    return b.want[key]


def upload(rec):
    off, ops = rec.packed()
    return {"rows": to_dev(rec.rows.reshape(-1)), "rl": to_dev(rec.rl), "ref": to_dev(rec.ref), "nm": to_dev(rec.nm),
            "off": to_dev(off), "ops": to_dev(np.concatenate([ops, np.zeros(4, np.uint32)])),
            "strand": to_dev(rec.strand), "mapq": to_dev(rec.mapq), "cap": int(off[-1])}


def add_device(pile, rec, d, quals_dev, qual_stride, min_baseq, min_mapq=10):
    pile.add_device(d["rows"].data_ptr(), d["rl"].data_ptr(), rec.rows.shape[1], rec.n, d["ref"].data_ptr(),
                    d["nm"].data_ptr(), d["off"].data_ptr(), d["ops"].data_ptr(), d["cap"], d["strand"].data_ptr(),
                    d["mapq"].data_ptr(), min_mapq, 0, 0 if quals_dev is None else quals_dev.data_ptr(), qual_stride,
                    min_baseq)


def compare(pile, want):
    counts, used, skipped, lowq = want
    assert pile.lowq_columns() == lowq                      # valid before the finish ...
    pile.finish()
    got = pile.counts()
    bad = np.argwhere(got != counts)
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8, 0]].tolist(), counts[bad[:8, 0]].tolist())
    s = pile.summary()
    assert (s["reads_used"], s["reads_skipped"]) == (used, skipped)
    assert pile.lowq_columns() == lowq                      # ... and after it


@pytest.mark.parametrize("qual_stride", [STRIDE, 100])
def test_device_form(gpu_ctx, batch, qual_stride):
    """qual_stride equal to the row stride, and smaller than the reads of 128, 129 and 150 bases."""
    want = oracle(batch, qual_stride, N)
    depth = int(po.depth(want[0]).sum())
    assert want[3] > depth // 10 and depth > 50000 and want[1] > 1500 and want[2] >= 3
    g = gpu_ctx.load_genome(batch.genome)
    pile = gpu_ctx.pileup(g)
    d = upload(batch.rec)
    q = to_dev(np.ascontiguousarray(batch.quals[:, :qual_stride]).reshape(-1))
    add_device(pile, batch.rec, d, q, qual_stride, N)
    compare(pile, want)
    pile.close()
    g.close()


@pytest.mark.parametrize("qual_stride,chunk", [(STRIDE, 0), (100, 333)])
def test_host_form(gpu_ctx, batch, qual_stride, chunk):
    """The reads as given: the GPU flips a strand-1 row, the quality rows stay in the order of the file."""
    r = batch.rec
    g = gpu_ctx.load_genome(batch.genome)
    pile = gpu_ctx.pileup(g)
    pile.add(batch.given, r.rl, r.ref, r.nm, r.cigars, strand=r.strand, mapq=r.mapq, min_mapq=10, chunk_reads=chunk,
             quals=batch.quals[:, :qual_stride], min_baseq=N)
    compare(pile, oracle(batch, qual_stride, N))
    pile.close()
    g.close()


def test_no_threshold_or_no_qualities_is_the_plain_add(gpu_ctx, batch):
    r = batch.rec
    g = gpu_ctx.load_genome(batch.genome)
    d = upload(r)
    q = to_dev(batch.quals.reshape(-1))
    got = []
    for quals_dev, min_baseq in ((None, 0), (q, 0), (None, N)):
        pile = gpu_ctx.pileup(g)
        add_device(pile, r, d, quals_dev, STRIDE, min_baseq)
        assert pile.lowq_columns() == 0
        pile.finish()
        got.append((pile.counts(), pile.summary()))
        pile.close()
    for min_baseq, quals in ((0, batch.quals), (N, None)):
        pile = gpu_ctx.pileup(g)
        pile.add(batch.given, r.rl, r.ref, r.nm, r.cigars, strand=r.strand, mapq=r.mapq, min_mapq=10, quals=quals,
                 min_baseq=min_baseq)
        assert pile.lowq_columns() == 0
        pile.finish()
        got.append((pile.counts(), pile.summary()))
        pile.close()
    for counts, summ in got[1:]:
        assert np.array_equal(counts, got[0][0]) and summ == got[0][1]
    want = po.new_counts(GLEN)
    po.add(want, r.rows, r.rl, r.ref, r.nm, r.cigars, r.strand, r.mapq, 10)
    assert np.array_equal(got[0][0], want)
    g.close()


def test_two_adds_with_different_thresholds(gpu_ctx, batch):
    r = batch.rec
    a, b = oracle(batch, STRIDE, N), oracle(batch, 100, 41)
    counts = a[0] + b[0]
    g = gpu_ctx.load_genome(batch.genome)
    pile = gpu_ctx.pileup(g)
    d = upload(r)
    q = to_dev(batch.quals.reshape(-1))
    q100 = to_dev(np.ascontiguousarray(batch.quals[:, :100]).reshape(-1))
    add_device(pile, r, d, q, STRIDE, N)
    add_device(pile, r, d, q100, 100, 41)
    compare(pile, (counts, a[1] + b[1], a[2] + b[2], a[3] + b[3]))
    assert b[3] > a[3]
    pile.close()
    g.close()


def test_threshold_range(gpu_ctx, batch):
    import mini_parallel_amd as mpa
    from mini_parallel_amd._lib import MSW_E_RANGE
    r = batch.rec
    g = gpu_ctx.load_genome(batch.genome)
    pile = gpu_ctx.pileup(g)
    d = upload(r)
    q = to_dev(batch.quals.reshape(-1))
    for form in ("device", "host"):
        with pytest.raises(mpa.MswError) as e:
            if form == "device":
                add_device(pile, r, d, q, STRIDE, 94)
            else:
                pile.add(batch.given, r.rl, r.ref, r.nm, r.cigars, strand=r.strand, quals=batch.quals, min_baseq=94)
        assert e.value.code == MSW_E_RANGE
    # 93 is accepted: only a byte of 126 or more passes
    add_device(pile, r, d, q, STRIDE, 93)
    compare(pile, oracle(batch, STRIDE, 93))
    n = ctypes.c_uint64()
    from mini_parallel_amd._lib import MSW_E_INVALID, lib
    assert lib().msw_pileup_lowq_columns(gpu_ctx.handle, pile.handle, None) == MSW_E_INVALID
    assert lib().msw_pileup_lowq_columns(gpu_ctx.handle, None, ctypes.byref(n)) == MSW_E_INVALID
    pile.close()
    g.close()
