"""tests/pileup_qual_oracle.py against tests/pileup_oracle.py and by hand: the
base-quality rules of include/msw.h ("Pileup", "Base qualities")."""
import numpy as np
import pytest

import pileup_oracle as po
import pileup_qual_oracle as pq

ACGT = np.frombuffer(b"ACGT", np.uint8)
HIGH = 33 + 40


def rand_records(rng, glen, n, stride=48):
    rows = ACGT[rng.integers(0, 4, (n, stride))].copy()
    rl = rng.integers(1, stride + 1, n).astype(np.uint16)
    ref = rng.integers(-5, glen + 3, n).astype(np.int64)
    nm = rng.integers(-1, 4, n).astype(np.int32)
    texts = ("%dM", "2S%dM", "3M2I%dM1D2M", "1M3D%dM")
    cigars = [po.cigar(texts[p % 4] % max(1, int(rl[p]) - 4)) if p % 11 else np.zeros(0, np.uint32) for p in range(n)]
    return rows, rl, ref, nm, cigars, rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 61, n).astype(np.uint8)


@pytest.mark.parametrize("seed", [1, 2])
def test_no_threshold_or_no_qualities_is_the_plain_oracle(seed):
    rng = np.random.default_rng(seed)
    glen = 120
    rows, rl, ref, nm, cigars, strand, mapq = rand_records(rng, glen, 80)
    quals = rng.integers(0, 256, rows.shape).astype(np.uint8)
    want = po.new_counts(glen)
    used, skipped = po.add(want, rows, rl, ref, nm, cigars, strand, mapq, 20)
    assert used > 20 and skipped > 5
    for kw in ({"quals": quals, "min_baseq": 0}, {"quals": None, "min_baseq": 30}, {}):
        got = po.new_counts(glen)
        assert pq.add(got, rows, rl, ref, nm, cigars, strand, mapq, 20, **kw) == (used, skipped, 0)
        assert np.array_equal(got, want)
    # and a threshold no byte fails against a full-width quality row
    got = po.new_counts(glen)
    assert pq.add(got, rows, rl, ref, nm, cigars, strand, mapq, 20, quals=np.full(rows.shape, 126, np.uint8),
                  min_baseq=93) == (used, skipped, 0)
    assert np.array_equal(got, want)


def one(genome, row, ref, cig, q, strand=None, min_baseq=20, qual_stride=None):
    row = np.frombuffer(row, np.uint8)
    return pq.pileup(genome, [row], [len(row)], [ref], [0], [po.cigar(cig)], None if strand is None else [strand], None,
                     0, [np.asarray(q, np.uint8)], qual_stride, min_baseq)


def test_a_low_quality_matching_column():
    q = [HIGH] * 6
    q[2] = 33 + 19
    counts, used, skipped, lowq = one(b"AACGTTAA", b"ACGTTA", 1, "6M", q)
    assert (used, skipped, lowq) == (1, 0, 1)
    want = po.new_counts(8)
    for pos, b in ((1, 0), (2, 1), (4, 3), (5, 3), (6, 0)):     # position 3 (the G) is gone
        want[pos, b] = 1
    assert np.array_equal(counts, want)


def test_a_low_quality_mismatching_column():
    q = [HIGH] * 4
    q[1] = 33
    counts, _, _, lowq = one(b"AAAAAA", b"ATAA", 1, "4M", q)
    assert lowq == 1
    want = po.new_counts(6)
    want[1, 0] = want[3, 0] = want[4, 0] = 1                      # the T at position 2 adds to no channel
    assert np.array_equal(counts, want) and counts[2].sum() == 0


def test_strand_1_first_base_as_given_is_the_last_column():
    """The row is the oriented read; quality byte 0 belongs to base 0 of the
    read as given, which is the LAST column of the oriented row."""
    q = [33 + 2] + [HIGH] * 4
    counts, _, _, lowq = one(b"CCACGTTCC", b"ACGTT", 2, "5M", q, strand=1)
    assert lowq == 1
    want = po.new_counts(9)
    for pos, b in ((2, 0), (3, 1), (4, 2), (5, 3)):
        want[pos, b] = 1
        want[pos, po.CH_REV] = 1
    assert np.array_equal(counts, want) and counts[6].sum() == 0  # neither channel 3 nor channel 7
    # with a soft clip in front the index still counts from the end of the read
    counts, _, _, lowq = one(b"CCACGTTCC", b"NNACGTT", 2, "2S5M", q + [HIGH] * 2, strand=1)
    assert lowq == 1 and counts[6].sum() == 0 and counts[5, 3] == 1
    # the same bytes on strand 0 drop the first column
    counts, _, _, lowq = one(b"CCACGTTCC", b"ACGTT", 2, "5M", q, strand=0)
    assert lowq == 1 and counts[2].sum() == 0 and counts[6, 3] == 1 and counts[:, po.CH_REV].sum() == 0


@pytest.mark.parametrize("n", [1, 20, 93])
def test_quality_byte_values(n):
    assert [pq.phred(b) for b in (0, 32, 33, 34, 126, 255)] == [0, 0, 0, 1, 93, 222]
    q = [0, 32, 33, 33 + n - 1, 33 + n, 126, 255]
    passes = [False, False, False, False, True, True, True]
    counts, _, _, lowq = one(b"A" * 7, b"A" * 7, 0, "7M", q, min_baseq=n)
    assert counts[:, 0].tolist() == [int(x) for x in passes]
    assert lowq == 4


def test_qual_stride_shorter_than_the_read():
    q = [HIGH] * 8
    counts, _, _, lowq = one(b"A" * 8, b"A" * 8, 0, "8M", q, qual_stride=5)
    assert counts[:, 0].tolist() == [1] * 5 + [0] * 3 and lowq == 3
    # strand 1: the bases without a quality byte are the first columns of the oriented row
    counts, _, _, lowq = one(b"A" * 8, b"A" * 8, 0, "8M", q, strand=1, qual_stride=5)
    assert counts[:, 0].tolist() == [0] * 3 + [1] * 5 and counts[:, po.CH_REV].tolist() == [0] * 3 + [1] * 5
    assert lowq == 3


def test_columns_outside_the_range_rules_are_not_low_quality():
    """Only a column that passes the range rules can be dropped and counted."""
    counts, _, _, lowq = one(b"AAAA", b"AAAAAAAA", 2, "8M", [33] * 8)     # six columns lie past the genome
    assert lowq == 2 and counts.sum() == 0
    row = np.frombuffer(b"AAAAAAAA", np.uint8)                              # read_len 3: five columns past the read
    assert pq.pileup(b"A" * 9, [row], [3], [0], [0], [po.cigar("8M")], None, None, 0, [[33] * 8], None, 20)[3] == 3
    # D and I runs are as before
    counts, _, _, lowq = one(b"AAAAAAAA", b"AAAAAA", 1, "2M2D1I3M", [33] * 6)
    assert lowq == 5 and counts[:, po.CH_DEL].tolist() == [0, 0, 0, 1, 1, 0, 0, 0] and counts[4, po.CH_INS] == 1
    assert counts[:, :5].sum() == 0
