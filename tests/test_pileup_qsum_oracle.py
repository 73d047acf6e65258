"""tests/pileup_qsum_oracle.py against rows worked out by hand from include/msw.h
("Quality sums and weighted genotypes"), and against the two older oracles
where the rules overlap."""
import numpy as np

import pileup_oracle as po
import pileup_qsum_oracle as pqs
import pileup_qual_oracle as pq

GENOME = b"ACGTACGTACGTACGTACGTACGTACGTAC"          # 30 bases, genome[k] = "ACGT"[k % 4]
CIGAR = "3S5M2I4M1D6M2S"                            # 22 read bases
# M columns: read offset -> genome position, for ref_pos 4
COLUMNS = {3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 10: 9, 11: 10, 12: 11, 13: 12, 14: 14, 15: 15, 16: 16, 17: 17, 18: 18, 19: 19}


def oriented_row():
    """A row that shows the genome over its M columns, but for two mismatches:
    offset 5 (genome 6, a G) shows T and offset 16 (genome 16, an A) shows N."""
    row = bytearray(b"n" * 22)
    for o, g in COLUMNS.items():
        row[o] = GENOME[g]
    row[5], row[16] = ord("T"), ord("N")
    return np.frombuffer(bytes(row), np.uint8)


def run(strand, quals, min_baseq=0, qual_stride=None, genome=GENOME):
    return pqs.pileup(genome, [oriented_row()], [22], [4], [0], [po.cigar(CIGAR)], [quals],
                      strand=None if strand is None else [strand], qual_stride=qual_stride, min_baseq=min_baseq)


def test_both_strands_with_a_quality_per_column():
    quals = np.arange(34, 34 + 22, dtype=np.uint8)          # byte t has Phred t + 1
    for strand in (0, 1):
        counts, qsums, used, skipped, lowq = run(strand, quals)
        assert (used, skipped, lowq) == (1, 0, 0)
        want = np.zeros((30, 4), np.uint32)
        for o, g in COLUMNS.items():
            t = 21 - o if strand else o                     # the reversed index on strand 1
            if o == 5:
                want[g, 3] = t + 1                          # the T over a G
            elif o != 16:                                   # the N adds to no sum
                want[g, g % 4] = t + 1
        assert np.array_equal(qsums, want), strand
        assert int(counts[13, po.CH_DEL]) == 1 and int(counts[8, po.CH_INS]) == 1 and not qsums[13].any()
        assert int(counts[16, po.CH_OTHER]) == 1 and int(counts[6, 3]) == 1 and int(counts[6, 2]) == 0
        assert int(counts[:, po.CH_REV].sum()) == (15 if strand else 0)
    # strand None is strand 0
    assert np.array_equal(run(None, quals)[1], run(0, quals)[1])


def test_a_dropped_column_between_two_kept_ones():
    quals = np.full(22, 33 + 30, np.uint8)
    quals[11] = 33 + 7                                      # genome position 10 on strand 0
    counts, qsums, _, _, lowq = run(0, quals, min_baseq=8)
    assert lowq == 1 and not counts[10].any() and not qsums[10].any()
    assert int(qsums[9, 1]) == 30 and int(qsums[11, 3]) == 30 and int(counts[9, 1]) == 1
    counts, qsums, _, _, lowq = run(0, quals, min_baseq=7)
    assert lowq == 0 and int(qsums[10, 2]) == 7 and int(counts[10, 2]) == 1
    # on strand 1 byte 11 belongs to read offset 10, genome position 9
    counts, qsums, _, _, lowq = run(1, quals, min_baseq=8)
    assert lowq == 1 and not counts[9].any() and int(qsums[10, 2]) == 30


def test_quality_bytes_at_the_edges_of_the_phred_rule():
    for byte, value in ((0, 0), (32, 0), (33, 0), (126, 93)):
        quals = np.full(22, byte, np.uint8)
        counts, qsums, _, _, lowq = run(0, quals)
        assert lowq == 0 and int(counts[4, 0]) == 1 and int(qsums[4, 0]) == value, byte
        counts, qsums, _, _, lowq = run(0, quals, min_baseq=93)
        assert lowq == (0 if value == 93 else 15) and int(qsums[4, 0]) == (93 if value == 93 else 0)


def test_qual_stride_shorter_than_the_read_drops_the_columns_past_it_even_at_threshold_zero():
    quals = np.full(22, 33 + 40, np.uint8)
    counts, qsums, _, _, lowq = run(0, quals, qual_stride=12)
    # offsets 12 .. 19 (8 columns) have no quality byte
    assert lowq == 8 and not counts[11:20, :5].any() and int(qsums[10, 2]) == 40 and not qsums[11:].any()
    counts, qsums, _, _, lowq = run(1, quals, qual_stride=12)
    # strand 1: t = 21 - offset < 12 needs offset >= 10
    assert lowq == 5 and not counts[4:9, :5].any() and int(qsums[9, 1]) == 40 and int(qsums[19, 3]) == 40


def test_n_in_the_genome():
    genome = bytearray(GENOME)
    genome[7], genome[16] = ord("N"), ord("n")
    quals = np.full(22, 33 + 20, np.uint8)
    counts, qsums, _, _, _ = run(0, quals, genome=bytes(genome))
    # the read shows T over the N at 7: the sum goes to the read byte's channel, whatever the genome holds
    assert int(qsums[7, 3]) == 20 and int(counts[7, 3]) == 1 and not qsums[16].any() and int(counts[16, 4]) == 1


def test_agrees_with_the_threshold_oracle_on_counts_and_with_the_plain_one_without_a_threshold():
    rng = np.random.default_rng(3)
    genome = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 200))
    n = 60
    rows = rng.choice(np.frombuffer(b"ACGTNa", np.uint8), (n, 40))
    rl = rng.integers(1, 41, n)
    ref = rng.integers(-2, 190, n)
    nm = rng.integers(-1, 3, n)
    cigars = [po.cigar("2S10M1I12M3D15M") for _ in range(n)]
    strand = rng.integers(0, 2, n)
    quals = rng.integers(30, 80, (n, 40)).astype(np.uint8)
    for min_baseq in (0, 20, 45):
        counts, qsums, used, skipped, lowq = pqs.pileup(genome, rows, rl, ref, nm, cigars, quals, strand=strand,
                                                        min_baseq=min_baseq)
        if min_baseq:
            want = pq.pileup(genome, rows, rl, ref, nm, cigars, strand, quals=quals, min_baseq=min_baseq)
            assert np.array_equal(counts, want[0]) and (used, skipped, lowq) == want[1:]
        else:
            want = po.pileup(genome, rows, rl, ref, nm, cigars, strand)
            assert np.array_equal(counts, want[0]) and (used, skipped, lowq) == (want[1], want[2], 0)
        assert used > 30 and qsums.any()
        # a sum is at most 93 per counted observation and at least min_baseq
        c = counts[:, :4].astype(np.int64)
        assert (qsums <= 93 * c).all() and (qsums >= min_baseq * c).all()
