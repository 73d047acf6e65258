"""tests/pileup_oracle.py against hand-worked pileups (include/msw.h, "Pileup").

The expected rows are written out by hand from the definition, so the oracle
the GPU tests compare against is itself pinned, independently of the kernels.
"""
import numpy as np
import pytest

import pileup_oracle as po

A, C, G, T, X, DEL, INS, REV = range(8)
GENOME = (b"ACGT" * 8)[:30]          # genome[pos] = "ACGT"[pos % 4]


def rows_of(expect, glen):
    """{pos: {channel: count}} -> counts[glen][8]"""
    out = po.new_counts(glen)
    for pos, chans in expect.items():
        for ch, v in chans.items():
            out[pos, ch] = v
    return out


# 3S5M2I4M1D6M2S at ref_pos 4: 22 read bases, 16 genome bases (4..19)
READ = b"TTT" + b"ACCTA" + b"GG" + b"CGTA" + b"GTACGT" + b"AA"
#              genome 4..8 is ACGTA: column 2 (pos 6) shows C against G
HAND = {4: {A: 1}, 5: {C: 1}, 6: {C: 1}, 7: {T: 1}, 8: {A: 1, INS: 1},        # I after pos 8 = g - 1 with g = 9
        9: {C: 1}, 10: {G: 1}, 11: {T: 1}, 12: {A: 1},
        13: {DEL: 1},
        14: {G: 1}, 15: {T: 1}, 16: {A: 1}, 17: {C: 1}, 18: {G: 1}, 19: {T: 1}}


@pytest.mark.parametrize("strand", [None, 0, 1])
def test_hand_worked_cigar_both_strands(strand):
    assert len(READ) == 22
    cig = po.cigar("3S5M2I4M1D6M2S")
    counts, used, skipped = po.pileup(GENOME, [READ], [22], [4], [4], [cig], None if strand is None else [strand])
    expect = {pos: dict(ch) for pos, ch in HAND.items()}
    if strand == 1:   # every M column, and only those, also counts in channel 7
        for pos, ch in expect.items():
            if DEL not in ch:
                ch[REV] = 1
    assert np.array_equal(counts, rows_of(expect, 30))
    assert (used, skipped) == (1, 0)
    d = po.depth(counts)
    assert d[4:20].tolist() == [1] * 16 and d.sum() == 16
    # the mismatch column is the only one where the reference base is in the minority
    s = po.summary(counts, GENOME, 1)
    assert s == {"covered": 16, "depth_sum": 16, "max_depth": 1, "minority_ref": 2}  # pos 6 and the deleted pos 13
    assert po.summary(counts, GENOME, 2)["minority_ref"] == 0


def test_n_and_lower_case_in_read_and_genome():
    genome = b"ANgTAC"
    # read bytes: N over A, N over N, g over g, t over T, 0 over A, C over C
    row = bytes([ord("N"), ord("N"), ord("g"), ord("t"), 0, ord("C")])
    counts, used, _ = po.pileup(genome, [row], [6], [0], [0], [po.cigar("6M")])
    assert used == 1
    assert np.array_equal(counts, rows_of({0: {X: 1}, 1: {X: 1}, 2: {X: 1}, 3: {X: 1}, 4: {X: 1}, 5: {C: 1}}, 6))
    # the reference channel of a genome byte that is not upper-case ACGT is 4
    s = po.summary(counts, genome, 1)
    assert s["minority_ref"] == 3     # pos 0 (A), 3 (T), 4 (A) show no reference base; pos 1, 2 have code 4 == X


def test_runs_cut_by_genome_end_position_zero_and_read_len():
    genome = b"ACGTACGT"
    # cut by the genome end: 6M at 5 counts columns 0..2 only; the D run after it lies outside
    counts, used, _ = po.pileup(genome, [b"CGTACG"], [6], [5], [0], [po.cigar("6M2D")])
    assert used == 1
    assert np.array_equal(counts, rows_of({5: {C: 1}, 6: {G: 1}, 7: {T: 1}}, 8))
    # a D run cut by the genome end, and an I run standing at g == glen marks glen - 1
    counts, _, _ = po.pileup(genome, [b"GTAA"], [4], [6], [0], [po.cigar("2M2I")])
    assert np.array_equal(counts, rows_of({6: {G: 1}, 7: {T: 1, INS: 1}}, 8))
    counts, _, _ = po.pileup(genome, [b"AC"], [2], [4], [0], [po.cigar("2M5D")])
    assert np.array_equal(counts, rows_of({4: {A: 1}, 5: {C: 1}, 6: {DEL: 1}, 7: {DEL: 1}}, 8))
    # position 0: an I run met at g == 0 would mark -1, which is outside
    counts, _, _ = po.pileup(genome, [b"TTAC"], [4], [0], [0], [po.cigar("2I2M")])
    assert np.array_equal(counts, rows_of({0: {A: 1}, 1: {C: 1}}, 8))
    # cut by read_len: the CIGAR speaks of 6 bases, the read has 4
    counts, _, _ = po.pileup(genome, [b"ACGTAC"], [4], [0], [0], [po.cigar("6M")])
    assert np.array_equal(counts, rows_of({0: {A: 1}, 1: {C: 1}, 2: {G: 1}, 3: {T: 1}}, 8))
    # ... also behind a soft clip: i starts at 3, one base is left
    counts, _, _ = po.pileup(genome, [b"TTTACG"], [4], [0], [0], [po.cigar("3S3M")])
    assert np.array_equal(counts, rows_of({0: {A: 1}}, 8))
    # past the end: the read counts as used, no column does
    counts, used, skipped = po.pileup(genome, [b"AC"], [2], [8], [0], [po.cigar("2M")])
    assert not counts.any() and (used, skipped) == (1, 0)


def test_insert_mark_sits_at_g_minus_one():
    genome = b"ACGTACGT"
    counts, _, _ = po.pileup(genome, [b"GTTTA"], [5], [2], [0], [po.cigar("2M2I1M")])
    assert np.array_equal(counts, rows_of({2: {G: 1}, 3: {T: 1, INS: 1}, 4: {A: 1}}, 8))
    # +1 per run, whatever its length; two runs in a row at one g both mark g - 1
    counts, _, _ = po.pileup(genome, [b"GTTTTT"], [6], [2], [0],
                             [np.array([po.op(1, "M"), po.op(2, "I"), po.op(2, "I"), po.op(1, "M")], np.uint32)])
    assert np.array_equal(counts, rows_of({2: {G: 1, INS: 2}, 3: {T: 1}}, 8))


def test_skipped_reads_and_unknown_ops():
    genome = b"ACGTACGT"
    rows = [b"ACGT"] * 6
    cig = po.cigar("4M")
    cigars = [cig, cig, cig, np.zeros(0, np.uint32), cig, None]
    counts, used, skipped = po.pileup(genome, rows, [4] * 6, [0, -1, 0, 0, 0, 0], [0, 0, -1, 0, 0, 0], cigars,
                                      mapq=[30, 60, 60, 60, 29, 60], min_mapq=30)
    assert (used, skipped) == (1, 5)
    assert np.array_equal(counts, rows_of({0: {A: 1}, 1: {C: 1}, 2: {G: 1}, 3: {T: 1}}, 8))
    # without a mapq array min_mapq is not looked at
    _, used, skipped = po.pileup(genome, rows[:1], [4], [0], [0], [cig], min_mapq=99)
    assert (used, skipped) == (1, 0)
    # an op code that is none of M I D S moves nothing
    odd = np.array([po.op(1, "M"), po.op(3, 3), po.op(2, 7), po.op(1, "M")], np.uint32)
    counts, _, _ = po.pileup(genome, [b"AC"], [2], [0], [0], [odd])
    assert np.array_equal(counts, rows_of({0: {A: 1}, 1: {C: 1}}, 8))


def test_summary_rule_at_half_and_one_below():
    genome = b"AAAAAA"
    counts = po.new_counts(6)
    counts[0, [A, C]] = [2, 2]          # 2 * 2 == 4: not a minority
    counts[1, [A, C]] = [1, 3]          # 2 * 1 < 4
    counts[2, [A, DEL]] = [2, 3]        # depth 5 with the deleted reads: 4 < 5
    counts[3, [A, C]] = [1, 2]          # depth 3: below min_depth 4
    counts[4, [INS, REV]] = [9, 9]      # neither channel is depth
    counts[5, A] = 7
    s = po.summary(counts, genome, 4)
    assert s == {"covered": 5, "depth_sum": 4 + 4 + 5 + 3 + 7, "max_depth": 7, "minority_ref": 2}
    assert po.summary(counts, genome, 3)["minority_ref"] == 3
    assert po.summary(counts, genome, 1)["minority_ref"] == 3
    with pytest.raises(AssertionError):
        po.summary(counts, genome, 0)
