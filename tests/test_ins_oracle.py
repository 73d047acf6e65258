"""tests/ins_oracle.py against rows worked out by hand from include/msw.h
("Pileup", "Inserted sequences")."""
import pytest

import ins_oracle as io
import pileup_oracle as po


def walk(row, ref, cig, glen=30, rl=None, **kw):
    return io.events(glen, [row], [len(row) if rl is None else rl], [ref], [0], [po.cigar(cig)], **kw)


CG = 1 | 2 << 2   # C then G


@pytest.mark.parametrize("row, cig, ref, kw, want", [
    # i = 8 after 3S5M, g = 15: the run CG follows base 14
    (b"TTTACGTACGTTAC", "3S5M2I4M", 10, {}, {14: [(2, 0, CG)]}),
    # the same read as given on strand 1: its reverse complement, flipped back
    (b"GTAACGTACGTAAA", "3S5M2I4M", 10, {"strand": [1], "flip": True}, {14: [(2, 0, CG)]}),
    # strand 1 in the device form: the row is already oriented
    (b"TTTACGTACGTTAC", "3S5M2I4M", 10, {"strand": [1]}, {14: [(2, 0, CG)]}),
    (b"ACGNTAC", "2M3I2M", 4, {}, {5: [(3, io.OTHER, 0)]}),
    (b"ACgTTAC", "2M3I2M", 4, {}, {5: [(3, io.OTHER, 0)]}),
    (b"A" + b"C" * 33 + b"G", "1M33I1M", 7, {}, {7: [(33, io.LONG, 0)]}),
    (b"A" + b"C" * 32 + b"N" * 2 + b"G", "1M34I1M", 7, {}, {7: [(34, io.LONG, 0)]}),        # the Ns are bases 32, 33: not looked at
    (b"A" + b"C" * 31 + b"N" * 3 + b"G", "1M34I1M", 7, {}, {7: [(34, io.LONG | io.OTHER, 0)]}),
    (b"A" + b"T" * 32 + b"G", "1M32I1M", 7, {}, {7: [(32, 0, (1 << 64) - 1)]}),
    (b"GGACG", "2I3M", 0, {}, {}),                                                         # g - 1 = -1
    (b"ACG", "2M1I", 28, {}, {29: [(1, 0, 2)]}),                                           # g - 1 = glen - 1
    (b"T", "1I", 30, {}, {29: [(1, 0, 3)]}),                                               # g = glen
    (b"T", "1I", 31, {}, {}),
    (b"ACGT", "2M2I", 3, {"rl": 3}, {4: [(2, io.OTHER, 0)]}),                              # base 3 is past read_len
    (b"ACGTAC", "1M1I1M2I1M", 3, {}, {3: [(1, 0, 1)], 4: [(2, 0, 3 | 0 << 2)]}),           # two runs: C, then TA
    (b"ACGTAC", "1M1I1M2I1M", 3, {"mapq": [9], "min_mapq": 10}, {}),
])
def test_events(row, cig, ref, kw, want):
    assert walk(row, ref, cig, **kw) == want


A, C, AA = (1, 0, 0), (1, 0, 1), (2, 0, 0)


@pytest.mark.parametrize("evs, want", [
    ([C, A, C], (3, 2, 2, 1, 1, 1)),                       # on count
    ([AA, C, AA, C], (4, 2, 2, 2, 1, 1)),                  # a tie on count: the shorter
    ([C, A, C, A], (4, 2, 2, 2, 1, 0)),                    # and on len: the smaller seq
    ([(3, io.OTHER, 0)] * 3 + [C], (4, 2, 1, 0, 1, 1)),    # flagged alleles count as alleles, never win
    ([(40, io.LONG, 0), (41, io.LONG, 0)], (2, 2, 0, 0, 0, 0)),
])
def test_vote(evs, want):
    assert io.table({7: evs, 2: [A]}) == [(2, 1, 1, 1, 0, 1, 0, 0), (7,) + want[:5] + (0, want[5])]
