"""The restatement of read placement (tests/seed_oracle.py) against cases
worked by hand from the contract in include/msw.h ("Placing reads"), and the
placement condition on the synthetic lane data.  CPU only."""
import numpy as np
import pytest

import seed_oracle as sd
import strand_oracle as so

# position : k-mer (k = 4)
#  0 ACGT  1 CGTA  2 GTAC  3 TACG  4 ACGG  5 CGGA  6 GGAC  7 GACG  8 ACGT  9 CGTA  10 GTAC  11 TACT  12 ACTT
TWO_LOCI = b"ACGTACGGACGTACTT"
#  0 AACC  1 ACCG  2 CCGG  3 CGGT  4 GGTT  5 GTTA  6 TTAC  7 TACG  8 ACGA  9 CGAT  10 GATC  11 ATCA  12 TCAG
UNIQUE = b"AACCGGTTACGATCAG"


def test_codes():
    code, coded = sd.codes(b"ACGTNACGa", 4)
    # ACGT = 0*64 + 1*16 + 2*4 + 3 = 27; the four k-mers over N and the one over 'a' have no code
    assert coded.tolist() == [True, False, False, False, False, False]
    assert code[0] == 27
    assert sd.codes(b"ACG", 4)[0].shape == (0,)
    assert sd.codes(b"TTTT", 4)[0].tolist() == [255]


def test_index_by_hand():
    ix = sd.Index(TWO_LOCI, 4, 64)
    by_code = {int(c): ix.pos[s:s + n].tolist() for c, s, n in zip(ix.ucode, ix.start, ix.count)}
    code = lambda s: int(sd.codes(s, 4)[0][0])
    assert by_code[code(b"ACGT")] == [0, 8] and by_code[code(b"CGTA")] == [1, 9] and by_code[code(b"GTAC")] == [2, 10]
    assert by_code[code(b"TACG")] == [3] and len(by_code) == 10 and ix.pos.shape[0] == 13
    off = sd.dense_off(ix)
    assert off.shape == (257,) and off[0] == 0 and off[256] == 13
    assert off[code(b"ACGT") + 1] - off[code(b"ACGT")] == 2


def test_unique_placement():
    """GTTACGA = genome[5:12]: its four k-mers sit at 5, 6, 7, 8, all on
    diagonal 5; its reverse complement TCGTAAC shares no k-mer with the
    genome.  W = 14, band 1: pad = (14 - 7) // 2 = 3."""
    ix = sd.Index(UNIQUE, 4, 64)
    assert sd.seed_one(ix, b"GTTACGA", 1, 64, 1) == (5, 4, 4, False)
    assert sd.seed_one(ix, so.revcomp(b"GTTACGA"), 1, 64, 1) == (None, 0, 0, False)
    assert sd.place_one(ix, b"GTTACGA", True, 1, 64, 1, 1, 0) == (2, 4, 4, 0)
    # the reverse-complemented read is found through the reverse orientation only
    assert sd.place_one(ix, so.revcomp(b"GTTACGA"), True, 1, 64, 1, 1, 0) == (2, 4, 4, 1)
    assert sd.place_one(ix, so.revcomp(b"GTTACGA"), False, 1, 64, 1, 1, 0) == (-1, 0, 0, 0)
    # step 2: offsets 0 and 2 only; step 64: offset 0 only
    assert sd.seed_one(ix, b"GTTACGA", 1, 64, 2) == (5, 2, 2, False)
    assert sd.seed_one(ix, b"GTTACGA", 1, 64, 64) == (5, 1, 1, False)
    # window 20: pad = (20 - 7) // 2 = 6 -> max(0, 5 - 6); band 16: pad = (14 - 22) < 0 -> 0
    assert sd.place_one(ix, b"GTTACGA", False, 1, 64, 1, 1, 20)[0] == 0
    assert sd.place_one(ix, b"GTTACGA", False, 16, 64, 1, 1, 0)[0] == 5


def test_equal_votes_take_the_smaller_diagonal():
    """ACGTAC occurs at 0 and at 8: D = {0, 0, 0, 8, 8, 8}."""
    ix = sd.Index(TWO_LOCI, 4, 64)
    assert sd.seed_one(ix, b"ACGTAC", 4, 64, 1) == (0, 3, 6, False)
    assert sd.seed_one(ix, b"ACGTAC", 8, 64, 1) == (0, 3, 6, False)     # [0, 8) stops short of 8
    assert sd.seed_one(ix, b"ACGTAC", 9, 64, 1) == (0, 6, 6, False)
    # its reverse complement GTACGT: GTAC {2, 10} - 0, TACG {3} - 1, ACGT {0, 8} - 2: D = {-2, 2, 2, 6, 10}
    assert sd.seed_one(ix, b"GTACGT", 4, 64, 1) == (2, 2, 5, False)
    assert sd.place_one(ix, b"ACGTAC", True, 4, 64, 1, 1, 0) == (0, 3, 6, 0)


def test_orientation_tie_goes_forward():
    #  0 AACC  1 ACCA  2 CCAG  3 CAGG  4 AGGT  5 GGTT  6 GTTA
    ix = sd.Index(b"AACCAGGTTA", 4, 64)
    assert sd.seed_one(ix, b"AACC", 1, 64, 1) == (0, 1, 1, False)
    assert sd.seed_one(ix, b"GGTT", 1, 64, 1) == (5, 1, 1, False)
    assert sd.place_one(ix, b"AACC", True, 1, 64, 1, 1, 0) == (0, 1, 1, 0)      # 1 : 1 -> forward, d0 = 0
    assert sd.place_one(ix, b"GGTT", True, 1, 64, 1, 1, 0) == (3, 1, 1, 0)      # pad (8 - 4) // 2 = 2
    # a palindrome is its own reverse complement
    assert so.revcomp(b"ACGTACGT") == b"ACGTACGT"
    ix = sd.Index(TWO_LOCI, 4, 64)
    assert sd.place_one(ix, b"ACGTACGT", True, 4, 64, 1, 1, 0)[3] == 0


def test_cap_rule():
    """ACGTAC on TWO_LOCI: c = 2, 2, 2 and P = 2, 4, 6."""
    ix = sd.Index(TWO_LOCI, 4, 64)
    assert sd.seed_one(ix, b"ACGTAC", 4, 6, 1) == (0, 3, 6, False)      # P = cap contributes
    assert sd.seed_one(ix, b"ACGTAC", 4, 5, 1) == (0, 2, 4, True)       # P = cap + 1 does not
    assert sd.seed_one(ix, b"ACGTAC", 4, 4, 1) == (0, 2, 4, True)
    assert sd.seed_one(ix, b"ACGTAC", 4, 1, 1) == (None, 0, 0, True)
    assert sd.place_one(ix, b"ACGTAC", False, 4, 5, 1, 1, 0) == (0, 2, 4, 2)
    assert sd.place_one(ix, b"ACGTAC", False, 4, 1, 1, 1, 0) == (-1, 0, 0, 2)


def test_max_occ():
    """CAAAAAAAC: AAAA at 1, 2, 3, 4."""
    at = sd.Index(b"CAAAAAAAC", 4, 4)
    assert at.n_masked == 0 and at.pos.tolist() == [1, 2, 3, 4, 5, 0]      # AAAA 0, AAAC 1 (at 5), CAAA 64 (at 0)
    over = sd.Index(b"CAAAAAAAC", 4, 3)
    assert over.n_masked == 1 and over.pos.tolist() == [5, 0]
    assert sd.seed_one(at, b"AAAA", 2, 64, 1) == (1, 2, 4, False)
    assert sd.seed_one(over, b"AAAA", 2, 64, 1) == (None, 0, 0, False)


def test_negative_diagonal_is_clamped():
    """TTACGTAC overhangs the genome start by two bases: TACG {3} - 1,
    ACGT {0, 8} - 2, CGTA {1, 9} - 3, GTAC {2, 10} - 4: D = {-2 x 3, 2, 6 x 3}."""
    ix = sd.Index(TWO_LOCI, 4, 64)
    assert sd.seed_one(ix, b"TTACGTAC", 4, 64, 1) == (-2, 3, 7, False)
    assert sd.place_one(ix, b"TTACGTAC", False, 4, 64, 1, 1, 0) == (0, 3, 7, 0)
    assert sd.place_one(ix, b"TTACGTAC", False, 16, 64, 1, 1, 0)[0] == 0     # pad 0: max(0, -2)


def test_min_votes():
    ix = sd.Index(TWO_LOCI, 4, 64)
    assert sd.place_one(ix, b"ACGTAC", False, 4, 64, 1, 3, 0) == (0, 3, 6, 0)
    assert sd.place_one(ix, b"ACGTAC", False, 4, 64, 1, 4, 0) == (-1, 3, 6, 0)
    assert sd.place_one(ix, b"ACG", False, 4, 64, 1, 1, 0) == (-1, 0, 0, 0)      # L < k
    assert sd.place_one(ix, b"", True, 4, 64, 1, 1, 0) == (-1, 0, 0, 0)


def test_batch_form_and_k14():
    rng = np.random.default_rng(7)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 5000)]
    ix = sd.Index(g, 14, 64)
    R = np.zeros((3, 64), np.uint8)
    R[0, :50] = g[1000:1050]
    R[1, :40] = np.frombuffer(so.revcomp(g[2000:2040].tobytes()), np.uint8)
    rl = np.array([50, 40, 0], np.uint16)
    wp, votes, hits, flags = sd.place(ix, R, rl, band=16, window=0)
    # pad = (100 - 65) // 2 = 17, (80 - 55) // 2 = 12
    assert wp.tolist() == [1000 - 17, 2000 - 12, -1] and votes.tolist() == [37, 27, 0] and flags.tolist() == [0, 1, 0]
    assert hits.tolist() == [37, 27, 0]


@pytest.mark.parametrize("k,least", [(12, 69), (10, 81)])
def test_lane_reads_are_placed(k, least):
    """Lane file 0 of the default dataset, 2,000 reads of 150 bp: every
    related read's origin lies inside the chosen window with 8 bases to spare
    on both sides.  The smallest winning vote is 69 (k = 12) and 81 (k = 10);
    the largest vote of an unrelated read, over both orientations, is 7 and 9
    (printed, not a condition)."""
    from mini_parallel_amd import synthetic as syn
    g = syn.wgs_genome()
    b, _, _ = syn._lane_reads(g, 0, 2000, 150, 2.0, 1004)
    ix = sd.Index(g, k, 64)
    wp, votes, hits, flags = sd.place(ix, b.reads, b.read_len, both=True, band=16, cap=4096)
    related = b.pos >= 0
    origin = b.pos + (b.win_len.astype(np.int64) - 150) // 2
    W = np.minimum(2 * b.read_len.astype(np.int64), 4096)
    print("related", int(related.sum()), "least vote", int(votes[related].min()), "most unrelated",
          int(votes[~related].max()))
    assert int(related.sum()) == 1793
    ok = (wp >= 0) & (origin >= wp + 8) & (origin <= wp + W - 8 - 150)
    assert ok[related].all(), np.flatnonzero(related & ~ok)[:8]
    assert int(votes[related].min()) == least
    assert not (flags[related] & 1).any()
