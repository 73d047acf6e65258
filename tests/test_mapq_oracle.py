"""tests/mapq_oracle.py against hand-worked cases of the contract
(include/msw.h, "Candidates and mapping quality"), and the rule itself on a
genome with planted repeats.  CPU only."""
import numpy as np
import pytest

import mapq_oracle as mo
import seed_oracle as sd
import strand_oracle as so

ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---------------------------------------------------------------------------
# 1. one orientation: the second band
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1, -1])
def test_exactly_sep_is_admissible(sign):
    band, sep = 16, 300
    first = [1000] * 5
    assert mo.two_bands(sorted(first + [1000 + sign * sep] * 3), band, sep) == ((1000, 5), (1000 + sign * sep, 3))
    assert mo.two_bands(sorted(first + [1000 + sign * (sep - 1)] * 3), band, sep) == ((1000, 5), (None, 0))
    assert mo.admissible(1000 + sign * sep, 1000, sep) and not mo.admissible(1000 + sign * (sep - 1), 1000, sep)


def test_band_below_the_excluded_range_is_clipped():
    """band 16, sep 20, first band at 100.  70 is admissible, 82 is not
    (18 < 20): the band [70, 86) holds both but counts one."""
    D = sorted([100] * 5 + [70, 82])
    assert mo.best_band(D, 16) == (100, 5)
    assert mo.best_band([70, 82], 16) == (70, 2)             # what an unclipped count would give
    assert mo.two_bands(D, 16, 20) == ((100, 5), (70, 1))
    # 80 = 100 - 20 is admissible and inside [70, 86): two votes
    assert mo.two_bands(sorted(D + [80]), 16, 20) == ((100, 5), (70, 2))


def test_second_band_takes_the_smaller_start_on_ties_and_none_when_empty():
    assert mo.two_bands([], 16, 16) == ((None, 0), (None, 0))
    assert mo.two_bands([5, 5, 6], 16, 16) == ((5, 3), (None, 0))
    assert mo.two_bands(sorted([500] * 4 + [900, 901] + [100, 103]), 16, 300) == ((500, 4), (100, 2))
    # negative diagonals
    assert mo.two_bands(sorted([-40] * 3 + [-400, -399]), 16, 300) == ((-40, 3), (-400, 2))


# ---------------------------------------------------------------------------
# 2. the merge
# ---------------------------------------------------------------------------
NONE = (None, 0)


def test_merge_forward_only_and_empty():
    assert mo.merge((NONE, NONE), None, 300, 1) == ((0, None, 0), (0, None, 0))
    assert mo.merge(((1000, 10), (5000, 6)), None, 300, 1) == ((0, 1000, 10), (0, 5000, 6))
    assert mo.merge(((1000, 10), NONE), None, 300, 1) == ((0, 1000, 10), (0, None, 0))


def test_merge_other_first_inadmissible_second_admissible():
    fwd, rev = ((1000, 10), NONE), ((1100, 8), (2000, 4))
    assert mo.merge(fwd, rev, 300, 1) == ((0, 1000, 10), (1, 2000, 4))
    # exactly sep away from d0: the other orientation's first band is taken
    assert mo.merge(fwd, ((1300, 8), (2000, 4)), 300, 1) == ((0, 1000, 10), (1, 1300, 8))
    assert mo.merge(fwd, ((1299, 8), (2000, 4)), 300, 1) == ((0, 1000, 10), (1, 2000, 4))
    # the other orientation's second band is admissible against its own first, not against d0
    assert mo.merge(fwd, ((1700, 8), (1200, 4)), 300, 1) == ((0, 1000, 10), (1, 1700, 8))
    assert mo.merge(fwd, ((700, 8), (1200, 4)), 300, 1) == ((0, 1000, 10), (1, 700, 8))
    assert mo.merge(fwd, ((800, 8), (1200, 4)), 300, 1) == ((0, 1000, 10), (0, None, 0))


def test_merge_three_way_tie():
    """Equal votes: forward before reverse, then the smaller diagonal."""
    assert mo.merge(((1000, 10), (5000, 6)), ((2000, 6), (3000, 6)), 300, 1) == ((0, 1000, 10), (0, 5000, 6))
    # the reverse orientation is candidate 0: forward holds two of the three
    assert mo.merge(((2000, 6), (3000, 6)), ((1000, 10), (5000, 6)), 300, 1) == ((1, 1000, 10), (0, 2000, 6))
    # reverse only in the tie: the smaller diagonal
    assert mo.merge(((1000, 10), NONE), ((4000, 6), (2000, 6)), 300, 1) == ((0, 1000, 10), (1, 2000, 6))
    # orientation tie for candidate 0 goes forward; the reverse first band is candidate 1
    assert mo.merge(((1000, 10), NONE), ((9000, 10), NONE), 300, 1) == ((0, 1000, 10), (1, 9000, 10))


def test_merge_min_votes():
    fwd, rev = ((1000, 10), (5000, 3)), ((7000, 4), (9000, 2))
    assert mo.merge(fwd, rev, 300, 1)[1] == (1, 7000, 4)
    assert mo.merge(fwd, rev, 300, 4)[1] == (1, 7000, 4)
    assert mo.merge(fwd, rev, 300, 5)[1] == (0, None, 0)
    assert mo.merge(fwd, None, 300, 4)[1] == (0, None, 0)
    # candidate 0 below min_votes: nothing else can reach it either
    assert mo.merge(fwd, rev, 300, 11) == ((0, 1000, 10), (0, None, 0))


# ---------------------------------------------------------------------------
# 3. selection and mapping quality
# ---------------------------------------------------------------------------
def test_select():
    assert mo.select(10, 11) == (1, 11, 10)
    assert mo.select(10, 10) == (0, 10, 10)
    assert mo.select(10, 0) == (0, 10, 0)
    assert mo.select(0, 0) == (0, 0, 0)


def test_mapq_values():
    assert mo.mapq(0, 0, 2, 150) == 0                    # s1 = 0
    assert mo.mapq(-3, -7, 2, 150) == 0
    assert mo.mapq(100, 150, 2, 150) == 0                # s2 > s1: clamped to s1
    assert mo.mapq(100, 100, 2, 150) == 0                # s2 = s1
    assert mo.mapq(300, 0, 2, 150) == 60                 # 120: the cap
    assert mo.mapq(300, -9, 2, 150) == 60                # a negative sub-optimal score counts as 0
    assert mo.mapq(200, 150, 2, 150) == 20               # 6000 / 300
    assert mo.mapq(200, 151, 2, 150) == 19               # 5880 / 300 = 19.6: the floor
    assert mo.mapq(149, 0, 2, 150) == 59                 # 17880 / 300 = 59.6
    assert mo.mapq(150, 0, 2, 150) == 60
    assert mo.mapq(5, 0, 2, 0) == 0 and mo.mapq(5, 0, 0, 150) == 0
    assert mo.mapq(2 ** 31 - 1, 0, 1, 65535) == 60       # 64-bit intermediates


# ---------------------------------------------------------------------------
# 4. a tiny genome end to end: placement, flags, sep = 0
# ---------------------------------------------------------------------------
def rand_seq(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def test_candidates_one_on_a_two_copy_genome():
    rng = np.random.default_rng(31)
    g = bytearray(rand_seq(rng, 6000))
    g[4000:4100] = g[1000:1100]
    g = bytes(g)
    ix = sd.Index(g, 8, 64)
    read = g[1010:1090]
    kw = dict(band=16, cap=4096, step=1, min_votes=1, window=0)
    c0, c1 = mo.candidates_one(ix, read, True, sep=0, **kw)
    assert c0 == sd.place_one(ix, read, True, **kw)
    pad = (160 - (80 + 15)) // 2
    assert c0[0] == 1010 - pad and c1[0] == 4010 - pad and c0[1] == c1[1] == 73 and c1[2] == 0
    # the reverse complement: both candidates come from the reverse orientation
    c0, c1 = mo.candidates_one(ix, so.revcomp(read), True, sep=0, **kw)
    assert c0[0] == 1010 - pad and c0[3] & 1 and c1 == (4010 - pad, 73, 1)
    # a separation beyond the genome: no second candidate
    assert mo.candidates_one(ix, read, True, sep=10000, **kw)[1] == (-1, 0, 0)
    # sep = 0 is max(W, band): a short read's W = 2 L = 16 < band 40
    assert mo.effective_sep(0, 40, 0, 8) == 40 and mo.effective_sep(0, 16, 0, 150) == 300
    assert mo.effective_sep(0, 16, 500, 150) == 500 and mo.effective_sep(77, 16, 500, 150) == 77
    # forward only, unrelated read, empty read
    assert mo.candidates_one(ix, b"", False, sep=0, **kw) == ((-1, 0, 0, 0), (-1, 0, 0))
    assert mo.candidates_one(ix, read, False, sep=300, **kw)[1] == (4010 - pad, 73, 0)


# ---------------------------------------------------------------------------
# 5. the rule on planted repeats: 1 Mbase, k = 12, max_occ 64, band 16, sep 300
# ---------------------------------------------------------------------------
def test_planted_repeats():
    """Three sources of 60 reads (150 bp, 1 % substitutions, every other one
    reverse-complemented): a segment with an exact copy 500,000 bases away, a
    segment whose copy differs in every 33rd base (3 %, evenly spread so that
    every read spans at least four differences), and unique sequence."""
    rng = np.random.default_rng(20261)
    g = np.frombuffer(rand_seq(rng, 1 << 20), np.uint8).copy()
    g[600000:620000] = g[100000:120000]
    div = g[200000:220000].copy()
    at = np.arange(7, 20000, 33)
    div[at] = ACGT[(np.searchsorted(ACGT, div[at]) + rng.integers(1, 4, at.shape[0])) % 4]
    g[700000:720000] = div
    assert (g[700000:720000] != g[200000:220000]).sum() == at.shape[0]
    g = g.tobytes()
    ix = sd.Index(g, 12, 64)
    band, sep = 16, 300

    def reads_from(lo):
        out = []
        for p in range(60):
            a = lo + int(rng.integers(0, 20000 - 150))
            r = np.frombuffer(g[a:a + 150], np.uint8).copy()
            hit = rng.random(150) < 0.01
            r[hit] = ACGT[(np.searchsorted(ACGT, r[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
            out.append((a, so.revcomp(r.tobytes()) if p % 2 else r.tobytes(), p % 2))
        return out

    def cands(read):
        f = mo.two_bands(mo.diagonals(ix, read, 4096, 1)[0], band, sep)
        r = mo.two_bands(mo.diagonals(ix, so.revcomp(read), 4096, 1)[0], band, sep)
        return mo.merge(f, r, sep, 1)

    first_votes = []
    # exact copy: the two candidates are the two copies, in the read's orientation
    for a, read, rev in reads_from(100000):
        (o0, d0, v0), (o1, d1, v1) = cands(read)
        first_votes.append(v0)
        assert (o0, o1) == (rev, rev) and abs(d0 - a) < band and abs(d1 - (a + 500000)) < band, (a, d0, d1)
    # diverged copy: candidate 0 at the origin, candidate 1 at the copy with fewer votes
    for a, read, rev in reads_from(200000):
        (o0, d0, v0), (o1, d1, v1) = cands(read)
        first_votes.append(v0)
        assert (o0, o1) == (rev, rev) and abs(d0 - a) < band and abs(d1 - (a + 500000)) < band, (a, d0, d1)
        assert 0 < v1 < v0, (a, v0, v1)
    # unique sequence: only chance hits are left for candidate 1
    second_votes = []
    for a, read, rev in reads_from(300000):
        (o0, d0, v0), (o1, d1, v1) = cands(read)
        first_votes.append(v0)
        second_votes.append(v1)
        assert o0 == rev and abs(d0 - a) < band
    assert max(second_votes) < min(first_votes), (max(second_votes), min(first_votes))
