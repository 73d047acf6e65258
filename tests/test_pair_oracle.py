"""tests/pair_oracle.py on hand-worked cases (include/msw.h, "Pairs"), and the
host-only msw_insert_bounds beside it.  No GPU.
"""
import numpy as np
import pytest

import pair_oracle as po

L = 100


def at(left, strand, score, win_pos=None, length=L):
    """A gap-free full-length candidate whose oriented read starts at `left`."""
    w = max(0, left - 20) if win_pos is None else win_pos
    return po.Cand(score, strand, w, length - 1, left + length - 1 - w)


@pytest.mark.parametrize("bonus,c,flags,tlen,mapq", [(10, (0, 0), 0, -3600, (0, 60)), (11, (1, 0), 1, 400, (0, 60)),
                                                     (60, (1, 0), 1, 400, (30, 60))])
def test_a_proper_pair_wins_exactly_when_the_bonus_exceeds_the_gap(bonus, c, flags, tlen, mapq):
    m1 = [at(5000, 0, 200), at(1000, 0, 190)]
    m2 = [at(1300, 1, 200), None]
    ch = po.choose(m1, L, m2, L, 2, po.Params(300, 500, bonus, 0, 0))
    # S(0, 0) = 400, S(1, 0) = 390 + bonus; mate 1's alternative is the other one of the two, mate 2's is "none"
    assert (ch.c, ch.flags, ch.tlen, ch.mapq, ch.sub_score) == (c, flags, tlen, mapq, (190 if c[0] == 0 else 200, 0))


def test_ties_none_and_same_strand():
    q = po.Params(300, 500, 17, 0, 0)
    same = [at(1000, 0, 150), at(3000, 0, 150)]
    ch = po.choose(same, L, same, L, 2, q)
    assert (ch.c, ch.cand, ch.proper, ch.tlen, ch.mapq, ch.sub_score) == ((0, 0), (0, 0), False, 0, (0, 0), (150, 150))
    # a mate without candidates takes "none": reported as 0, mapq 0; its partner's alternative is (none, none)
    ch = po.choose([at(1000, 0, 200), None], L, [None, po.Cand(0, 0, 700, -1, -1)], L, 2, q)
    assert (ch.c, ch.cand, ch.mapq, ch.sub_score, ch.flags, ch.tlen) == ((0, po.NONE), (0, 0), (60, 0), (0, 0), 0, 0)
    # a positive score at win_pos -1 is no candidate either
    assert po.choose([po.Cand(9, 0, -1, 3, 3)], L, [None], L, 2, q).c == (po.NONE, po.NONE)


@pytest.mark.parametrize("right,ok", [(1299, False), (1300, True), (1500, True), (1501, False)])
def test_insert_bounds_are_inclusive(right, ok):
    q = po.Params(300, 500, 17, 0, 0)
    f, r = at(1000, 0, 200), at(right - L, 1, 200)
    assert po.proper(f, L, r, L, q) == (ok, True, right - 1000)
    assert po.proper(r, L, f, L, q) == (ok, True, right - 1000)      # whichever mate is the forward one
    assert po.choose([r], L, [f], L, 2, q).flags == int(ok)
    # the reverse mate to the left of the forward one: not proper, whatever the distance
    assert po.proper(at(1000, 1, 200), L, at(1400, 0, 200), L, q)[0] is False


def test_spans_and_rescue_windows():
    assert po.span(at(1000, 0, 200), L) == (1000, 1100) and po.span(at(5, 1, 200, win_pos=0), L) == (5, 105)
    # the best cell 10 bases before the read's end, the first base 7 before the window: left_u is negative
    assert po.span(po.Cand(150, 0, 0, 89, 82), L) == (-7, 93)
    q = po.Params(300, 500, 17, 100, 10)
    none = [None, None]
    # anchor on strand 0 at 1000: the mate (80 bases) ends in [1300, 1500]
    assert po.rescue_pos([at(1000, 0, 200), None], L, none, 80, q) == [-1, 1000 + 300 - 80 - 10]
    # anchor on strand 1 ending at 1400: the mate starts in [900, 1100]
    assert po.rescue_pos(none, 80, [at(1300, 1, 200), None], L, q) == [1400 - 500 - 10, -1]
    assert po.rescue_pos(none, 80, [at(300, 1, 200), None], L, q) == [0, -1]           # 400 - 510, clamped
    assert po.rescue_pos(none, 80, [at(300, 1, 99), None], L, q) == [-1, -1]           # below rescue_min_score
    # an improper pair: each mate is searched for near the other; a proper one: neither
    far = po.rescue_pos([at(1000, 0, 200), None], L, [at(3000, 1, 200), None], L, q)
    assert far == [3100 - 510, 1000 + 300 - 100 - 10]
    assert po.rescue_pos([at(1000, 0, 200), None], L, [at(1300, 1, 200), None], L, q) == [-1, -1]
    assert po.rescue_window(q, 100) == 200 + 100 + 20 and po.rescue_on(q) and not po.rescue_on(po.Params(1, 9, 0, 0, 0))


def test_histogram_rule_and_bounds():
    import mini_parallel_amd as mpa
    assert [po.hist_adds(t, 30, 20, 20) for t in (0, 1, 4095, 4096, -5)] == [False, True, True, False, False]
    assert not po.hist_adds(400, 19, 60, 20) and not po.hist_adds(400, 60, 19, 20)
    h = np.zeros(4096, np.uint32)
    h[[100, 200, 300]] = 1, 2, 1           # N = 4: the counts 1, 2, 3 are reached at 100, 200, 200
    assert po.bounds(h) == mpa.insert_bounds(h) == (1, 500, 200)
    h[:] = 0
    h[[300, 310, 320]] = 10, 10, 20        # N = 40: 10, 20, 30 are reached at 300, 310, 320
    assert po.bounds(h) == mpa.insert_bounds(h) == (240, 380, 310)
    h[:] = 0
    h[4000] = 7
    assert po.bounds(h) == mpa.insert_bounds(h) == (4000, 4000, 4000)
    with pytest.raises(mpa.MswError) as e:          # N = 0
        mpa.insert_bounds(np.zeros(4096, np.uint32))
    assert e.value.code == -1
