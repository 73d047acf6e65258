"""Candidates and mapping quality restated on the host (include/msw.h,
"Candidates and mapping quality").

TEST INFRASTRUCTURE ONLY.  Built on tests/seed_oracle.py (index, k-mer codes,
the cap rule) and tests/strand_oracle.py (reverse complement, both-strand
scores from the C oracle).  The second band is what the contract says it is:
the seed rule run again over the admissible diagonals alone, a filtered list,
where the kernel clips a search over the one sorted array.

    diagonals(index, read, cap, step) -> (sorted list of int, truncated)
    best_band(D, band) -> (d, votes) or (None, 0)
    admissible(e, d, sep) -> bool
    two_bands(D, band, sep) -> ((d1, v1), (d2, v2))
    merge(fwd, rev, band, sep, min_votes) -> dict: candidate 0 and candidate 1
    candidates_one(index, read, both, band, cap, step, min_votes, window, sep)
    candidates(index, reads, read_len, ...) -> (cand0 4 arrays, cand1 3 arrays)
    mapq(s1, sub, match, L) -> int
    select(s_p, s_a) -> (cand, score, sub_score)
    map_records(...) -> per-read records of the composition
"""
from typing import NamedTuple

import numpy as np

import aln_oracle as ao
import seed_oracle as sd
import strand_oracle as so


def diagonals(index, read, cap, step):
    """The multiset D of one orientation, ascending, and the truncated bit
    (steps 1-3 of "Placing reads")."""
    code, coded = sd.codes(read, index.k)
    if code.shape[0] == 0:
        return [], False
    coded = coded & (np.arange(code.shape[0]) % step == 0)
    st, cnt = index.lookup(code, coded)
    P = np.cumsum(cnt)
    D = []
    for i in np.flatnonzero((cnt > 0) & (P <= cap)):
        D.extend(int(p) - int(i) for p in index.pos[st[i]:st[i] + cnt[i]])
    return sorted(D), bool(P[-1] > cap)


def best_band(D, band):
    """Steps 4-6: the start of maximal count, the smallest on ties."""
    if len(D) == 0:
        return None, 0
    u, c = np.unique(np.asarray(D, np.int64), return_counts=True)
    upto = np.concatenate([[0], np.cumsum(c)])                # diagonals below u[j]
    v = upto[np.searchsorted(u, u + band, side="left")] - upto[:-1]
    j = int(np.argmax(v))                                     # the first maximum: the smallest start
    return int(u[j]), int(v[j])


def admissible(e, d, sep):
    return abs(e - d) >= sep


def two_bands(D, band, sep):
    """An orientation's first band, and its second: the seed rule over the
    diagonals admissible against the first."""
    assert sep >= band >= 1
    d1, v1 = best_band(D, band)
    if v1 == 0:
        return (None, 0), (None, 0)
    return (d1, v1), best_band([e for e in D if admissible(e, d1, sep)], band)


def merge(fwd, rev, sep, min_votes):
    """fwd / rev: two_bands of each orientation (rev None: forward only).
    Returns (orient0, d0, v0), (orient1, d1, v1) with d None where there is
    no such candidate; candidate 0 by today's orientation rule, before
    min_votes (placement applies it)."""
    o0 = 1 if rev is not None and rev[0][1] > fwd[0][1] else 0
    own, other = (rev, fwd) if o0 else (fwd, rev)
    d0, v0 = own[0]
    if v0 == 0:
        return (o0, None, 0), (0, None, 0)
    pool = [(o0, own[1])]
    if other is not None:
        pool += [(1 - o0, other[0]), (1 - o0, other[1])]
    ok = [(o, d, v) for o, (d, v) in pool if v >= min_votes and v > 0 and admissible(d, d0, sep)]
    if not ok:
        return (o0, d0, v0), (0, None, 0)
    ok.sort(key=lambda t: (-t[2], t[0], t[1]))      # votes, then forward first, then the smaller diagonal
    return (o0, d0, v0), ok[0]


def effective_sep(sep, band, window, L):
    return sep if sep else max(sd.window_want(window, L), band)


def position(d, L, band, window):
    pad = max(0, sd.window_want(window, L) - (L + band - 1)) // 2
    return max(0, d - pad)


def candidates_one(index, read, both, band, cap, step, min_votes, window, sep):
    """((win_pos, votes, hits, flags), (win_pos1, votes1, flags1)) of one read."""
    assert min_votes >= 1 and (sep == 0 or sep >= band)
    read = sd._arr(read).tobytes()
    L = len(read)
    s = effective_sep(sep, band, window, L)
    Df, tf = diagonals(index, read, cap, step)
    fwd, rev, Dr, tr = two_bands(Df, band, s), None, [], False
    if both:
        Dr, tr = diagonals(index, so.revcomp(read), cap, step)
        rev = two_bands(Dr, band, s)
    (o0, d0, v0), (o1, d1, v1) = merge(fwd, rev, s, min_votes)
    hits, trunc = (len(Dr), tr) if o0 else (len(Df), tf)
    wp0 = position(d0, L, band, window) if v0 >= min_votes and v0 > 0 else -1
    c0 = (wp0, v0, hits, o0 | (2 if trunc else 0))
    if d1 is None:
        return c0, (-1, 0, 0)
    return c0, (position(d1, L, band, window), v1, o1)


def candidates(index, reads, read_len, both=True, band=16, cap=4096, step=1, min_votes=1, window=0, sep=0):
    n = len(read_len)
    c0 = (np.empty(n, np.int64), np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint8))
    c1 = (np.empty(n, np.int64), np.empty(n, np.uint32), np.empty(n, np.uint8))
    for p in range(n):
        a, b = candidates_one(index, reads[p][:int(read_len[p])], both, band, cap, step, min_votes, window, sep)
        for arr, v in zip(c0 + c1, a + b):
            arr[p] = v
    return c0, c1


def mapq(s1, sub, match, L):
    """The uncalibrated heuristic of the contract, on Python integers."""
    if s1 <= 0 or match * L == 0:
        return 0
    s2 = min(max(sub, 0), s1)
    return min(60, (120 * (s1 - s2)) // (match * L))


def select(s_p, s_a):
    """(cand, score, sub_score): the alternate wins iff it scores strictly more."""
    return (1, s_a, s_p) if s_a > s_p else (0, s_p, s_a)


class Mapped(NamedTuple):
    score: int
    end_i: int
    end_j: int
    strand: int
    ref_pos: int
    nm: int
    ops: list
    mapq: int
    sub_score: int
    cand: int


def map_records(genome, index, reads, scheme, both, band=16, cap=4096, step=1, min_votes=1, window=0, sep=0):
    """The composition: both candidates scored against their windows (both
    strands through strand_oracle when `both`), the select, and the winner's
    record."""
    g = np.frombuffer(genome, np.uint8)
    rl = [len(r) for r in reads]
    c0, c1 = candidates(index, reads, rl, both, band, cap, step, min_votes, window, sep)
    recs = []
    for wp in (c0[0], c1[0]):
        wins = [ao.window_of(g, int(p), sd.window_want(window, len(r))).tobytes() for p, r in zip(wp, reads)]
        if both:
            recs.append(so.records(reads, wins, wp, scheme))
        else:
            recs.append([so.Record(r.score, r.end_i, r.end_j, 0, r.ref_pos, r.nm, r.ops)
                         for r in (ao.record(rd, w, int(p), *scheme) for rd, w, p in zip(reads, wins, wp))])
    out = []
    for p, (a, b) in enumerate(zip(*recs)):
        cand, s, sub = select(a.score, b.score)
        w = b if cand else a
        out.append(Mapped(w.score, w.end_i, w.end_j, w.strand, w.ref_pos, w.nm, w.ops,
                          mapq(s, sub, scheme[0], rl[p]), sub, cand))
    return out, c0, c1
