"""Pairs restated on the host (include/msw.h, "Pairs").

TEST INFRASTRUCTURE ONLY.  Plain Python integers on top of mapq_oracle (candidates) and strand_oracle (records).
"""
from typing import NamedTuple

import numpy as np

import aln_oracle as ao
import mapq_oracle as mo
import seed_oracle as sd
import strand_oracle as so

NONE = 3      # the pseudo-candidate, after 0, 1 and 2 in the tie order


class Params(NamedTuple):
    min_ins: int = 1
    max_ins: int = 1000
    pair_bonus: int = 17
    rescue_min_score: int = 60
    slack: int = 16


class Cand(NamedTuple):
    score: int
    strand: int
    win_pos: int
    end_i: int
    end_j: int


def exists(c):
    return c is not None and c.win_pos >= 0 and c.score > 0


def span(c, L):
    right = c.win_pos + (c.end_j + 1) + (L - 1 - c.end_i)
    return right - L, right


def proper(c1, L1, c2, L2, q):
    """(proper, opposite strands, tlen) of two existing candidates."""
    if c1.strand == c2.strand:
        return False, False, 0
    (lf, rf), (lr, rr) = (span(c1, L1), span(c2, L2)) if c1.strand == 0 else (span(c2, L2), span(c1, L1))
    tlen = rr - lf
    return lf <= lr and rf <= rr and q.min_ins <= tlen <= q.max_ins, True, tlen


class Chosen(NamedTuple):
    c: tuple            # per mate 0, 1, 2 or NONE
    cand: tuple         # per mate, as reported: 0 for NONE
    sub_score: tuple
    mapq: tuple
    proper: bool
    tlen: int
    flags: int


def choose(cands1, L1, cands2, L2, match, q):
    """cands1 / cands2: lists of K Cand (None or a non-existing one: missing)."""
    ids = lambda cs: [k for k, c in enumerate(cs) if exists(c)] + [NONE]
    table = {}
    for i in ids(cands1):
        for j in ids(cands2):
            s1 = cands1[i].score if i != NONE else 0
            s2 = cands2[j].score if j != NONE else 0
            pr = (False, False, 0) if NONE in (i, j) else proper(cands1[i], L1, cands2[j], L2, q)
            table[(i, j)] = (s1 + s2 + (q.pair_bonus if pr[0] else 0), pr)
    best = min(table, key=lambda ij: (-table[ij][0], ij))          # the largest S, then the smallest (c1, c2)
    S, (is_proper, opposite, tlen) = table[best]
    sub, mq = [], []
    for m, (cs, L) in enumerate(((cands1, L1), (cands2, L2))):
        others = [c.score for k, c in enumerate(cs) if k != best[m] and exists(c)]
        sub.append(max(others, default=0))
        own = cs[best[m]].score if best[m] != NONE else 0
        alt = [v[0] for ij, v in table.items() if ij[m] != best[m]]
        mq.append(0 if own <= 0 or match * L == 0 or not alt else min(60, 120 * (S - max(alt)) // (match * L)))
    tlen = max(-(2 ** 31 - 1), min(2 ** 31 - 1, tlen)) if opposite else 0
    flags = (1 if is_proper else 0) | (2 if best[0] == 2 else 0) | (4 if best[1] == 2 else 0)
    return Chosen(best, tuple(0 if c == NONE else c for c in best), tuple(sub), tuple(mq), is_proper, tlen, flags)


def rescue_pos(cands1, L1, cands2, L2, q):
    """The plan: the K = 2 choice, then each mate's rescue window position."""
    ch = choose(cands1[:2], L1, cands2[:2], L2, 1, q)
    out = []
    for m, (L, partner, Lp) in enumerate(((L1, cands2, L2), (L2, cands1, L1))):
        a = ch.c[1 - m]
        if ch.proper or a == NONE or partner[a].score < q.rescue_min_score:
            out.append(-1)
            continue
        left, right = span(partner[a], Lp)
        wp = left + q.min_ins - L - q.slack if partner[a].strand == 0 else right - q.max_ins - q.slack
        out.append(max(0, wp))
    return out


rescue_on = lambda q: q.rescue_min_score != 0 or q.slack != 0
rescue_window = lambda q, max_read_len: q.max_ins - q.min_ins + max_read_len + 2 * q.slack


def hist_adds(tlen, mapq1, mapq2, min_mapq):      # the reported tlen: 0 unless both exist on opposite strands
    return 0 < tlen < 4096 and mapq1 >= min_mapq and mapq2 >= min_mapq


def bounds(hist):
    hist = [int(v) for v in hist]
    N = sum(hist)
    assert N > 0
    q = []
    for need in (-(-N // 4), -(-N // 2), -(-3 * N // 4)):
        cum = 0
        for k, v in enumerate(hist):
            cum += v
            if cum >= need:
                q.append(k)
                break
    iqr = q[2] - q[0]
    return max(1, q[0] - 3 * iqr), min(4095, q[2] + 3 * iqr), q[1]


def map_pairs(genome, index, reads, scheme, q, band=16, cap=4096, step=1, min_votes=1, window=0, sep=0):
    """msw_map_pairs: (mapq_oracle.Mapped per row, flags per pair, tlen per pair)."""
    g = np.frombuffer(genome, np.uint8)
    rl = [len(r) for r in reads]
    c0, c1 = mo.candidates(index, reads, rl, True, band, cap, step, min_votes, window, sep)
    recs = []
    for wp in (c0[0], c1[0]):
        wins = [ao.window_of(g, int(p), sd.window_want(window, len(r))).tobytes() for p, r in zip(wp, reads)]
        recs.append((so.records(reads, wins, wp, scheme), [int(p) for p in wp]))
    as_cand = lambda rec, wp: Cand(rec.score, rec.strand, wp, rec.end_i, rec.end_j)
    cands = [[as_cand(rc[p], wp[p]) for rc, wp in recs] for p in range(len(reads))]
    if rescue_on(q):
        wr = rescue_window(q, max(rl))
        wp2 = []
        for p in range(0, len(reads), 2):
            wp2 += rescue_pos(cands[p], rl[p], cands[p + 1], rl[p + 1], q)
        wins = [ao.window_of(g, p, wr).tobytes() for p in wp2]
        recs.append((so.records(reads, wins, wp2, scheme), wp2))
        for p in range(len(reads)):
            cands[p].append(as_cand(recs[2][0][p], wp2[p]))
    out, flags, tlen = [], [], []
    for p in range(0, len(reads), 2):
        ch = choose(cands[p], rl[p], cands[p + 1], rl[p + 1], scheme[0], q)
        for m in (0, 1):
            # "none": score 0, candidate 0's other results stay
            w = recs[0][0][p + m]._replace(score=0) if ch.c[m] == NONE else recs[ch.c[m]][0][p + m]
            out.append(mo.Mapped(w.score, w.end_i, w.end_j, w.strand, w.ref_pos, w.nm, w.ops, ch.mapq[m],
                                 ch.sub_score[m], ch.cand[m]))
        flags.append(ch.flags)
        tlen.append(ch.tlen)
    return out, flags, tlen
