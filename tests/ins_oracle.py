"""The inserted sequences of include/msw.h ("Pileup", "Inserted sequences"),
restated: the walk of tests/pileup_oracle.py with one (len, flags, seq) per I
run in a dict of lists, collections.Counter for the vote, Python ints for seq.
It shares nothing with the kernels (msw_ins.hip).
"""
from collections import Counter

import numpy as np

from pileup_oracle import OP_D, OP_I, OP_M, OP_S

OTHER, LONG = 1, 2
_COMP = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCAtgca")}
SITE_FIELDS = ("pos", "events", "alleles", "best_count", "second_count", "best_len", "reserved", "seq")


def events(glen, rows, read_len, ref_pos, nm, cigars, strand=None, mapq=None, min_mapq=0, flip=False, into=None):
    """{pos: [(len, flags, seq), ...]} of one batch.  flip: the rows are the
    reads as given, base t of a strand-1 row is comp(row[read_len - 1 - t])."""
    out = {} if into is None else into
    for p in range(len(ref_pos)):
        ops = cigars[p]
        if not (int(ref_pos[p]) >= 0 and int(nm[p]) >= 0 and ops is not None and len(ops) > 0
                and (mapq is None or int(mapq[p]) >= min_mapq)):
            continue
        rl = int(read_len[p])
        mirror = flip and strand is not None and int(strand[p]) != 0
        i, g = 0, int(ref_pos[p])
        for word in ops:
            ln, kind = int(word) >> 4, int(word) & 15
            if kind in (OP_S, OP_M):
                i += ln
            if kind in (OP_M, OP_D):
                g += ln
            if kind == OP_I:
                if 0 <= g - 1 < glen:
                    flags, seq = (LONG if ln > 32 else 0), 0
                    for k in range(min(ln, 32)):
                        t = i + k
                        b = 0 if t >= rl else int(rows[p][rl - 1 - t] if mirror else rows[p][t])
                        b = _COMP.get(b, b) if mirror else b
                        if t >= rl or b not in b"ACGT":
                            flags |= OTHER
                        else:
                            seq |= b"ACGT".index(b) << 2 * k
                    out.setdefault(g - 1, []).append((ln, flags, 0 if flags else seq))
                i += ln
    return out


def table(ev):
    """The site records, in ascending pos, as tuples in SITE_FIELDS order."""
    out = []
    for pos in sorted(ev):
        votes = Counter(ev[pos])
        plain = sorted(((-c, ln, seq) for (ln, flags, seq), c in votes.items() if flags == 0))
        best = plain[0] if plain else (0, 0, 0)
        out.append((pos, len(ev[pos]), len(votes), -best[0], -plain[1][0] if len(plain) > 1 else 0, best[1], 0, best[2]))
    return out


def as_tuples(rec):
    """A structured array of msw_ins_site_t as the tuples table() gives."""
    return [tuple(int(r[f]) for f in SITE_FIELDS) for r in np.asarray(rec)]
