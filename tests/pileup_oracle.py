"""The pileup of include/msw.h ("Pileup"), restated column by column.

Plain Python over numpy arrays: one increment per counted column, in the order
the definition walks them.  It shares nothing with the kernels' difference
form (msw_pileup.hip), so the two can be compared value for value.
"""
import numpy as np

CHANNELS = 8
CH_OTHER, CH_DEL, CH_INS, CH_REV = 4, 5, 6, 7
OP_M, OP_I, OP_D, OP_S = 0, 1, 2, 4
_CODE = np.full(256, CH_OTHER, np.int64)
for _k, _b in enumerate(b"ACGT"):
    _CODE[_b] = _k


def code(byte) -> int:
    """A 0, C 1, G 2, T 3 (upper case only), anything else 4."""
    return int(_CODE[int(byte)])


def op(length, kind) -> int:
    return int(length) << 4 | {"M": OP_M, "I": OP_I, "D": OP_D, "S": OP_S}.get(kind, kind)


def cigar(text) -> np.ndarray:
    """"3S5M2I" -> packed ops."""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(op(int(num), ch))
            num = ""
    return np.array(out, np.uint32)


def new_counts(glen) -> np.ndarray:
    return np.zeros((glen, CHANNELS), np.uint32)


def add(counts, rows, read_len, ref_pos, nm, cigars, strand=None, mapq=None, min_mapq=0):
    """Adds the batch's records to counts[glen][8] in place; returns
    (reads_used, reads_skipped).  rows[p] are the bytes the CIGAR of read p
    refers to (any sequence of byte values at least read_len[p] long)."""
    glen = counts.shape[0]
    used = skipped = 0
    for p in range(len(ref_pos)):
        ops = cigars[p]
        counted = (int(ref_pos[p]) >= 0 and int(nm[p]) >= 0 and ops is not None and len(ops) > 0
                   and (mapq is None or int(mapq[p]) >= min_mapq))
        if not counted:
            skipped += 1
            continue
        used += 1
        row, rl = rows[p], int(read_len[p])
        rev = strand is not None and int(strand[p]) != 0
        i, g = 0, int(ref_pos[p])
        for word in ops:
            ln, kind = int(word) >> 4, int(word) & 15
            if kind == OP_S:
                i += ln
            elif kind == OP_M:
                for k in range(ln):
                    if 0 <= g + k < glen and i + k < rl:
                        counts[g + k, code(row[i + k])] += 1
                        if rev:
                            counts[g + k, CH_REV] += 1
                i += ln
                g += ln
            elif kind == OP_I:
                if 0 <= g - 1 < glen:
                    counts[g - 1, CH_INS] += 1
                i += ln
            elif kind == OP_D:
                for k in range(ln):
                    if 0 <= g + k < glen:
                        counts[g + k, CH_DEL] += 1
                g += ln
    return used, skipped


def pileup(genome, rows, read_len, ref_pos, nm, cigars, strand=None, mapq=None, min_mapq=0):
    """-> (counts, reads_used, reads_skipped) of one batch over `genome`."""
    counts = new_counts(len(genome))
    used, skipped = add(counts, rows, read_len, ref_pos, nm, cigars, strand, mapq, min_mapq)
    return counts, used, skipped


def depth(counts) -> np.ndarray:
    return counts[:, :6].astype(np.uint64).sum(axis=1)


def summary(counts, genome, min_depth=1) -> dict:
    """covered, depth_sum, max_depth, minority_ref of finished counts."""
    assert min_depth >= 1
    g = np.frombuffer(bytes(genome), np.uint8) if isinstance(genome, (bytes, bytearray)) else np.asarray(genome, np.uint8)
    covered = depth_sum = max_depth = minority = 0
    for pos in range(counts.shape[0]):
        d = sum(int(counts[pos, ch]) for ch in range(6))
        covered += d > 0
        depth_sum += d
        max_depth = max(max_depth, d)
        if d >= min_depth and 2 * int(counts[pos, code(g[pos])]) < d:
            minority += 1
    return {"covered": covered, "depth_sum": depth_sum, "max_depth": max_depth, "minority_ref": minority}
